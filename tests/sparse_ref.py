"""Expected sparse distances for the tests (test infrastructure only).

The reference's sparse distance (ComputeDistanceHelper, include/space/space_sparse_vector.h:137-215) merges the two
id lists into union order (0 where an id is missing) and calls the dense function on the two union arrays.  This
module restates that for one query against many rows at once, in numpy:
  * the dense functions' SSE layout: lane = union position mod 4, products and sums rounded separately, lanes summed
    left to right (np.add.at accumulates in index order, in float32);
  * the scalar tail (the last union length mod 4 positions): the reference's build contracts it into fused
    multiply-adds, restated as a float64 product (exact for float32 inputs) plus a float64 add rounded to float32 --
    an FMA except for a very rare double rounding.  The CPU oracle (oracle/knn_oracle.c) does not contract, so
    orc.space_distance on the union arrays differs from the reference in the last bits of l2 / cosine / dot tails;
  * acos is libm's acosf, as in the reference.
For l1 / linf the oracle's formula is the same; distance_oracle() exposes that path as a cross-check.
"""
import ctypes as C

import numpy as np

from tests import orc

SPACES = ("cosinesimil_sparse", "angulardist_sparse", "negdotprod_sparse", "querynorm_negdotprod_sparse",
          "l1_sparse", "l2_sparse", "linf_sparse")
LP = {1.0: "l1_sparse", 2.0: "l2_sparse", -1.0: "linf_sparse"}
ORC_SPACE = {"l1_sparse": "l1", "l2_sparse": "l2", "linf_sparse": "linf", "cosinesimil_sparse": "cosinesimil",
             "angulardist_sparse": "angulardist", "negdotprod_sparse": "negdotprod"}
EPS = np.float32(np.finfo(np.float32).tiny * 2)
f32 = np.float32

_libm = C.CDLL("libm.so.6")
_libm.acosf.restype = C.c_float
_libm.acosf.argtypes = [C.c_float]
_acosf = np.frompyfunc(lambda v: _libm.acosf(float(v)), 1, 1)


def csr(rows):
    """list of (ids, values) -> (ptr int64 [n+1], ids uint32, vals float32)"""
    counts = np.array([len(r[0]) for r in rows], np.int64)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    ids = np.concatenate([np.asarray(r[0], np.uint32) for r in rows]) if rows else np.zeros(0, np.uint32)
    vals = np.concatenate([np.asarray(r[1], np.float32) for r in rows]) if rows else np.zeros(0, np.float32)
    return ptr, ids, vals


def _fma(a, x, y):
    return (a.astype(np.float64) + x.astype(np.float64) * y.astype(np.float64)).astype(np.float32)


def scan(space, rows, q, query_right=True):
    """distance(row, q) for every row (query_right) or distance(q, row).  rows: CSR triple or list of (ids, values)."""
    ptr, rid, rval = rows if isinstance(rows, tuple) else csr(rows)
    n = len(ptr) - 1
    qi, qv = np.asarray(q[0], np.uint32), np.asarray(q[1], np.float32)
    rown = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    # row elements, with the query's value where the id is shared
    loc = np.searchsorted(qi, rid)
    hit = (loc < len(qi)) & (qi[np.minimum(loc, max(len(qi) - 1, 0))] == rid) if len(qi) else np.zeros(len(rid), bool)
    ry = np.where(hit, qv[np.minimum(loc, max(len(qi) - 1, 0))] if len(qi) else 0, 0).astype(np.float32)
    # query elements missing from each row
    qrow = np.repeat(np.arange(n, dtype=np.int64), len(qi))
    qid = np.tile(qi, n)
    qval = np.tile(qv, n)
    shared = np.zeros(len(qid), bool)
    if len(rid):
        key_r = rown.astype(np.uint64) << np.uint64(32) | rid.astype(np.uint64)
        key_q = qrow.astype(np.uint64) << np.uint64(32) | qid.astype(np.uint64)
        shared = np.isin(key_q, key_r[hit])
    row = np.concatenate([rown, qrow[~shared]])
    uid = np.concatenate([rid, qid[~shared]])
    x = np.concatenate([rval, np.zeros(int((~shared).sum()), np.float32)])
    y = np.concatenate([ry, qval[~shared]])
    order = np.lexsort((uid, row))
    row, x, y = row[order], x[order], y[order]
    if not query_right:
        x, y = y, x
    ulen = np.bincount(row, minlength=n)
    start = np.concatenate([[0], np.cumsum(ulen)[:-1]])
    pos = np.arange(len(row)) - start[row]
    n4 = ulen // 4 * 4
    body = pos < n4[row]
    lane = row * 4 + (pos & 3)
    tails = [(pos == n4[row] + t) for t in range(3)]

    def lanes(term):
        acc = np.zeros(4 * n, np.float32)
        np.add.at(acc, lane[body], term[body])
        acc = acc.reshape(n, 4)
        return f32(1) * (((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3])

    def tail_fma(res, a, b):
        for t in tails:
            rr = row[t]
            res[rr] = _fma(res[rr], a[t], b[t])
        return res

    if space == "linf_sparse":
        out = np.zeros(n, np.float32)
        np.maximum.at(out, row, np.abs(x - y))
        return out
    if space == "l1_sparse":
        res = lanes(np.abs(x - y)).astype(np.float64)
        for t in tails:
            res[row[t]] += np.abs(x[t] - y[t]).astype(np.float64)
        return res.astype(np.float32)
    if space == "l2_sparse":
        d = (x - y).astype(np.float32)
        return np.sqrt(tail_fma(lanes(d * d), d, d)).astype(np.float32)
    if space == "negdotprod_sparse":
        return -tail_fma(lanes(x * y), x, y)
    if space == "querynorm_negdotprod_sparse":  # src/distcomp_scalar.cc:64-79: one sequential, contracted loop
        s = np.zeros(n, np.float32)
        n2 = np.zeros(n, np.float32)
        for p in range(int(ulen.max()) if n else 0):
            m = pos == p
            rr = row[m]
            n2[rr] = _fma(n2[rr], y[m], y[m])
            s[rr] = _fma(s[rr], x[m], y[m])
        return -(s / np.sqrt(np.maximum(n2, EPS))).astype(np.float32)
    # cosine / angular: NormScalarProductSIMD, distcomp_scalar.cc:83-168
    s = tail_fma(lanes(x * y), x, y)
    n1 = tail_fma(lanes(x * x), x, x)
    n2 = tail_fma(lanes(y * y), y, y)
    with np.errstate(divide="ignore", invalid="ignore"):
        v = (s / np.sqrt(n1) / np.sqrt(n2)).astype(np.float32)
    v = np.where((n1 < EPS) | (n2 < EPS), f32(0), np.maximum(f32(-1), np.minimum(f32(1), v))).astype(np.float32)
    if space == "angulardist_sparse":
        return np.array(_acosf(v), np.float32)
    return np.maximum(f32(0), f32(1) - v).astype(np.float32)


def distance(space, a, b):
    """IndexTimeDistance(a, b); a, b = (ids, values)."""
    return float(scan(space, [a], b)[0])


def distance_oracle(space, a, b):
    """The same through the CPU oracle's dense formula on the union arrays (no FMA in the tails)."""
    ia, ib = np.asarray(a[0], np.uint32), np.asarray(b[0], np.uint32)
    u = np.union1d(ia, ib)
    x = np.zeros(len(u), np.float32)
    y = np.zeros(len(u), np.float32)
    x[np.searchsorted(u, ia)] = a[1]
    y[np.searchsorted(u, ib)] = b[1]
    L = orc.lib()
    return float(np.float32(L.orc_space_distance(orc.SPACES[ORC_SPACE[space]], x.ctypes.data_as(C.c_void_p),
                                                 y.ctypes.data_as(C.c_void_p), len(x))))


def seq_search(space, rows, queries, k):
    """seq_search: per query the k smallest (distance(row, query), position); -> pos, dist [nq, k] (-1 / inf pad)"""
    rows = rows if isinstance(rows, tuple) else csr(rows)
    n = len(rows[0]) - 1
    pos = np.full((len(queries), k), -1, np.int32)
    dist = np.full((len(queries), k), np.inf, np.float32)
    for qi, q in enumerate(queries):
        d = scan(space, rows, q)
        order = np.lexsort((np.arange(n), d))[:k]
        pos[qi, :len(order)] = order
        dist[qi, :len(order)] = d[order]
    return pos, dist
