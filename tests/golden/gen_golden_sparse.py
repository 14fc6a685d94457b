#!/usr/bin/env python3
"""Sparse-vector fixture from the REAL reference (oracle/_ref/libnmslib_ref.so through its C ABI, data type 1, seq_search).

    make -C oracle ref && python3 tests/golden/gen_golden_sparse.py

For every space configuration of SPACES:
  * "main" set (Zipf-like ids, one-element rows, a row and a query of 20 000 elements, a query disjoint from every row,
    a query with an id beyond every row id): k = 10 and k = 100 (ids, distances, counts), range queries at two radii
    with a small and a large capacity, get_distance over fixed pairs;
  * "ties" set (integer values over a small vocabulary: exact distances, many equal ones): k = 10;
  * "tiny" set (7 rows): k = 10 > n.
Only the reference's outputs are stored; the inputs are regenerated from their seeds and pinned by SHA-256.

Tie order.  The reference's result queue holds pair<distance, Object*> (knnqueue.h:73-74), so rows at equal distance
come out in the order of their ADDRESSES; for rows of different lengths that is the allocator's order, which changes
from one process to the next.  The k-NN cases therefore ask the reference for every row (k = n) and store its
distances in (distance, position) order -- NMSLIB's documented order and this library's -- cut to k.  Distances and
range results (insertion order) are the reference's as they come.
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import orc  # noqa: E402

# (tag, space name, space params).  querynorm_negdotprod_sparse is not here: the reference registers only its
# "_fast" variant (include/factory/init_spaces.h:87-103), so its C ABI refuses the name.
SPACES = [
    ("cosinesimil_sparse", "cosinesimil_sparse", {}),
    ("angulardist_sparse", "angulardist_sparse", {}),
    ("negdotprod_sparse", "negdotprod_sparse", {}),
    ("l1_sparse", "l1_sparse", {}),
    ("l2_sparse", "l2_sparse", {}),
    ("linf_sparse", "linf_sparse", {}),
    ("lp_sparse_p1", "lp_sparse", {"p": 1.0}),
    ("lp_sparse_p2", "lp_sparse", {"p": 2.0}),
    ("lp_sparse_pm1", "lp_sparse", {"p": -1.0}),
]
RANGE_CAPS = (4, 1000)
LONG = 20000


def sha(rows):
    h = hashlib.sha256()
    for ids, vals in rows:
        h.update(np.ascontiguousarray(ids, np.uint32).tobytes())
        h.update(np.ascontiguousarray(vals, np.float32).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def zipf_row(rng, m, vocab, a=1.1):
    """m distinct ids drawn Zipf-like over [0, vocab), sorted; values in (-1, 1) as float32."""
    ids = set()
    while len(ids) < m:
        for v in rng.zipf(a, size=2 * (m - len(ids)) + 4):
            if v - 1 < vocab:
                ids.add(int(v - 1))
                if len(ids) == m:
                    break
    ids = np.array(sorted(ids), np.uint32)
    vals = rng.uniform(-1, 1, size=m).astype(np.float32)
    return ids, vals


def uniform_row(rng, m, lo, hi):
    ids = np.sort(rng.choice(np.arange(lo, hi, dtype=np.int64), size=m, replace=False)).astype(np.uint32)
    return ids, rng.uniform(-1, 1, size=m).astype(np.float32)


def inputs_main():
    rng = np.random.default_rng(20261015)
    vocab = 50000
    rows = [zipf_row(rng, int(rng.integers(1, 61)), vocab) for _ in range(600)]
    for i in range(0, 600, 97):                         # one-element rows
        rows[i] = zipf_row(rng, 1, vocab)
    rows[333] = uniform_row(rng, LONG, 0, vocab)        # one long row
    qs = [zipf_row(rng, int(rng.integers(1, 41)), vocab) for _ in range(20)]
    qs.append(uniform_row(rng, 12, 1 << 30, (1 << 30) + 1000))       # disjoint from every row
    ids, vals = zipf_row(rng, 9, vocab)                               # an id beyond every row id
    qs.append((np.append(ids, np.uint32(4000000000)), np.append(vals, np.float32(0.5))))
    qs.append(uniform_row(rng, LONG, 0, vocab))                       # one long query
    qs.append(zipf_row(rng, 1, vocab))                                # one element
    pairs = np.array([[0, 1], [5, 5], [333, 7], [7, 333], [97, 194], [12, 400], [599, 0], [333, 333]]
                     + rng.integers(0, 600, size=(12, 2)).tolist(), np.int64)
    return rows, qs, pairs


def inputs_ties():
    rng = np.random.default_rng(77)

    def row():
        m = int(rng.integers(1, 9))
        ids = np.sort(rng.choice(40, size=m, replace=False)).astype(np.uint32)
        return ids, rng.integers(1, 4, size=m).astype(np.float32)

    return [row() for _ in range(300)], [row() for _ in range(12)]


def inputs_tiny():
    rng = np.random.default_rng(5)
    return [zipf_row(rng, int(rng.integers(1, 6)), 100) for _ in range(7)], \
           [zipf_row(rng, int(rng.integers(1, 6)), 100) for _ in range(3)]


def pack(rows):
    """-> back-to-back elements (uint32 id, float32 value) and counts"""
    counts = np.array([len(r[0]) for r in rows], np.uint64)
    el = np.zeros(int(counts.sum()), [("id", "<u4"), ("value", "<f4")])
    at = 0
    for ids, vals in rows:
        el["id"][at:at + len(ids)] = ids
        el["value"][at:at + len(ids)] = vals
        at += len(ids)
    return el, counts


# ---- the reference's C ABI (include/nmslib_c.h) over ctypes ---------------------------------------------------------
class _Alloc(C.Structure):
    _fields_ = [("alloc", C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)),
                ("free", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)), ("ctx", C.c_void_p)]


class _Result(C.Structure):
    _fields_ = [("ids", C.POINTER(C.c_int32)), ("distances", C.POINTER(C.c_float)),
                ("size", C.c_size_t), ("capacity", C.c_size_t)]


_libc = C.CDLL(None)
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]
_libc.free.argtypes = [C.c_void_p]
_ALLOC = _Alloc(_Alloc._fields_[0][1](lambda n, ctx: _libc.malloc(max(n, 1))),
                _Alloc._fields_[1][1](lambda p, ctx: _libc.free(p)), None)


def ref_lib():
    L = C.CDLL(orc.REF_LIB)
    vp, sz = C.c_void_p, C.c_size_t
    L.nmslib_index_create.argtypes = [C.c_char_p, vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(_Alloc), C.POINTER(vp)]
    L.nmslib_create_params.restype = vp
    L.nmslib_create_params.argtypes = [C.POINTER(_Alloc)]
    L.nmslib_add_param.argtypes = [vp, C.c_char_p, C.c_int, vp]
    L.nmslib_free_params.argtypes = [vp]
    L.nmslib_add_data_point_batch.argtypes = [vp, vp, sz, sz, vp, vp]
    L.nmslib_create_index.argtypes = [vp, vp, C.c_int]
    L.nmslib_knn_query_batch.argtypes = [vp, vp, sz, sz, sz, C.POINTER(_Result), vp, sz]
    L.nmslib_range_query_fill.argtypes = [vp, vp, sz, C.c_double, C.POINTER(_Result), sz]
    L.nmslib_get_distance.argtypes = [vp, sz, sz, C.POINTER(C.c_float)]
    L.nmslib_index_destroy.argtypes = [vp]
    return L


class RefIndex:
    """seq_search over sparse rows in the compiled reference."""

    def __init__(self, L, space, space_params, rows):
        self.L = L
        L.nmslib_init()
        sp = None
        if space_params:
            sp = C.c_void_p(L.nmslib_create_params(C.byref(_ALLOC)))
            for k, v in space_params.items():
                d = C.c_double(v)
                assert L.nmslib_add_param(sp, k.encode(), 1, C.byref(d)) == 0
        self.h = C.c_void_p()
        rc = L.nmslib_index_create(space.encode(), sp, b"seq_search", 1, 0, C.byref(_ALLOC), C.byref(self.h))
        if sp:
            L.nmslib_free_params(sp)
        assert rc == 0, f"reference refused {space}: {rc}"
        el, counts = pack(rows)
        assert L.nmslib_add_data_point_batch(self.h, el.ctypes.data, len(rows), int(counts.max()), None,
                                             counts.ctypes.data) == 0
        assert L.nmslib_create_index(self.h, None, 0) == 0

    def knn(self, queries, k):
        el, counts = pack(queries)
        nq, width = len(queries), int(counts.max())
        slots = np.zeros((nq, width), el.dtype)               # the slot layout, nmslib_c.cpp:1003-1031
        at = 0
        for i, c in enumerate(counts):
            slots[i, :c] = el[at:at + c]
            at += int(c)
        ids = np.full((nq, k), -1, np.int32)
        ds = np.full((nq, k), np.inf, np.float32)
        res = (_Result * nq)()
        for i in range(nq):
            res[i] = _Result(ids[i].ctypes.data_as(C.POINTER(C.c_int32)), ds[i].ctypes.data_as(C.POINTER(C.c_float)),
                             0, k)
        assert self.L.nmslib_knn_query_batch(self.h, slots.ctypes.data, nq, 2 * width, k, res, counts.ctypes.data,
                                             1) == 0
        return ids, ds, np.array([res[i].size for i in range(nq)], np.int32)

    def knn_canonical(self, queries, k, n):
        """the reference's distances to all n rows, in (distance, position) order, cut to k"""
        ids, ds, cnt = self.knn(queries, n)
        assert (cnt == n).all()
        out_i = np.full((len(queries), k), -1, np.int32)
        out_d = np.full((len(queries), k), np.inf, np.float32)
        for q in range(len(queries)):
            o = np.lexsort((ids[q], ds[q]))[:k]
            out_i[q, :len(o)], out_d[q, :len(o)] = ids[q][o], ds[q][o]
        return out_i, out_d, np.full(len(queries), min(k, n), np.int32)

    def range(self, query, radius, capacity):
        el, _ = pack([query])
        ids = np.full(capacity, -1, np.int32)
        ds = np.full(capacity, np.inf, np.float32)
        r = _Result(ids.ctypes.data_as(C.POINTER(C.c_int32)), ds.ctypes.data_as(C.POINTER(C.c_float)), 0, capacity)
        assert self.L.nmslib_range_query_fill(self.h, el.ctypes.data, 2 * len(el), float(radius), C.byref(r),
                                              len(el)) == 0
        return ids[:r.size], ds[:r.size]

    def distance(self, a, b):
        v = C.c_float()
        assert self.L.nmslib_get_distance(self.h, int(a), int(b), C.byref(v)) == 0
        return v.value

    def close(self):
        self.L.nmslib_index_destroy(self.h)


def range_radii(d10):
    """two radii per query from its k=10 distances: the 3rd and the 10th (rows at the radius are in)"""
    return np.stack([d10[:, 2], d10[:, 9]], axis=1).astype(np.float64)


def run_reference():
    L = ref_lib()
    main_rows, main_q, pairs = inputs_main()
    tie_rows, tie_q = inputs_ties()
    tiny_rows, tiny_q = inputs_tiny()
    out = {"main_rows_sha": sha(main_rows), "main_queries_sha": sha(main_q), "main_pairs": pairs,
           "ties_rows_sha": sha(tie_rows), "ties_queries_sha": sha(tie_q),
           "tiny_rows_sha": sha(tiny_rows), "tiny_queries_sha": sha(tiny_q)}
    for tag, space, sp in SPACES:
        ix = RefIndex(L, space, sp, main_rows)
        for k in (10, 100):
            out[f"{tag}_k{k}_ids"], out[f"{tag}_k{k}_dists"], out[f"{tag}_k{k}_cnt"] = \
                ix.knn_canonical(main_q, k, len(main_rows))
        radii = range_radii(out[f"{tag}_k10_dists"])
        out[f"{tag}_radii"] = radii
        for cap in RANGE_CAPS:
            rid, rd, rn = [], [], []
            for qi, q in enumerate(main_q):
                for r in radii[qi]:
                    a, b = ix.range(q, r, cap)
                    rid.append(a)
                    rd.append(b)
                    rn.append(len(a))
            out[f"{tag}_range{cap}_n"] = np.array(rn, np.int32)
            out[f"{tag}_range{cap}_ids"] = np.concatenate(rid).astype(np.int32)
            out[f"{tag}_range{cap}_dists"] = np.concatenate(rd).astype(np.float32)
        out[f"{tag}_pair_dists"] = np.array([ix.distance(a, b) for a, b in pairs], np.float32)
        ix.close()
        ix = RefIndex(L, space, sp, tie_rows)
        out[f"{tag}_ties_ids"], out[f"{tag}_ties_dists"], out[f"{tag}_ties_cnt"] = \
            ix.knn_canonical(tie_q, 10, len(tie_rows))
        ix.close()
        ix = RefIndex(L, space, sp, tiny_rows)
        out[f"{tag}_tiny_ids"], out[f"{tag}_tiny_dists"], out[f"{tag}_tiny_cnt"] = ix.knn_canonical(tiny_q, 10, len(tiny_rows))  # k > n
        ix.close()
    return out


def main():
    assert os.path.exists(orc.REF_LIB), "build oracle/_ref first: make -C oracle ref"
    out = run_reference()
    path = os.path.join(HERE, "golden_sparse.npz")
    # np.savez_compressed stamps zip times: write the members with a fixed date so a rerun gives the same bytes
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.save(buf, out[key], allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(2020, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(len(out), "arrays ->", path)


if __name__ == "__main__":
    main()
