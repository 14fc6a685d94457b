"""-m gpu: the inverted-file filter of the sparse inner-product spaces (last_path 15) against the exact scan
(the same batch with NMSLIB_GPU_SPARSE_FAST=0, byte for byte) and against float64 (scipy.sparse product, norms in f64)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import nmslib_zig_amd as nz

pytestmark = pytest.mark.gpu

SPACES = ["negdotprod_sparse", "querynorm_negdotprod_sparse", "cosinesimil_sparse", "angulardist_sparse"]
BLOCK, N, NQ, NEAR, VOCAB = 16384, 65536 + 37, 300, 140, 1 << 20     # a last block of 37 rows; NEAR > the largest K' = 136
U = 2.0 ** -24


def zipf_rows(rng, n, mean_len, signed):
    """n rows as (row, id, value) triples sorted by (row, id): Poisson(mean_len) Zipf(1.1) draws each, duplicates merged"""
    lens = np.clip(rng.poisson(mean_len, size=n), 1, None)
    draws = np.empty(0, np.int64)
    while len(draws) < lens.sum():
        d = rng.zipf(1.1, size=int(lens.sum())) - 1
        draws = np.concatenate([draws, d[d < VOCAB]])
    key = np.unique(np.repeat(np.arange(n, dtype=np.int64), lens) * VOCAB + draws[:lens.sum()])
    vals = rng.uniform(0.1, 1.0, size=len(key)) * (rng.choice([-1.0, 1.0], size=len(key)) if signed else 1.0)
    return key // VOCAB, key % VOCAB, vals


@functools.lru_cache(maxsize=None)
def data(signed):
    """Zipf rows and queries; term 0 in every row (one segment covers a whole block), tail terms in one row of one block.
    Query 1 has a single element, query 2 has 4096.  Per query NEAR planted rows a (q + t |q| e), e a term of their own:
    their products fall by 0.004 |q|^2 and their cosines by 0.003 per rank, far above what a random row reaches.
    -> X (csr, f32 values), queries [(ids, values)]"""
    rng = np.random.default_rng(11 + signed)
    qr, qi, qv = zipf_rows(rng, NQ, 32, signed)
    queries = [(qi[qr == j], qv[qr == j]) for j in range(NQ)]
    queries[1] = (np.array([777777]), np.array([0.7]))                                  # (a tail term: the planted rows alone hold it)
    queries[2] = (np.sort(rng.choice(VOCAB, 4096, replace=False)), rng.uniform(0.1, 1.0, 4096) * 0.08)
    xr, xi, xv = zipf_rows(rng, N, 64, signed)
    keep = xi != 0
    xr, xi, xv = (np.concatenate([v[keep], h]) for v, h in ((xr, np.arange(N)), (xi, np.zeros(N, np.int64)),
                                                            (xv, rng.uniform(0.1, 1.0, N))))
    where = BLOCK + rng.permutation(N - BLOCK)[:NQ * NEAR].reshape(NQ, NEAR)            # (block 0 keeps term 0 in every row)
    free = ~np.isin(xr, where)
    rows, ids, vals = [xr[free]], [xi[free]], [xv[free]]
    cos = 0.98 - 0.003 * np.arange(NEAR)
    for j, (ti, tv) in enumerate(queries):
        a, t = 1.56 - 0.004 * np.arange(NEAR), np.sqrt(1.0 / cos ** 2 - 1.0) * np.linalg.norm(tv)
        rows.append(np.repeat(where[j], len(ti) + 1))
        ids.append(np.concatenate([np.tile(ti, (NEAR, 1)), VOCAB + j * NEAR + np.arange(NEAR)[:, None]], 1).ravel())
        vals.append((a[:, None] * np.concatenate([np.tile(tv, (NEAR, 1)), t[:, None]], 1)).ravel())
    X = sp.csr_matrix((np.concatenate(vals).astype(np.float32), (np.concatenate(rows), np.concatenate(ids))),
                      shape=(N, VOCAB + NQ * NEAR))
    X.sort_indices()
    return X, [(i.astype(np.uint32), v.astype(np.float32)) for i, v in queries]


def as_rows(X):
    return X.indptr.astype(np.int64), X.indices.astype(np.uint32), X.data


@functools.lru_cache(maxsize=None)
def reference(signed):
    """float64: the products Q X^T, the norms, and per pair the relative bound of the scan's f32 inner product"""
    X, queries = data(signed)
    Q = sp.csr_matrix((np.concatenate([v for _, v in queries]).astype(np.float64), np.concatenate([i for i, _ in queries]),
                       np.cumsum([0] + [len(i) for i, _ in queries])), shape=(NQ, X.shape[1]))
    X = X.astype(np.float64)
    S = np.asarray((Q @ X.T).todense())
    xn, qn = np.sqrt(np.asarray(X.multiply(X).sum(1)).ravel()), np.sqrt(np.asarray(Q.multiply(Q).sum(1)).ravel())
    m = np.diff(Q.indptr)
    return S, xn, qn, m, m + np.diff(X.indptr).max()                     # (union positions at most)


@functools.lru_cache(maxsize=None)
def expected(space, signed, k):
    """-> positions [NQ, k], distances, their bounds (sparse_filter.hpp: E_ref, E_cos), after the fixture's own gaps: rank k
    above every block's K'-th score by ten times the proof's bound, ranks up to k twice the pair bound apart"""
    S, xn, qn, m, L = reference(signed)
    rel = 1.001 * (L + 8.0) * U                                          # of |q| |b|, per query
    if space == "negdotprod_sparse":
        score, pair, proof = S, (rel * qn)[:, None] * xn[None, :], 2 * rel * qn * xn.max()
    elif space == "querynorm_negdotprod_sparse":
        score = S / qn[:, None]
        pair, proof = rel[:, None] * xn[None, :] + np.abs(score) * (1.001 * (m + 8.0) * U)[:, None], 2 * rel * xn.max()
    else:
        score = S / (qn[:, None] * xn[None, :])
        pair = np.broadcast_to((1.001 * (2 * (L + 8.0) + 8) * U + 4 * U)[:, None], S.shape)
        proof = 2 * pair[:, 0]
    order = np.argpartition(-score, k + 1, 1)[:, :k + 1]
    order = np.take_along_axis(order, np.lexsort((order, -np.take_along_axis(score, order, 1)), axis=1), 1)
    top, tb = np.take_along_axis(score, order, 1), np.take_along_axis(pair, order, 1)
    kth = np.max([np.partition(score[:, b:b + BLOCK], -(k + 8), 1)[:, -(k + 8)] for b in range(0, N, BLOCK) if N - b >= k + 8], 0)
    assert (top[:, k - 1] - kth >= 10 * proof).all(), "the fixture's margin over the blocks' thresholds"
    assert (-np.diff(top, axis=1) > 2 * np.maximum(tb[:, 1:], tb[:, :-1])).all(), "the fixture's gaps"
    top, tb = top[:, :k], tb[:, :k]
    if space.startswith("cosine"):
        return order[:, :k], 1 - top, tb
    if space.startswith("angular"):
        lo, hi = np.arccos(np.clip(top + tb, -1, 1)), np.arccos(np.clip(top - tb, -1, 1))
        return order[:, :k], np.arccos(top), np.maximum(hi - np.arccos(top), np.arccos(top) - lo) + 16 * U * np.pi
    return order[:, :k], -top, tb


def index(space, X):
    idx = nz.Index(space, "seq_search", data_type="SparseVector")
    idx.addSparseBatch(as_rows(X))
    idx.buildIndex()
    return idx


def both(idx, queries, k, monkeypatch):
    """the batch with the path on and off -> the path-on answer and statistics; bytes equal"""
    monkeypatch.setenv("NMSLIB_GPU_SPARSE_FAST", "1")
    on = idx.knnQueryBatch(queries, k)
    st = idx.stats()
    monkeypatch.setenv("NMSLIB_GPU_SPARSE_FAST", "0")
    off = idx.knnQueryBatch(queries, k)
    assert idx.stats()["last_path"] == 0
    for x, y in zip(on, off):
        assert x.tobytes() == y.tobytes()
    return on, st


@pytest.fixture(scope="module")
def indexes():
    made = {}
    yield lambda space, signed: made.setdefault((space, signed), index(space, data(signed)[0]))
    for idx in made.values():
        idx.close()


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("space", SPACES)
def test_fast_path_equals_exact_scan_and_float64(indexes, space, k, monkeypatch):
    (ids, ds, cnt), st = both(indexes(space, False), data(False)[1], k, monkeypatch)
    assert st["last_path"] == 15 and st["fast_tiles"] == NQ and st["fast_tiles_fallback"] == 0, st
    pos, dd, bb = expected(space, False, k)
    assert (cnt == k).all()
    np.testing.assert_array_equal(ids, pos)
    assert (np.abs(ds.astype(np.float64) - dd) <= bb).all()


@pytest.mark.parametrize("space,k", [("negdotprod_sparse", 10), ("cosinesimil_sparse", 128)])
def test_signed_values_equal_exact_scan(indexes, space, k, monkeypatch):
    """signed values: touched rows score on both sides of the untouched rows' 0"""
    _, st = both(indexes(space, True), data(True)[1], k, monkeypatch)
    assert st["last_path"] == 15 and st["fast_tiles"] == NQ and st["fast_tiles_fallback"] < NQ, st


def test_mixed_batch_falls_back_per_query(monkeypatch):
    """Queries whose proof must fail -- K' + 1 exact copies of a query's best row inside one block, a query that shares no
    term with the index, a NaN query -- are redone by the exact scan while the others stay on the filter's answer.  Two
    copies of a best row on either side of a block boundary with k cutting the triple are all listed: the re-rank orders
    them by position as the scan does."""
    X, queries = data(False)
    pos, _, _ = expected("cosinesimil_sparse", False, 2)
    src = np.arange(N)
    src[BLOCK + 100:BLOCK + 100 + 2 + 8 + 1] = pos[0, 0]
    src[BLOCK - 1:BLOCK + 1] = pos[200, 0]
    X = X[src]
    queries = list(queries)
    queries[40] = (np.arange(5, dtype=np.uint32) + X.shape[1] + 9, np.ones(5, np.float32))
    queries[100] = (queries[100][0], np.where(np.arange(len(queries[100][0])) == 1, np.nan, queries[100][1]).astype(np.float32))
    idx = index("cosinesimil_sparse", X)
    (ids, ds, cnt), st = both(idx, queries, 2, monkeypatch)
    assert st["last_path"] == 15 and st["fast_tiles"] == NQ and 3 <= st["fast_tiles_fallback"] < NQ // 2, st
    assert list(ids[200]) == sorted([BLOCK - 1, BLOCK, int(pos[200, 0])])[:2]
    idx.close()


def test_gates(indexes, monkeypatch):
    X, queries = data(False)
    monkeypatch.setenv("NMSLIB_GPU_SPARSE_FAST", "0")
    idx = index("negdotprod_sparse", X)
    csr = idx.stats()["hbm_bytes"]                                           # turned off at finalize: no copy
    idx.knnQueryBatch(queries[:4], 10)
    assert idx.stats()["last_path"] == 0 and idx.stats()["hbm_bytes"] == csr
    monkeypatch.delenv("NMSLIB_GPU_SPARSE_FAST")                             # on by default; the copy is made now
    idx.knnQueryBatch(queries[:4], 129)
    assert idx.stats()["last_path"] == 0 and idx.stats()["hbm_bytes"] == csr
    idx.knnQueryBatch(queries[:4], 10)
    assert idx.stats()["last_path"] == 15 and idx.stats()["hbm_bytes"] >= csr + 6 * X.nnz
    long = (np.arange(4097, dtype=np.uint32), np.ones(4097, np.float32))
    idx.knnQueryBatch(queries[:4] + [long], 10)
    assert idx.stats()["last_path"] == 0
    idx.close()
    assert indexes("negdotprod_sparse", False).stats()["hbm_bytes"] >= csr + 6 * X.nnz   # at finalize
    idx = index("negdotprod_sparse", X[:65535])
    idx.knnQueryBatch(queries[:4], 10)
    assert idx.stats()["last_path"] == 0
    idx.close()
    # a duplicated id in a row never reaches an index: the interface refuses the row when it is added (the copy's own
    # check of ascending ids, which would leave such an index on the scan, stands behind that)
    p, i, v = as_rows(X[:8])
    i = i.copy()
    i[p[5] + 1] = i[p[5]]
    idx = nz.Index("negdotprod_sparse", "seq_search", data_type="SparseVector")
    with pytest.raises(nz.NmslibError, match="InvalidSparseElement"):
        idx.addSparseBatch((p, i, v))
    idx.close()
