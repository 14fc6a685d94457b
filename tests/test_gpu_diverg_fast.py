"""-m gpu: the bf16 MFMA filter scan of the Bregman "fast" divergences (last_path 14) against the exact scan
(the same batch with NMSLIB_GPU_DIVERG_FAST=0, byte for byte) and against float64 (tests/diverg_ref.py's formulas and bound,
evaluated as matrix products)."""
import functools

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import diverg_ref

pytestmark = pytest.mark.gpu

SPACES = ["kldivfast", "kldivfastrq", "kldivgenfast", "kldivgenfastrq", "itakurasaitofast"]
N, NQ, NEAR = 65536 + 37, 300, 132      # a partial row block, a partial query tile; NEAR > the largest k + 1
KEEP, SPLIT_ROWS = 32, 1056             # dvf::kKeep; rows per split at N (64 splits of 33 blocks)


def peaky(rng, n, D, heavy):
    """positive histograms with elements >= 1e-3 at D <= 256; heavy = 0 / 1: the half of the columns with twice the weight
    (histograms of different halves are far from each other at every D)"""
    x = (rng.uniform(0, 1, size=(n, D)) ** 4 + 0.25) * np.where((np.arange(D) < (D + 1) // 2) == bool(heavy), 2.0, 1.0)
    return x / x.sum(1, keepdims=True)


@functools.lru_cache(maxsize=None)
def data(D):
    """Rows far from every query, and per query NEAR rows on the segment from the query towards another histogram at
    steps that grow like sqrt(t): along it every one of these (convex) divergences grows by about the same gap per row."""
    rng = np.random.default_rng(100 + D)
    Q = peaky(rng, NQ, D, 1)
    X = peaky(rng, N, D, 0)
    if D == 8:   # random histograms crowd in 8 dimensions: distinct patterns of 1, 2, 4, 8 per column keep apart
        # (column 0 stays 1, so that no pattern is a multiple of another; the queries' patterns are their own, the other
        #  rows share theirs four by four, 1 % apart)
        pat = 4 * rng.permutation(4 ** 7)[np.concatenate([np.arange(NQ), NQ + np.arange(N) % (4 ** 7 - NQ)])]
        lat = 2.0 ** ((pat[:, None] >> (2 * np.arange(8))) & 3) * rng.uniform(0.99, 1.01, size=(N + NQ, 8))
        lat /= lat.sum(1, keepdims=True)
        Q, X = lat[:NQ], lat[NQ:]
    where = rng.permutation(N)[:NQ * NEAR].reshape(NQ, NEAR)
    P = peaky(rng, NQ, D, 1)
    # (in 8 dimensions the segment must end before the rows of the nearest other pattern: its steps are sized by the
    #  segment's own curvature, for gaps of 2e-5 in KL)
    s0 = np.sqrt(4e-5 / ((P - Q) ** 2 / Q).sum(1)) if D == 8 else np.full(NQ, 0.045)
    s = s0[:, None, None] * np.sqrt(np.arange(1, NEAR + 1))[None, :, None]
    X[where] = (1 - s) * Q[:, None, :] + s * P[:, None, :]
    X, Q = X.astype(np.float32), Q.astype(np.float32)
    assert X.min() >= 1e-3 and Q.min() >= 1e-3
    return X, Q


@functools.lru_cache(maxsize=None)
def reference(space, D):
    """float64 d(row, query) and the bound's S for all pairs -> positions, distances and bounds of the first 130, ascending
    (distance, position); asserts that the f64 gaps among them exceed twice the bound"""
    X, Q = (v.astype(np.float64) for v in data(D))
    lX, lQ = np.log(X), np.log(Q)
    a, b = (lX, Q) if space.endswith("rq") else (X, lQ)          # d = sign a.b + R_row + C_q
    if space.startswith("kldiv"):
        gen = space.startswith("kldivgen")
        R = (0 if space.endswith("rq") else (X * lX).sum(1)) + (X.sum(1) * (1 if space.endswith("rq") else -1) if gen else 0)
        C = ((Q * lQ).sum(1) if space.endswith("rq") else 0) + (Q.sum(1) * (-1 if space.endswith("rq") else 1) if gen else 0)
        d = -(Q @ lX.T if space.endswith("rq") else lQ @ X.T) + R + np.reshape(C, (-1, 1))
        own = (np.abs(X * lX).sum(1), np.abs(Q * lQ).sum(1))
        S = np.abs(b) @ np.abs(a).T + (own[1][:, None] if space.endswith("rq") else own[0][None, :])
        if gen:
            S = S + np.abs(X).sum(1)[None, :] + np.abs(Q).sum(1)[:, None]
    else:
        d = (1 / Q) @ X.T - lX.sum(1)[None, :] + lQ.sum(1)[:, None] - D
        S = (1 / Q) @ X.T + np.abs(lX).sum(1)[None, :] + np.abs(lQ).sum(1)[:, None] + D
    order = np.argsort(d, axis=1, kind="stable")[:, :130]
    dd = np.take_along_axis(d, order, 1)
    bb = diverg_ref.bound(np.take_along_axis(S, order, 1), D)
    return order, dd, bb


def index(space, X):
    idx = nz.Index(space, "seq_search")
    idx.addDenseBatch(X)
    idx.buildIndex()
    return idx


def both(idx, Q, k, monkeypatch):
    """the batch with the path on and off -> the path-on answer and statistics; bytes equal"""
    monkeypatch.setenv("NMSLIB_GPU_DIVERG_FAST", "1")
    on = idx.knnQueryBatch(Q, k)
    st = idx.stats()
    monkeypatch.setenv("NMSLIB_GPU_DIVERG_FAST", "0")
    off = idx.knnQueryBatch(Q, k)
    assert idx.stats()["last_path"] == 0
    for x, y in zip(on, off):
        assert x.tobytes() == y.tobytes()
    return on, st


@pytest.fixture(scope="module")
def indexes():
    made = {}
    yield lambda space, D: made.setdefault((space, D), index(space, data(D)[0]))
    for idx in made.values():
        idx.close()


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("D", [8, 100, 256])
@pytest.mark.parametrize("space", SPACES)
def test_fast_path_equals_exact_scan_and_float64(indexes, space, D, k, monkeypatch):
    X, Q = data(D)
    (ids, ds, cnt), st = both(indexes(space, D), Q, k, monkeypatch)
    assert st["last_path"] == 14 and st["fast_tiles"] == (NQ + 15) // 16 and st["fast_tiles_fallback"] == 0, st
    pos, dd, bb = reference(space, D)
    assert (np.diff(dd, axis=1) > 2 * np.maximum(bb[:, 1:], bb[:, :-1])).all(), "the fixture's gaps"
    assert (cnt == k).all()
    np.testing.assert_array_equal(ids, pos[:, :k])
    assert (np.abs(ds.astype(np.float64) - dd[:, :k]) <= bb[:, :k]).all()


def test_mixed_batch_falls_back_per_group(monkeypatch):
    """Groups whose proof must fail -- KEEP + 1 exact copies of a query's nearest row inside one split, a query with a zero
    element, a NaN query, identical rows on either side of a split boundary with k cutting between them -- are redone by
    the exact scan while the other groups stay on the filter's answer."""
    X, Q = (v.copy() for v in data(100))
    pos, _, _ = reference("kldivfast", 100)
    X[5 * SPLIT_ROWS + 10:5 * SPLIT_ROWS + 10 + KEEP + 1] = X[pos[0, 0]]     # query 0 (group 0)
    Q[40, 3] = 0.0                                                           # group 2
    Q[100, 7] = np.nan                                                       # group 6
    X[SPLIT_ROWS - 1] = X[SPLIT_ROWS] = X[pos[200, 0]]                       # query 200 (group 12): k = 2 cuts the triple
    idx = index("kldivfast", X)
    (ids, ds, cnt), st = both(idx, Q, 2, monkeypatch)
    assert st["last_path"] == 14 and 0 < st["fast_tiles_fallback"] < st["fast_tiles"], st
    assert sorted(ids[200]) == sorted([SPLIT_ROWS - 1, SPLIT_ROWS, int(pos[200, 0])])[:2]
    idx.close()


def test_gates(monkeypatch):
    X, Q = data(8)
    monkeypatch.setenv("NMSLIB_GPU_DIVERG_FAST", "0")
    idx = index("kldivfast", X)
    planes = idx.stats()["hbm_bytes"]                                        # turned off at finalize: no copy
    idx.knnQueryBatch(Q[:256], 10)
    assert idx.stats()["last_path"] == 0 and idx.stats()["hbm_bytes"] == planes
    monkeypatch.delenv("NMSLIB_GPU_DIVERG_FAST")                             # on by default; the copy is made now
    idx.knnQueryBatch(Q[:255], 10)
    assert idx.stats()["last_path"] == 0 and idx.stats()["hbm_bytes"] == planes
    idx.knnQueryBatch(Q[:256], 10)
    assert idx.stats()["last_path"] == 14
    assert idx.stats()["hbm_bytes"] >= planes + (N // 32) * 16 * 2 * 2 * 32   # the bf16 fragments
    idx.close()
    idx = index("kldivfast", X)
    assert idx.stats()["hbm_bytes"] >= planes + (N // 32) * 16 * 2 * 2 * 32   # at finalize
    idx.close()
    idx = index("kldivfast", X[:65535])
    idx.knnQueryBatch(Q[:256], 10)
    assert idx.stats()["last_path"] == 0
    idx.close()
