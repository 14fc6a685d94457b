"""-m gpu: the hardware-log2 filter scan of the four Jensen-Shannon spaces (last_path 16) against the exact
scan (the same batch with NMSLIB_GPU_DIVERG_FAST=0, byte for byte) and against float64 (tests/diverg_ref.py)."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import diverg_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPACES = ["jsdivslow", "jsdivfast", "jsmetrslow", "jsmetrfast"]
N, NQ, NEAR = 65536 + 37, 300, 132      # a partial row block, a partial query tile; NEAR > the largest k + 1
KEEP, SPLIT_ROWS = 32, 1088             # dvf::kKeep; rows of a wave's range at N (17 blocks of 64)
REF_Q = [0, 15, 16, 31, 32, 143, 144, 159, 160, 271, 272, 287, 288, 297, 298, 299]   # first, last, tile edges


def peaky(rng, n, D, heavy):
    """positive histograms; heavy = 0 / 1: the half of the columns with twice the weight"""
    x = (rng.uniform(0, 1, size=(n, D)) ** 4 + 0.25) * np.where((np.arange(D) < (D + 1) // 2) == bool(heavy), 2.0, 1.0)
    return x / x.sum(1, keepdims=True)


@functools.lru_cache(maxsize=None)
def data(D):
    """Rows far from every query, and per query NEAR rows on the segment from the query towards another histogram P.  To
    second order JS(q, q + s (p - q)) = s^2 chi2 / 8, chi2 = sum (p - q)^2 / q, so steps s_t = sqrt(a t) give equal gaps.
    The step is sized per D and query from the float64 reference's own bound: the first dozen rows keep gaps of 4 bounds
    ((D + 8) 2^-24 S with S <= 2 ln 2 + 2 ln D on a pair of histograms); the later rows follow at a twentieth of that,
    so that all of them stay inside the far rows (JS about 0.05)."""
    rng = np.random.default_rng(300 + D)
    Q, X, P = peaky(rng, NQ, D, 1), peaky(rng, N, D, 0), peaky(rng, NQ, D, 1)
    where = rng.permutation(N)[:NQ * NEAR].reshape(NQ, NEAR)
    gap = 4 * diverg_ref.bound(2 * np.log(2) + 2 * np.log(D), D)
    a = gap / (((P - Q) ** 2 / Q).sum(1) / 8)
    t = np.arange(1, NEAR + 1)
    s = np.sqrt(a[:, None] * np.where(t <= 12, t, 12 + (t - 12) / 20.0)[None, :])[:, :, None]
    assert s.max() < 1
    X[where] = (1 - s) * Q[:, None, :] + s * P[:, None, :]
    return X.astype(np.float32), Q.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(D):
    """float64 JS (jsmetr*: its square) of the REF_Q queries -> positions, distances and bounds of the first 10"""
    X, Q = data(D)
    return diverg_ref.seq_search("jsdivfast", X.astype(np.float64), Q[REF_Q].astype(np.float64), 10)


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
@pytest.mark.parametrize("D", [5, 100, 257])
@pytest.mark.parametrize("space", SPACES)
def test_filter_path_equals_exact_scan(indexes, space, D, k, monkeypatch):
    _, st = both(indexes(space, D), data(D)[1], k, monkeypatch)
    assert st["last_path"] == 16 and st["fast_tiles"] == (NQ + 15) // 16, st
    assert k > 10 or st["fast_tiles_fallback"] == 0, st


@pytest.mark.parametrize("D", [5, 100, 257])
@pytest.mark.parametrize("space", SPACES)
def test_filter_path_against_float64(indexes, space, D, monkeypatch):
    pos, dd, bb = reference(D)
    mask = diverg_ref.near_tie_mask(dd, bb)
    assert mask.mean() <= 0.10, "the fixture's gaps"
    monkeypatch.setenv("NMSLIB_GPU_DIVERG_FAST", "1")
    ids, ds, cnt = indexes(space, D).knnQueryBatch(data(D)[1], 10)
    assert indexes(space, D).stats()["last_path"] == 16 and (cnt == 10).all()
    assert diverg_ref.within(space, ds[REF_Q], dd, bb).all()
    assert (ids[REF_Q] == pos)[~mask].all()


def test_mixed_batch_falls_back_per_group(monkeypatch):
    """Groups whose proof must fail -- KEEP + 1 exact copies of a query's nearest row inside one wave's range, a NaN query, a
    query with a negative element -- are redone by the exact scan while the other groups stay on the filter's answer; a
    query and rows with zero elements keep their proof."""
    X, Q = (v.copy() for v in data(100))
    X[::7, 1::4] = 0.0
    Q[40, ::3] = 0.0                                                         # group 2: stays on the filter
    near0 = int(diverg_ref.seq_search("jsdivfast", X.astype(np.float64), Q[:1].astype(np.float64), 1)[0][0, 0])
    X[5 * SPLIT_ROWS + 10:5 * SPLIT_ROWS + 10 + KEEP + 1] = X[near0]         # query 0 (group 0)
    Q[100, 7] = np.nan                                                       # group 6
    Q[200, 3] = -0.01                                                        # group 12
    idx = index("jsmetrfast", X)
    (ids, ds, cnt), st = both(idx, Q, 2, monkeypatch)
    assert st["last_path"] == 16 and st["fast_tiles_fallback"] == 3 and st["fast_tiles"] == 19, st
    idx.close()


def test_gates(monkeypatch):
    X, Q = data(5)
    monkeypatch.setenv("NMSLIB_GPU_DIVERG_FAST", "1")
    plain = index("kldivgenslow", X)                  # the same planes and ids, no filter
    idx = index("jsdivslow", X)
    grown = idx.stats()["hbm_bytes"] - plain.stats()["hbm_bytes"]
    assert 4 * N <= grown < (N + 63) // 64 * 2 * 256 * 4, grown          # R32; less than one value plane
    plain.close()
    idx.knnQueryBatch(Q[:255], 10)
    assert idx.stats()["last_path"] == 0
    idx.knnQueryBatch(Q[:256], 10)
    assert idx.stats()["last_path"] == 16
    idx.close()
    idx = index("jsdivslow", X[:65535])
    idx.knnQueryBatch(Q[:256], 10)
    assert idx.stats()["last_path"] == 0
    idx.close()
    Y = X.copy()
    Y[1234, 2] = -1e-3
    idx = index("jsdivslow", Y)
    idx.knnQueryBatch(Q[:256], 10)
    assert idx.stats()["last_path"] == 0
    idx.close()


def test_hardware_log2_is_within_the_bounds_assumption():
    """every f32 in [2^-100, 2^128) through the raw logarithm instruction against float64 log2 (tools/probe/hwlog_probe.hip, a
    program of its own): the largest error, in ulp of the result, is what djs::kHwLog2Ulps assumes at most"""
    exe = os.path.join(ROOT, "nmslib_zig_amd", "csrc", "build", "hwlog_probe")
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    rec = json.loads(run.stdout.strip().splitlines()[-1])
    print(rec)
    assert rec["floats"] == 228 << 23 and 0 < rec["max_ulp"] <= rec["kHwLog2Ulps"], rec
