"""-m gpu: every instantiation of the list re-rank of the exact f32 scan (bf_rerank_f32_list_kernel<space, centred, long>).

The kernel is compiled once per score family and row-length class so that the served shape fits four workgroups on a
CU (DESIGN.md 4.1b "Residency").  Whichever instantiation serves an index, the answer must stay the adaptive path's
(NMSLIB_GPU_F32_FAST=0) bit for bit -- ids, distances and counts -- with no tile falling back.  n = 65536 rows and
256 queries is the smallest shape that takes the fast path."""
import os

import numpy as np
import pytest

from tests import refio
from tests.gpuutil import make_index, same_bits

pytestmark = pytest.mark.gpu

N = 65536
SPACES = ["l2", "negdotprod", "cosinesimil", "angulardist"]


def _adaptive(idx, Q, k):
    os.environ["NMSLIB_GPU_F32_FAST"] = "0"
    try:
        out = idx.knnQueryBatch(Q, k)
        assert idx.stats()["last_path"] == 0, idx.stats()
    finally:
        del os.environ["NMSLIB_GPU_F32_FAST"]
    return out


def _fast(idx, Q, k):
    out = idx.knnQueryBatch(Q, k)
    st = idx.stats()
    print(st)
    assert st["last_path"] == 1, st
    assert st["fast_tiles"] > 0 and st["fast_tiles_fallback"] == 0, st
    return out, st


def _check(space, X, Q, k, ids=None):
    idx = make_index(space, "seq_search", X, ids)
    try:
        got, st = _fast(idx, Q, k)
        same_bits(got, _adaptive(idx, Q, k))
    finally:
        idx.close()
    return got, st


@pytest.fixture(scope="module")
def rows():
    """Plain low-rank rows and 1025 queries per row length, made once and left unchanged."""
    return {D: (refio.s_lowrank(N, D, 501 + D), refio.s_lowrank(1025, D, 502 + D)) for D in (100, 128, 200)}


@pytest.fixture(scope="module")
def l2_128(rows):
    """One l2 index over the D = 128 rows, and the adaptive path's answer to the first 256 queries, k = 10."""
    X, Q = rows[128]
    idx = make_index("l2", "seq_search", X)
    ref = _adaptive(idx, Q[:256], 10)
    yield idx, X, Q, ref
    idx.close()


@pytest.mark.parametrize("D", [128, 100])
@pytest.mark.parametrize("space", SPACES)
def test_each_score_family_short_rows(rows, space, D):
    """D = 128: every column real; D = 100: the last 28 columns of the second 64-dimension step are predicated off."""
    X, Q = rows[D]
    _check(space, X, Q[:256], 10)


@pytest.mark.parametrize("space", ["cosinesimil", "angulardist"])
def test_centred_cosine(space):
    """Rows with a common offset: the selection runs on centred, augmented rows and the re-rank's proof reads qaux."""
    X = (refio.s_lowrank(N, 32, 511) + np.float32(1.5)).astype(np.float32)
    Q = (refio.s_lowrank(256, 32, 512) + np.float32(1.5)).astype(np.float32)
    _check(space, X, Q, 10)


def test_long_rows(rows):
    """D = 200: the instantiation that walks a row in 64-dimension steps (two chunks of 128 in the scan)."""
    X, Q = rows[200]
    _check("l2", X, Q[:256], 10)


def test_more_queries_than_resident_workgroups(rows):
    """1025 workgroups: one more than 256 CUs hold at four per CU."""
    X, Q = rows[128]
    _check("l2", X, Q, 10)


def test_wide_order_statistic(l2_128):
    """k = 100: want = 112 entries decide kappa among more than 256 listed positions per query (16 keys per lane)."""
    idx, X, Q, _ = l2_128
    got, st = _fast(idx, Q[:256], 100)
    same_bits(got, _adaptive(idx, Q[:256], 100))
    assert (got[2] == 100).all()


def test_split_product_tiles(l2_128, monkeypatch):
    """NMSLIB_GPU_F32_TERMS=3: every tile through the split-product scan; one-word entries, same instantiation."""
    idx, X, Q, ref = l2_128
    monkeypatch.setenv("NMSLIB_GPU_F32_TERMS", "3")
    got, st = _fast(idx, Q[:256], 10)
    assert st["fast_tiles_precise"] == st["fast_tiles"], st
    same_bits(got, ref)


def test_external_ids_that_are_not_row_numbers(l2_128):
    """A permutation (shifted) as ids: the output holds ids[position], in the (distance, position) order."""
    idx, X, Q, ref = l2_128
    ext = (np.random.default_rng(521).permutation(N) + 1000).astype(np.int32)
    got, _ = _check("l2", X, Q[:256], 10, ids=ext)
    np.testing.assert_array_equal(got[0], ext[ref[0]])
    same_bits((ref[0], got[1], got[2]), ref)
