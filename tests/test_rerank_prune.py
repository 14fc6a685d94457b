"""-m gpu: the cut in the list re-rank of the exact f32 scan (bf_rerank_f32_list_kernel).

The one-product scan's hit entries carry the largest scan score of their rows; the re-rank fetches only the entries
that can still hold a top-k row.  Whatever the cut drops, the answer must stay the adaptive path's (NMSLIB_GPU_F32_FAST=0)
bit for bit: ids, distances and counts.  n = 65536 rows and >= 256 queries is the smallest shape that takes the fast
path."""
import os

import numpy as np
import pytest

from tests import refio
from tests.gpuutil import make_index

pytestmark = pytest.mark.gpu

N = 65536


def _adaptive(idx, Q, k):
    """The same batch through the adaptive path, forced the way tests/test_gpu_bruteforce.py forces it."""
    os.environ["NMSLIB_GPU_F32_FAST"] = "0"
    try:
        out = idx.knnQueryBatch(Q, k)
        assert idx.stats()["last_path"] == 0
    finally:
        del os.environ["NMSLIB_GPU_F32_FAST"]
    return out


def _fast(idx, Q, k):
    out = idx.knnQueryBatch(Q, k)
    assert idx.stats()["last_path"] == 1, idx.stats()
    return out


def _same(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)


def _check(space, X, Q, k):
    idx = make_index(space, "seq_search", X)
    try:
        got = _fast(idx, Q, k)
        st = idx.stats()
        _same(got, _adaptive(idx, Q, k))
    finally:
        idx.close()
    return got, st


@pytest.fixture(scope="module")
def lowrank128():
    """One index over plain low-rank rows (D = 128, l2), 600 queries, and the adaptive path's answers for k = 10."""
    X, Q = refio.s_lowrank(N, 128, 301), refio.s_lowrank(600, 128, 302)
    idx = make_index("l2", "seq_search", X)
    ref600 = _adaptive(idx, Q, 10)
    yield idx, Q, ref600
    idx.close()


@pytest.mark.parametrize("nq", [256, 600])
def test_cut_keeps_the_adaptive_answer_l2(lowrank128, nq):
    """256 queries: one tile; 600: three tiles of 256 (one MFMA per K-step and query group), the last one part padding."""
    idx, Q, ref600 = lowrank128
    got = _fast(idx, Q[:nq], 10)
    assert idx.stats()["fast_tiles_fallback"] == 0, idx.stats()
    _same(got, ref600 if nq == 600 else _adaptive(idx, Q[:nq], 10))


def test_cut_at_the_top_of_the_register_sort_branch(lowrank128):
    """k = 32: the largest k of the first-k selection in registers; want = 36 entries decide kappa."""
    idx, Q, _ = lowrank128
    _same(_fast(idx, Q[:256], 32), _adaptive(idx, Q[:256], 32))


@pytest.mark.parametrize("D", [32, 200])
def test_cut_one_chunk_and_k_chunked_scans(D):
    """D = 32: one chunk, mostly padding columns; D = 200: the K-chunked scan (two chunks of 128)."""
    _check("l2", refio.s_lowrank(N, D, 311 + D), refio.s_lowrank(256, D, 312 + D), 10)


@pytest.mark.parametrize("space", ["negdotprod", "cosinesimil"])
def test_cut_other_score_modes(space):
    _check(space, refio.s_lowrank(N, 128, 321), refio.s_lowrank(256, 128, 322), 10)


def test_cut_near_duplicates():
    """Clusters of 80 copies at 1e-3 noise (built like test_f32_fast_path_near_duplicates_stay_exact): masks hold several
    rows per entry and the gaps between a cluster's scores fall inside E1.  Proven or fallen back, the answer is the
    adaptive path's."""
    rng = np.random.default_rng(191)
    C = rng.standard_normal((820, 64)).astype(np.float32)
    X = (np.repeat(C, 80, axis=0) + 1e-3 * rng.standard_normal((820 * 80, 64))).astype(np.float32)[:N]
    cq = rng.integers(0, 819, 256)
    Q = (C[cq] + 1e-3 * rng.standard_normal((256, 64))).astype(np.float32)
    (ids, ds, cnt), _ = _check("l2", X, Q, 10)
    assert (ids // 80 == cq[:, None]).all()


def test_cut_exact_ties():
    """Every row is present twice: each entry's best score is shared by a row of another entry.  (distance, position)
    order."""
    Y = refio.s_lowrank(N // 2, 128, 331)
    X = np.vstack([Y, Y])
    (ids, ds, cnt), _ = _check("l2", X, refio.s_lowrank(256, 128, 332), 10)
    assert (cnt == 10).all()
    assert (np.diff(ds, axis=1) >= 0).all()
    tied = np.diff(ds, axis=1) == 0
    assert (np.diff(ids, axis=1)[tied] > 0).all()
    np.testing.assert_array_equal(ids[:, 0::2] + N // 2, ids[:, 1::2])     # a row, then its copy


def test_split_product_tiles_unchanged(lowrank128, monkeypatch):
    """NMSLIB_GPU_F32_TERMS=3: every tile through the split-product scan, whose entries stay one word: no cut."""
    idx, Q, ref600 = lowrank128
    monkeypatch.setenv("NMSLIB_GPU_F32_TERMS", "3")
    got = _fast(idx, Q, 10)
    st = idx.stats()
    assert st["fast_tiles_precise"] == st["fast_tiles"] > 0, st
    _same(got, ref600)


def test_cut_is_deterministic(lowrank128):
    idx, Q, ref600 = lowrank128
    for _ in range(10):
        _same(_fast(idx, Q, 10), ref600)
