"""-m gpu: the l1 fast path of the exact scan (bf_l1_kernels.hip, stats()['last_path'] == 6).

The scan filters on an 8-bit copy of the rows with v_sad_u8, the survivors are re-ranked with the reference formula on
the original rows, and a per-query proof either shows that nothing was missed or sends the query's tile
to the adaptive VALU kernel.  Either way the answer must be the adaptive path's (NMSLIB_GPU_L1_FAST=0) bit for bit: ids,
distances and counts.  n = 65536 rows and 256 queries is the smallest shape that takes the path."""
import os

import numpy as np
import pytest

from tests import orc, refio
from tests.gpuutil import close_rel, make_index

pytestmark = pytest.mark.gpu

N = 65536


def _adaptive(idx, Q, k):
    os.environ["NMSLIB_GPU_L1_FAST"] = "0"
    try:
        out = idx.knnQueryBatch(Q, k)
        assert idx.stats()["last_path"] == 0
    finally:
        del os.environ["NMSLIB_GPU_L1_FAST"]
    return out


def _same(got, want):
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g.view(np.uint32) if g.dtype == np.float32 else g, w.view(np.uint32) if w.dtype == np.float32 else w)


def _oracle(X, Q, got, k, space="l1"):
    """24 queries against the oracle's full scan"""
    ids, ds, _ = got
    sel = np.unique(np.linspace(0, len(Q) - 1, 24).astype(int))
    opos, odist, _ = orc.seq_search(space, X, Q[sel], k + 22)
    assert refio.recall_nmslib(ids[sel], opos, odist, k) >= 0.999
    assert close_rel(ds[sel], odist[:, :k])


def _equal(idx, X, Q, k, path=6, fallback=0):
    """The batch through the index as it stands and through the adaptive path: equal.  path / fallback: what stats() must
    say about the first (None: anything)."""
    got = idx.knnQueryBatch(Q, k)
    st = idx.stats()
    if path is not None:
        assert st["last_path"] == path, st
    if path == 6:
        assert st["fast_tiles"] == (len(Q) + 127) // 128 and st["fast_tiles_precise"] == 0, st
        if fallback is not None:
            assert st["fast_tiles_fallback"] == fallback, st
    _same(got, _adaptive(idx, Q, k))
    _oracle(X, Q, got, k)
    return got, st


def _check(X, Q, k, **kw):
    idx = make_index("l1", "seq_search", X)
    try:
        return _equal(idx, X, Q, k, **kw)
    finally:
        idx.close()


@pytest.fixture(scope="module")
def lowrank128():
    X, Q = refio.s_lowrank(N, 128, 601), refio.s_lowrank(600, 128, 602)
    idx = make_index("l1", "seq_search", X)
    yield idx, X, Q
    idx.close()


@pytest.mark.parametrize("nq", [256, 600])
def test_l1_fast_equals_adaptive(lowrank128, nq):
    """256 queries: two tiles of 128; 600: five, the last one part padding."""
    idx, X, Q = lowrank128
    (ids, ds, cnt), _ = _equal(idx, X, Q[:nq], 10)
    assert (cnt == 10).all()


@pytest.mark.parametrize("gen", ["gauss", "lowrank"])
@pytest.mark.parametrize("D", [8, 21, 100, 128])
def test_l1_fast_dimensions(gen, D):
    """D = 8: two dwords per row; 21 and 100 (with s_gauss: no structure to help the filter): byte padding inside the last
    dword / a row count of dwords that is odd for the unrolled loop."""
    g = refio.s_gauss if gen == "gauss" else refio.s_lowrank
    _check(g(N, D, 611 + D), g(256, D, 612 + D), 10)


def test_l1_fast_dimension_limit():
    """257 dimensions: one past the scan's limit (a SAD over more bytes no longer fits the 16-bit field of its keys)."""
    D = 257
    X, Q = refio.s_lowrank(N, D, 621), refio.s_lowrank(256, D, 622)
    idx = make_index("l1", "seq_search", X)
    got = idx.knnQueryBatch(Q, 10)
    assert idx.stats()["last_path"] == 0
    _oracle(X, Q, got, 10)
    idx.close()


@pytest.mark.parametrize("k", [1, 32, 100, 129])
def test_l1_fast_values_of_k(lowrank128, k):
    """k = 32 and 100: lists of 64 keys per split; k = 129: above the plan's limit, the adaptive path."""
    idx, X, Q = lowrank128
    _equal(idx, X, Q[:256], k, path=6 if k <= 128 else 0, fallback=None)


def test_l1_fast_row_padding():
    """n = N + 37: the copy is padded to the scan's 128-row step with rows that are never listed."""
    X, Q = refio.s_lowrank(N + 37, 64, 631), refio.s_lowrank(256, 64, 632)
    Q[:37] = X[N:] + np.float32(1e-3)       # the nearest rows of these queries are the last ones before the padding
    (ids, ds, cnt), _ = _check(X, Q, 10)
    assert (cnt == 10).all() and ids.max() == N + 36 and ids.min() >= 0
    np.testing.assert_array_equal(ids[:37, 0], np.arange(N, N + 37))


@pytest.mark.parametrize("kind", ["tiny", "huge", "outlier_row", "outlier_query", "wide_range"])
def test_l1_fast_value_ranges(kind):
    """The cases of test_f32_fast_path_value_ranges.  The step scales with the data, so rows of 1e-12 or 1e12 filter like
    plain ones; one element of 3e6 ruins the step and columns spread over twelve decades leave only the widest ones in the
    bytes: there the proof fails and the tiles fall back, with the same answers."""
    n, D, nq, k = 70000, 48, 300, 10
    X, Q = refio.s_lowrank(n, D, 501), refio.s_lowrank(nq, D, 502)
    if kind == "tiny":
        X, Q = X * np.float32(1e-12), Q * np.float32(1e-12)
    elif kind == "huge":
        X, Q = X * np.float32(1e12), Q * np.float32(1e12)
    elif kind == "outlier_row":
        X = X.copy()
        X[12345, 7] = np.float32(3e6)
    elif kind == "outlier_query":
        Q = Q.copy()
        Q[5] *= np.float32(1e6)
    else:
        w = np.float32(10.0) ** np.linspace(-6, 6, D).astype(np.float32)
        X, Q = X * w, Q * w
    plain = kind in ("tiny", "huge")
    _, st = _check(X, Q, k, path=6 if plain else None, fallback=0 if plain else None)
    print(kind, st)


def test_l1_fast_exact_ties():
    """Every row is present twice: (distance, position) order, each row directly followed by its copy."""
    Y = refio.s_lowrank(N // 2, 128, 641)
    X = np.vstack([Y, Y])
    (ids, ds, cnt), st = _check(X, refio.s_lowrank(256, 128, 642), 10, fallback=None)
    print(st)
    assert (cnt == 10).all()
    np.testing.assert_array_equal(ds[:, 0::2].view(np.uint32), ds[:, 1::2].view(np.uint32))
    np.testing.assert_array_equal(ids[:, 0::2] + N // 2, ids[:, 1::2])


def test_l1_fast_integer_grid_with_a_planted_row():
    """Three symbols per column: many equal SADs and equal distances; one row planted 200 times, more copies than a split's
    list holds if they share a split."""
    rng = np.random.default_rng(651)
    X = (rng.integers(0, 3, (N, 32)) * 50).astype(np.float32)
    planted = rng.choice(N, 200, replace=False)
    X[planted] = X[planted[0]]
    Q = (rng.integers(0, 3, (256, 32)) * 50).astype(np.float32)
    Q[:8] = X[planted[0]]
    (ids, ds, cnt), st = _check(X, Q, 10, fallback=None)
    print(st)
    np.testing.assert_array_equal(ids[:8], np.tile(np.sort(planted)[:10], (8, 1)))
    assert (ds[:8] == 0).all()


def test_l1_fast_near_duplicates():
    """Clusters of 80 near-copies at 1e-3 noise: a cluster sits in one split and overflows its list.  Proven or fallen
    back, the answer is the adaptive path's and stays inside the query's cluster."""
    rng = np.random.default_rng(661)
    C = rng.standard_normal((820, 64)).astype(np.float32)
    X = (np.repeat(C, 80, axis=0) + 1e-3 * rng.standard_normal((820 * 80, 64))).astype(np.float32)[:N]
    cq = rng.integers(0, 819, 256)
    Q = (C[cq] + 1e-3 * rng.standard_normal((256, 64))).astype(np.float32)
    (ids, ds, cnt), st = _check(X, Q, 10, fallback=None)
    print(st)
    assert (ids // 80 == cq[:, None]).all()


def test_l1_fast_is_deterministic(lowrank128):
    idx, X, Q = lowrank128
    first = idx.knnQueryBatch(Q, 10)
    assert idx.stats()["last_path"] == 6
    for _ in range(10):
        _same(idx.knnQueryBatch(Q, 10), first)


def test_l1_fast_gates(lowrank128):
    """255 queries, 65535 rows and linf stay on the adaptive kernel."""
    idx, X, Q = lowrank128
    idx.knnQueryBatch(Q[:255], 10)
    assert idx.stats()["last_path"] == 0
    for space, rows in (("l1", X[:N - 1]), ("linf", X)):
        other = make_index(space, "seq_search", rows)
        got = other.knnQueryBatch(Q[:256], 10)
        assert other.stats()["last_path"] == 0, space
        _oracle(rows, Q[:256], got, 10, space)
        other.close()


def test_l1_fast_behind_shards():
    """gpu_shards=2 over 2N rows: each shard has its own step and offsets; the merged answer is the unsharded index's."""
    X, Q = refio.s_lowrank(2 * N, 32, 671), refio.s_lowrank(256, 32, 672)
    X[N:] *= np.float32(3.0)                 # the second shard's ranges differ from the first's
    one = make_index("l1", "seq_search", X, gpu_shards=1)
    two = make_index("l1", "seq_search", X, gpu_shards=2)
    try:
        want = one.knnQueryBatch(Q, 10)
        assert one.stats()["last_path"] == 6
        got = two.knnQueryBatch(Q, 10)
        st = two.stats()
        assert st["shards"] == 2 and st["last_path"] == 6, st
        _same(got, want)
        _oracle(X, Q, got, 10)
    finally:
        one.close()
        two.close()


def test_l1_fast_copy_is_counted(lowrank128):
    """hbm_bytes holds the f32 rows and the byte copy: at least n * D * 5."""
    idx, X, Q = lowrank128
    idx.knnQueryBatch(Q[:256], 10)
    st = idx.stats()
    assert st["last_path"] == 6 and st["hbm_bytes"] >= N * 128 * 5, st
