"""-m gpu: exact k-NN for 512 < k <= 4096 on the batched scan (last_path 12).  Every answer is compared, bit
for bit, with the per-query sort's (NMSLIB_GPU_BIGK_BATCH=0, last_path 5) and with the oracle's scan.  The row and batch
gates are opened (NMSLIB_GPU_BIGK_MIN_ROWS=1, NMSLIB_GPU_BIGK_MIN_QUERIES=1) unless a case is about them."""
import numpy as np
import pytest

from . import orc, refio
from .gpuutil import close_rel, enqueue_knn, expect_path, make_index, same_bits

pytestmark = pytest.mark.gpu

KINDS = [("l2", 5), ("l1", 64), ("linf", 65), ("cosinesimil", 129), ("angulardist", 192), ("negdotprod", 256),
         ("l2sqr_sift", 128)]
N, NQ = 9001, 33


@pytest.fixture
def gates(monkeypatch):
    monkeypatch.setenv("NMSLIB_GPU_BIGK_MIN_ROWS", "1")
    monkeypatch.setenv("NMSLIB_GPU_BIGK_MIN_QUERIES", "1")
    return monkeypatch


def rows_of(space, D, n, seed):
    return refio.s_sift_like(n, seed) if space == "l2sqr_sift" else refio.s_lowrank(n, D, seed)


def both_routes(idx, Q, k, mp, path=12, **stats):
    """-> the batch's answer, checked to be `path`'s and equal to the per-query sort's"""
    got = idx.knnQueryBatch(Q, k)
    st = expect_path(idx, path, **stats)
    mp.setenv("NMSLIB_GPU_BIGK_BATCH", "0")
    old = idx.knnQueryBatch(Q, k)
    expect_path(idx, 5)
    mp.delenv("NMSLIB_GPU_BIGK_BATCH")
    same_bits(got, old)
    return got, st


def check_oracle(space, X, Q, k, got, sel):
    """the comparators of the big-k cases in test_gpu_scan_switches"""
    ids, ds, cnt = got
    assert (cnt == k).all()
    if space == "l2sqr_sift":
        opos, odist, _ = orc.seq_search(space, X, Q[sel], k)
        np.testing.assert_array_equal(ds[sel], odist)
        np.testing.assert_array_equal(ids[sel], opos)
        return
    opos, odist, _ = orc.seq_search(space, X, Q[sel], k + 22)
    assert refio.recall_nmslib(ids[sel], opos, odist, k) >= 0.999
    rtol, atol = (1e-4, 1e-5) if space == "angulardist" else (1e-5, 1e-6)
    assert close_rel(ds[sel], odist[:, :k], rtol=rtol, atol=atol)


@pytest.fixture(scope="module")
def kinds():
    made = {}

    def get(space, D):
        if space not in made:
            X = rows_of(space, D, N, 1301)
            made[space] = (make_index(space, "seq_search", X), X, rows_of(space, D, NQ, 1302))
        return made[space]
    yield get
    for v in made.values():
        v[0].close()


@pytest.mark.parametrize("k", [513, 1000, 4096])
@pytest.mark.parametrize("space,D", KINDS)
def test_every_kind(kinds, gates, space, D, k):
    """9001 rows end in a ragged 64-row block and are all sampled (stride 1); 33 queries: a ragged second tile"""
    idx, X, Q = kinds(space, D)
    got, _ = both_routes(idx, Q, k, gates, fast_tiles=NQ, fast_tiles_fallback=0, fast_tiles_precise=0)
    check_oracle(space, X, Q, k, got, [0, 31, 32])


def test_route_edges(kinds, gates):
    idx, X, Q = kinds("l2", 5)
    idx.knnQueryBatch(Q, 512)
    assert idx.stats()["last_path"] not in (5, 12)
    idx.knnQueryBatch(Q, 4097)
    expect_path(idx, 5)
    small = make_index("l2", "seq_search", X[:8191])
    small.knnQueryBatch(Q, 4096)                  # n < 2 k
    expect_path(small, 5)
    small.close()
    wide = make_index("l2", "seq_search", refio.s_lowrank(2000, 257, 1303))
    wide.knnQueryBatch(refio.s_lowrank(NQ, 257, 1304), 513)
    expect_path(wide, 5)
    wide.close()
    gates.delenv("NMSLIB_GPU_BIGK_MIN_ROWS")      # the default row gate
    big = make_index("l2", "seq_search", refio.s_lowrank(20000, 5, 1305))
    big.knnQueryBatch(Q, 513)
    expect_path(big, 5)
    big.close()


# ---- 40 000 rows: 625 blocks, every third one sampled, rank 261 at k = 600 ----
BIG_N, BIG_K = 40000, 600


def grid_rows(rng, far_from):
    """integer rows (exact distances) at graded squared distances 10 000 .. from the origin"""
    X = rng.integers(-3, 4, (BIG_N, 8)).astype(np.float32)
    X[:, 0] = far_from + np.arange(BIG_N) % 997
    return X


def test_sample_and_ties_at_the_cut(gates):
    """twenty copies of one row straddle rank 600 of query 0: positions decide"""
    rng = np.random.default_rng(1311)
    X = rng.integers(0, 64, (BIG_N, 8)).astype(np.float32)
    Q = rng.integers(0, 64, (5, 8)).astype(np.float32)
    d = ((X.astype(np.int64) - Q[0].astype(np.int64)) ** 2).sum(1)
    order = np.argsort(d, kind="stable")
    X[rng.permutation(BIG_N)[:20]] = X[order[BIG_K - 5]]
    d = ((X.astype(np.int64) - Q[0].astype(np.int64)) ** 2).sum(1)
    order = np.argsort(d, kind="stable")
    assert d[order[BIG_K - 1]] == d[order[BIG_K]]                     # the cut goes through equal distances
    ext = (np.arange(BIG_N, dtype=np.int32) * 7 + 3)[::-1].copy()
    idx = make_index("l2", "seq_search", X, ext)
    got, _ = both_routes(idx, Q, BIG_K, gates, fast_tiles=5, fast_tiles_fallback=0)
    np.testing.assert_array_equal(got[0][0], ext[order[:BIG_K]])
    np.testing.assert_array_equal(got[1][0], np.sqrt(d[order[:BIG_K]].astype(np.float32)))
    idx.close()


def test_underflow_is_redone(gates):
    """400 rows near the origin, 300 of them in sampled blocks: the 261st sample distance lies among them, the radius
    admits 400 < 600 rows.  Queries 0 and 2 sit there; query 1 is ordinary."""
    rng = np.random.default_rng(1312)
    X = grid_rows(rng, 100)
    pos = np.arange(BIG_N)
    sampled, other = pos[pos // 64 % 3 == 0], pos[pos // 64 % 3 != 0]
    near = np.r_[rng.permutation(sampled)[:300], rng.permutation(other)[:100]]
    X[near] = rng.integers(-1, 2, (400, 8)).astype(np.float32)
    Q = np.zeros((3, 8), np.float32)
    Q[1] = [500, 1, -2, 0, 3, 1, 0, -1]
    Q[2, 1] = 1
    idx = make_index("l2", "seq_search", X)
    got, _ = both_routes(idx, Q, BIG_K, gates, fast_tiles=3, fast_tiles_fallback=2)
    check_oracle("l2", X, Q, BIG_K, got, [0, 1, 2])
    idx.close()


def test_overflow_is_redone(gates):
    """20 000 identical rows nearest to query 0: more than a list holds; among them positions decide"""
    rng = np.random.default_rng(1313)
    X = grid_rows(rng, 100)
    same = np.sort(rng.permutation(BIG_N)[:20000])
    X[same] = [1, 0, 0, 0, 0, 0, 0, 2]
    Q = np.array([[1, 0, 0, 0, 0, 0, 0, 0], [400, 0, 1, 0, 0, 2, 0, 0]], np.float32)
    idx = make_index("l2", "seq_search", X)
    got, _ = both_routes(idx, Q, BIG_K, gates, fast_tiles=2, fast_tiles_fallback=1)
    np.testing.assert_array_equal(got[0][0], same[:BIG_K])
    assert (got[1][0] == 2).all()
    idx.close()


def test_two_device_batches_back_to_back(kinds, gates):
    """a foreign stream, no host synchronisation between the calls; the second batch is larger: the workspaces grow"""
    import torch
    idx, X, Q = kinds("l2", 5)
    more = rows_of("l2", 5, 70, 1314)
    stream = torch.cuda.Stream()
    first = enqueue_knn(idx, Q[:7], 600, stream)
    second = enqueue_knn(idx, more, 513, stream)
    stream.synchronize()
    expect_path(idx, 12, fast_tiles=70)
    gates.setenv("NMSLIB_GPU_BIGK_BATCH", "0")
    same_bits(first.result(), idx.knnQueryBatch(Q[:7], 600))
    same_bits(second.result(), idx.knnQueryBatch(more, 513))
    expect_path(idx, 5)


def test_three_slices(kinds, gates):
    """room for 14 lists: 33 queries go through as 14 + 14 + 5"""
    idx, X, Q = kinds("l2sqr_sift", 128)
    gates.setenv("NMSLIB_GPU_BIGK_WS_BYTES", str(14 * 16384 * 8))
    both_routes(idx, Q, 700, gates, fast_tiles=5, fast_tiles_fallback=0)
