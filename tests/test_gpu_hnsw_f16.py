"""-m gpu: HNSW search with the walk on an fp16 copy of the rows and an exact f32 re-rank (gpu_rows=f16).

Both traversals run over ONE index object (the query-time parameter switches them), so the graph is the same.  On integer
grids every partial sum of both is exact, so they must agree in every bit and counter; on float data the walk may differ,
but every returned distance is the f32 distance of that row."""
import os

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import orc, refio
from tests.gpuutil import close_rel, make_index

pytestmark = pytest.mark.gpu

K = 10


def search(idx, Q, k, rows, mw=None, **qparams):
    """-> dict(ids, bits of the distances, counts, [ndc, hops, hops_up], stats) of one batch"""
    old = os.environ.get("NMSLIB_HNSW_MW")
    if mw is not None:
        os.environ["NMSLIB_HNSW_MW"] = mw
    try:
        idx.setQueryTimeParams(gpu_rows=rows, **qparams)
        ids, ds, cnt = idx.knnQueryBatch(Q, k)
        ctr = [x.copy() for x in idx.read_counters(len(Q))]
        st = idx.stats()
    finally:
        if mw is not None:
            if old is None:
                del os.environ["NMSLIB_HNSW_MW"]
            else:
                os.environ["NMSLIB_HNSW_MW"] = old
    return dict(ids=ids, ds=ds, cnt=cnt, ctr=ctr, st=st)


def same_bits(a, b, counters=True):
    np.testing.assert_array_equal(a["ids"], b["ids"])
    np.testing.assert_array_equal(a["ds"].view(np.uint32), b["ds"].view(np.uint32))
    np.testing.assert_array_equal(a["cnt"], b["cnt"])
    if counters:
        for x, y in zip(a["ctr"], b["ctr"]):
            np.testing.assert_array_equal(x, y)


def grid(n, D, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(n, D)).astype(np.float32)


def check_grid(space, D, M, efs=(16, 200), n=2000, nq=200, **qparams):
    """Integers in [-8, 8], also times 2^20 and 2^-20: every partial sum is exact in f32 (at most 260 * 256 < 2^24 units),
    and every value is exact in the scaled fp16 copy, so both traversals, and both kernels, compute the same bits."""
    X0, Q0 = grid(n, D, 100 + D), grid(nq, D, 200 + D)
    for mult in (1.0, 2.0 ** 20, 2.0 ** -20):
        X, Q = X0 * np.float32(mult), Q0 * np.float32(mult)
        idx = make_index(space, "hnsw", X, M=M, efConstruction=40, indexThreadQty=1)
        for ef in efs:
            want = search(idx, Q, K, "f32", "2", efSearch=ef, **qparams)
            assert want["st"]["last_path"] == 4
            for mw in ("2", "0"):
                got = search(idx, Q, K, "f16", mw, efSearch=ef, **qparams)
                assert got["st"]["last_path"] == 5
                same_bits(got, want)
        idx.close()


@pytest.mark.parametrize("space", ["l2", "l1", "linf", "negdotprod"])
@pytest.mark.parametrize("D", [4, 21, 100, 128, 256, 260])
def test_grid_fp16_walk_equals_f32_walk_bit_for_bit(space, D):
    check_grid(space, D, 8)


def test_grid_wide_lists_m40():
    check_grid("l2", 100, 40)


def test_grid_visited_table_overflow_route():
    """The LDS visited table overflows only where the planner had to halve it: rows of 1664 dimensions leave room for 4096
    entries instead of the 16384 it wants for maxM0 = 60 and ef = 113, and a query is re-run once it has visited more than
    7/8 of them, 3584.  High-dimensional grid rows make neighbour lists overlap little: on the host builder's graphs of these
    rows (all threads) the oracle's search evaluates 3935 rows per query on average and more than 3584 for all 40 queries.
    The LDS-table launch and the bitset launch that re-runs those queries are both fp16 launches; the re-rank runs behind
    them.  Run with each kernel in the table launch.  (1664 dimensions: six and a half steps of the fp16 gather.)"""
    n, D, nq, ef = 16000, 1664, 40, 113
    X, Q = grid(n, D, 61), grid(nq, D, 62)
    idx = make_index("l2", "hnsw", X, M=30, efConstruction=40, gpu_build=0)
    want = search(idx, Q, K, "f32", "2", efSearch=ef, algoType="v1merge")
    assert want["st"]["hnsw_redone"] > 0, "the configuration no longer overflows the visited table"
    for mw in ("2", "0"):
        got = search(idx, Q, K, "f16", mw, efSearch=ef, algoType="v1merge")
        assert got["st"]["last_path"] == 5 and got["st"]["hnsw_redone"] > 0, got["st"]
        assert got["st"]["hnsw_redone"] == want["st"]["hnsw_redone"]
        same_bits(got, want)
    idx.close()


@pytest.mark.parametrize("space,n,D", [("l2", 20000, 128), ("cosinesimil", 5000, 768)])
def test_float_data_distances_are_f32_and_recall_holds(space, n, D):
    nq, ef = 256, 128
    X, Q = refio.s_lowrank(n, D, 91), refio.s_lowrank(nq, D, 92)
    bf = make_index(space, "brute_force", X)
    gt_i, gt_d, _ = bf.knnQueryBatch(Q, 32)
    bf.close()
    idx = make_index(space, "hnsw", X, M=16, efConstruction=100, gpu_build=1)
    f32 = search(idx, Q, K, "f32", "2", efSearch=ef)
    f16 = search(idx, Q, K, "f16", "2", efSearch=ef)
    one = search(idx, Q, K, "f16", "0", efSearch=ef)
    idx.close()
    assert f32["st"]["last_path"] == 4 and f16["st"]["last_path"] == 5 and one["st"]["last_path"] == 5
    same_bits(f16, one)                                          # multi-wave and one-wave kernel: identical bits
    ids, ds = f16["ids"], f16["ds"]
    assert (f16["cnt"] == K).all()
    assert all(len(set(r)) == K for r in ids.tolist())
    assert np.all(np.diff(ds, axis=1) >= 0)
    tie = np.diff(ds, axis=1) == 0
    assert np.all(np.diff(ids, axis=1)[tie] > 0)                 # (distance, position); ids are positions here
    # every id the f32 traversal returned too carries the same distance, bit for bit
    shared = 0
    for q in range(nq):
        d32 = dict(zip(f32["ids"][q].tolist(), f32["ds"][q].view(np.uint32).tolist()))
        for i, b in zip(ids[q].tolist(), ds[q].view(np.uint32).tolist()):
            if i in d32:
                shared += 1
                assert d32[i] == b, (q, i)
    assert shared > 0.9 * nq * K
    # ... and is the oracle's distance of that pair
    # (the optimized cosine index holds normalised rows and normalises the query; the oracle's pair distance takes them so)
    def unit(v):
        return v / np.sqrt(np.sum(v * v, dtype=np.float32)) if space == "cosinesimil" else v
    want = np.array([[orc.hnsw_opt_distance(space, unit(Q[q]), unit(X[i])) for i in ids[q]] for q in range(0, nq, 4)],
                    np.float32)
    assert close_rel(ds[::4], want)
    gt_key = gt_d ** 2 if space == "l2" else gt_d
    r32 = refio.recall_nmslib(f32["ids"], gt_i, gt_key, K)
    r16 = refio.recall_nmslib(ids, gt_i, gt_key, K)
    print(f"recall@10 {space} {n}x{D}: f32 walk {r32:.4f}, fp16 walk {r16:.4f}")
    assert r16 >= r32 - 0.01, (r32, r16)


def test_fallback_routes_stay_on_f32_rows():
    """SearchOld (hybrid at ef >= 1000) and the HBM-array kernel (max(ef, k) > 1024) read the f32 rows whatever gpu_rows
    says: the f32 traversal's bits, last_path 4."""
    X, Q = refio.s_lowrank(3000, 24, 31), refio.s_lowrank(64, 24, 32)
    idx = make_index("l2", "hnsw", X, M=8, efConstruction=40, indexThreadQty=1, gpu_rows="f16")
    for qp in (dict(efSearch=1000, algoType="hybrid"), dict(efSearch=1500, algoType="v1merge")):
        want = search(idx, Q, K, "f32", **qp)
        got = search(idx, Q, K, "f16", **qp)
        assert got["st"]["last_path"] == 4
        same_bits(got, want)
    got = search(idx, Q, K, "f16", efSearch=100, algoType="hybrid")
    assert got["st"]["last_path"] == 5
    idx.close()


def test_edges_padding_rerank_clamp_switch_back_and_bytes():
    # fewer rows than k: padding and the count
    X7 = refio.s_lowrank(7, 20, 41)
    idx = make_index("l2", "hnsw", X7, M=4, efConstruction=10, indexThreadQty=1, gpu_rows="f16")
    ids, ds, cnt = idx.knnQueryBatch(refio.s_lowrank(5, 20, 42), K)
    assert idx.stats()["last_path"] == 5
    assert (cnt == 7).all() and (ids[:, 7:] == -1).all() and np.isinf(ds[:, 7:]).all()
    assert all(sorted(r[:7]) == list(range(7)) for r in ids.tolist())
    idx.close()

    n, D, nq = 4000, 44, 128
    X, Q = refio.s_lowrank(n, D, 43), refio.s_lowrank(nq, D, 44)
    idx = make_index("l2", "hnsw", X, M=8, efConstruction=40, indexThreadQty=1)
    before = search(idx, Q, K, "f32", efSearch=60)
    bytes0, mem0 = before["st"]["hbm_bytes"], nz.lib().nmslib_index_memory_usage(idx.h)
    dflt = search(idx, Q, K, "f16", efSearch=60)
    # the copy: n rows of D halves, rows padded to 16 bytes
    assert dflt["st"]["hbm_bytes"] - bytes0 == n * ((D + 7) // 8 * 8) * 2
    assert nz.lib().nmslib_index_memory_usage(idx.h) - mem0 == n * ((D + 7) // 8 * 8) * 2
    # gpu_rerank clamps to [k, max(ef, k)]
    same_bits(search(idx, Q, K, "f16", efSearch=60, gpu_rerank=1), search(idx, Q, K, "f16", efSearch=60, gpu_rerank=K))
    same_bits(search(idx, Q, K, "f16", efSearch=60, gpu_rerank=10 ** 6), dflt)
    same_bits(search(idx, Q, K, "f16", efSearch=60, gpu_rerank=60), dflt)
    # k > ef: the array holds k entries
    big = search(idx, Q, 100, "f16", efSearch=60, gpu_rerank=10 ** 6)
    assert (big["cnt"] == 100).all() and np.all(np.diff(big["ds"], axis=1) >= 0)
    # back to f32: the bits of before
    same_bits(search(idx, Q, K, "f32", efSearch=60), before)
    idx.close()

    # on grid data re-ranking only the first k entries changes nothing
    Xg, Qg = grid(2000, 21, 45), grid(100, 21, 46)
    idx = make_index("l2", "hnsw", Xg, M=8, efConstruction=40, indexThreadQty=1)
    same_bits(search(idx, Qg, K, "f16", efSearch=50, gpu_rerank=K), search(idx, Qg, K, "f16", efSearch=50, gpu_rerank=50))
    idx.close()


def test_shards_pass_the_settings_on():
    n, D, nq = 6000, 40, 64
    X, Q = refio.s_lowrank(n, D, 47), refio.s_lowrank(nq, D, 48)
    idx = make_index("l2", "hnsw", X, M=8, efConstruction=40, gpu_shards=2, gpu_rows="f16")
    idx.setQueryTimeParams(efSearch=64)
    ids, ds, cnt = idx.knnQueryBatch(Q, K)
    st = idx.stats()
    assert st["shards"] == 2 and st["last_path"] == 5
    assert st["hbm_bytes"] >= n * D * 2
    assert (cnt == K).all() and np.all(np.diff(ds, axis=1) >= 0)
    want = np.array([[orc.hnsw_opt_distance("l2", Q[q], X[i]) for i in ids[q]] for q in range(nq)], np.float32)
    assert close_rel(ds, want)
    idx.setQueryTimeParams(efSearch=64, gpu_rows="f32")
    idx.knnQueryBatch(Q, K)
    assert idx.stats()["last_path"] == 4
    idx.close()
