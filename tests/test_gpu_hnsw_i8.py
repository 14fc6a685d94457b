"""-m gpu: HNSW search with the walk on an 8-bit copy of the rows, in a kernel of its own, and the exact f32 re-rank behind
it (gpu_rows=i8).

Built like test_gpu_hnsw_f16.py: both walks run over ONE index, switched by the query-time parameter.  On integer grids in
[-8, 8] (times any power of two) rows and queries are their own codes at the scale 2^-3, the integer keys are an exact
positive multiple of the f32 walk's and every f32 partial sum is exact: both walks see the same order and the same ties --
and integer keys tie all the time -- so they must agree in every bit and counter.  On float data the walk differs, but every
returned distance is the f32 distance of that row."""
import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import orc, refio
from tests.gpuutil import close_rel, make_index

pytestmark = pytest.mark.gpu

K = 10


def search(idx, Q, k, rows, **qparams):
    """-> dict(ids, distances, counts, [ndc, hops, hops_up], stats) of one batch"""
    idx.setQueryTimeParams(gpu_rows=rows, **qparams)
    ids, ds, cnt = idx.knnQueryBatch(Q, k)
    return dict(ids=ids, ds=ds, cnt=cnt, ctr=[x.copy() for x in idx.read_counters(len(Q))], st=idx.stats())


def same_bits(a, b):
    np.testing.assert_array_equal(a["ids"], b["ids"])
    np.testing.assert_array_equal(a["ds"].view(np.uint32), b["ds"].view(np.uint32))
    np.testing.assert_array_equal(a["cnt"], b["cnt"])
    for x, y in zip(a["ctr"], b["ctr"]):
        np.testing.assert_array_equal(x, y)


def grid(n, D, seed):
    return np.random.default_rng(seed).integers(-8, 9, size=(n, D)).astype(np.float32)


def check_grid(space, D, M, efs, n=2000, nq=200, mults=(1.0, 2.0 ** 20, 2.0 ** -20)):
    """Codes in [-64, 64]: the largest key is 260 * 128^2 < 2^24, so every key is exact as a float too."""
    X0, Q0 = grid(n, D, 100 + D), grid(nq, D, 200 + D)
    for mult in mults:
        idx = make_index(space, "hnsw", X0 * np.float32(mult), M=M, efConstruction=40, indexThreadQty=1)
        for ef in efs:
            want = search(idx, Q0 * np.float32(mult), K, "f32", efSearch=ef)
            got = search(idx, Q0 * np.float32(mult), K, "i8", efSearch=ef)
            assert want["st"]["last_path"] == 4 and got["st"]["last_path"] == 13
            same_bits(got, want)
        idx.close()


@pytest.mark.parametrize("space", ["l2", "l1", "negdotprod"])
@pytest.mark.parametrize("D", [4, 16, 17, 128, 129, 260])
def test_grid_i8_walk_equals_f32_walk_bit_for_bit(space, D):
    """D: under one 16-byte load; exactly one; one byte into the second; exactly one step of the 8 lanes; one byte into the
    second step; a third step with a tail."""
    check_grid(space, D, 8, (16, 200))


def test_grid_wide_lists_m40():
    check_grid("l2", 100, 40, (16, 200))                        # lists longer than 62: the WIDE instantiations


def test_grid_emax_edges():
    check_grid("l2", 21, 8, (128, 129, 256, 257), mults=(1.0,))  # sorted array of 2, 4 and 16 entries a lane


def test_grid_pipeline_switch_changes_nothing(monkeypatch):
    """NMSLIB_HNSW_PIPE=0 takes the software pipeline across expansions out of the one-wave walk: a diagnostic that may
    change the schedule and nothing else.  On the grid ties are the rule, so both the pipelined branch and the sequential
    replay run.  NMSLIB_HNSW_MW=0: the f32 and fp16 rows are walked by hnsw_search_kernel too (both launchers read the
    switch per launch)."""
    monkeypatch.setenv("NMSLIB_HNSW_MW", "0")
    X, Q = grid(2000, 17, 117), grid(200, 17, 217)
    idx = make_index("l2", "hnsw", X, M=8, efConstruction=40, indexThreadQty=1)
    for ef in (16, 200):
        for rows in ("f32", "f16", "i8"):
            monkeypatch.delenv("NMSLIB_HNSW_PIPE", raising=False)
            piped = search(idx, Q, K, rows, efSearch=ef)
            monkeypatch.setenv("NMSLIB_HNSW_PIPE", "0")
            plain = search(idx, Q, K, rows, efSearch=ef)
            assert (piped["cnt"] == K).all() and piped["ctr"][1].min() > 0, (rows, ef)
            same_bits(plain, piped)
    idx.close()


def test_grid_visited_table_overflow_route():
    """test_gpu_hnsw_f16.py's configuration, whose docstring shows why it overflows the LDS visited table: both the table
    launch and the bitset launch that re-runs the overflowed queries are launches of the 8-bit kernel."""
    n, D, nq, ef = 16000, 1664, 40, 113
    X, Q = grid(n, D, 61), grid(nq, D, 62)
    idx = make_index("l2", "hnsw", X, M=30, efConstruction=40, gpu_build=0)
    want = search(idx, Q, K, "f32", efSearch=ef, algoType="v1merge")
    got = search(idx, Q, K, "i8", efSearch=ef, algoType="v1merge")
    idx.close()
    assert want["st"]["hnsw_redone"] > 0, "the configuration no longer overflows the visited table"
    assert got["st"]["last_path"] == 13 and got["st"]["hnsw_redone"] == want["st"]["hnsw_redone"], got["st"]
    same_bits(got, want)


FLOAT_CASES = [("l2", 20000, 128), ("cosinesimil", 5000, 768)]
# recall@10 the 8-bit walk may lose against the f32 walk over the same graph: the loss measured on these inputs, rounded up
# to a multiple of 0.005.  Measured: l2 0.9992 -> 0.9996, a loss of -0.0004; cosinesimil 1.0000 -> 1.0000, a
# loss of 0.0000; both round to 0.  Graph and walks are deterministic: there is no spread to cover.
RECALL_MARGIN = {"l2": 0.0, "cosinesimil": 0.0}


@pytest.fixture(scope="module", params=FLOAT_CASES, ids=lambda c: c[0])
def float_runs(request):
    space, n, D = request.param
    nq, ef = 256, 128
    X, Q = refio.s_lowrank(n, D, 91), refio.s_lowrank(nq, D, 92)
    bf = make_index(space, "brute_force", X)
    gt_i, gt_d, _ = bf.knnQueryBatch(Q, 32)
    bf.close()
    idx = make_index(space, "hnsw", X, M=16, efConstruction=100, gpu_build=1)
    f32 = search(idx, Q, K, "f32", efSearch=ef)
    i8 = search(idx, Q, K, "i8", efSearch=ef)
    far = search(idx, Q[:1] * np.float32(1000), K, "i8", efSearch=ef)      # saturated codes under l2
    idx.close()
    return dict(space=space, X=X, Q=Q, gt_i=gt_i, gt_d=gt_d, f32=f32, i8=i8, far=far)


def test_float_data_distances_are_the_f32_walks(float_runs):
    r = float_runs
    space, X, Q, f32, i8 = r["space"], r["X"], r["Q"], r["f32"], r["i8"]
    assert f32["st"]["last_path"] == 4 and i8["st"]["last_path"] == 13
    for run in (i8, r["far"]):
        ids, ds = run["ids"], run["ds"]
        assert (run["cnt"] == K).all() and np.isfinite(ds).all() and (ids >= 0).all()
        assert all(len(set(row)) == K for row in ids.tolist())
        assert np.all(np.diff(ds, axis=1) >= 0)
        assert np.all(np.diff(ids, axis=1)[np.diff(ds, axis=1) == 0] > 0)      # (distance, position); ids are positions here
    ids, ds = i8["ids"], i8["ds"]
    shared = 0
    for q in range(len(Q)):
        d32 = dict(zip(f32["ids"][q].tolist(), f32["ds"][q].view(np.uint32).tolist()))
        for i, b in zip(ids[q].tolist(), ds[q].view(np.uint32).tolist()):
            if i in d32:
                shared += 1
                assert d32[i] == b, (q, i)
    assert shared > 0.9 * len(Q) * K

    def unit(v):
        return v / np.sqrt(np.sum(v * v, dtype=np.float32)) if space == "cosinesimil" else v
    want = np.array([[orc.hnsw_opt_distance(space, unit(Q[q]), unit(X[i])) for i in ids[q]] for q in range(0, len(Q), 4)],
                    np.float32)
    assert close_rel(ds[::4], want)


def test_float_data_recall_against_the_f32_walk(float_runs):
    r = float_runs
    gt_key = r["gt_d"] ** 2 if r["space"] == "l2" else r["gt_d"]
    r32 = refio.recall_nmslib(r["f32"]["ids"], r["gt_i"], gt_key, K)
    r8 = refio.recall_nmslib(r["i8"]["ids"], r["gt_i"], gt_key, K)
    print(f"recall@10 {r['space']}: f32 walk {r32:.4f}, i8 walk {r8:.4f}, loss {r32 - r8:.4f}")
    assert r8 >= r32 - RECALL_MARGIN[r["space"]], (r32, r8)


def test_fall_through_routes_and_append():
    """SearchOld and the HBM-array kernel read the f32 rows whatever gpu_rows says.  An append drops the copy; the next i8
    batch packs all rows again, at the scale of all rows: the answer of a fresh index over them."""
    X, Q = refio.s_lowrank(3000, 24, 31), refio.s_lowrank(64, 24, 32)
    idx = make_index("l2", "hnsw", X, M=8, efConstruction=40, indexThreadQty=1)
    bytes0 = search(idx, Q, K, "f32", efSearch=100)["st"]["hbm_bytes"]
    got = search(idx, Q, K, "i8", efSearch=100, algoType="hybrid")
    # the copy is made at the first i8 batch and counted: per row 24 codes padded to 32 bytes, and the 16-byte slot
    assert got["st"]["last_path"] == 13 and got["st"]["hbm_bytes"] - bytes0 == 3000 * (32 + 16)
    for qp in (dict(efSearch=100, algoType="old"), dict(efSearch=1025, algoType="v1merge")):
        want, got = search(idx, Q, K, "f32", **qp), search(idx, Q, K, "i8", **qp)
        assert got["st"]["last_path"] == 4
        same_bits(got, want)
    idx.close()

    n0, n1 = 2000, 3000
    Xa = X.copy()
    Xa[n0:] *= np.float32(5)                                     # the new rows move the scale
    params = dict(M=8, efConstruction=40, gpu_build=1, gpu_rows="i8")
    idx = make_index("l2", "hnsw", Xa[:n0], np.arange(n0, dtype=np.int32), gpu_append=1, **params)
    idx.addDenseBatch(Xa[n0:], np.arange(n0, n1, dtype=np.int32))
    idx.finalize()
    assert idx.stats()["rows_appended"] == n1 - n0
    got = search(idx, Q, K, "i8", efSearch=64)
    idx.close()
    fresh = make_index("l2", "hnsw", Xa, np.arange(n1, dtype=np.int32), gpu_build_cut=n0, **params)
    want = search(fresh, Q, K, "i8", efSearch=64)
    fresh.close()
    assert got["st"]["last_path"] == 13
    same_bits(got, want)
