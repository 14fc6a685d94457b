"""-m gpu: rows deleted from an HNSW index (nmslib_gpu_delete_ids).

The yardstick is exact.  On the same index before the delete, the batch is searched for k' = max(efSearch, k) results.
On the host the deleted rows' ids are dropped from those lists and the lists are cut to k.  After the delete, ids,
distances and counts must be those BITS, and ndc / hops / hops_up the before-run's: deleted nodes stay in the graph as
stepping stones, the walk is the same walk, and the filter takes its first k live results in their order."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import refio
from tests.gpuutil import enqueue_knn, make_index, same_bits

from . import delete_poison_child

pytestmark = pytest.mark.gpu

N, D, K, NQ = 3000, 16, 10, 70
HOST = dict(M=8, efConstruction=60, indexThreadQty=1)
GPU = dict(M=8, efConstruction=60, gpu_build=1)
EFS = (4, 40, 200)                     # ef < k; the ordinary case; k' no multiple of 64


def ext_ids(n):
    """external ids that are no positions (a result that carries positions shows)"""
    return (5 * np.arange(n) + 7).astype(np.int32)


def run(idx, Q, k, env=None):
    """-> (ids, dists, counts), (ndc, hops, hops_up)"""
    old = {name: os.environ.get(name) for name in (env or {})}
    os.environ.update(env or {})
    try:
        res = idx.knnQueryBatch(Q, k)
        ctr = tuple(x.copy() for x in idx.read_counters(len(Q)))
    finally:
        for name, v in old.items():
            if v is None:
                del os.environ[name]
            else:
                os.environ[name] = v
    return res, ctr


def filtered(before, dead_ids, k):
    """the first k entries of every list of `before` (ids, dists, counts of the k'-result search) whose id is not deleted"""
    bids, bds, bcnt = before
    nq = len(bcnt)
    ids = np.full((nq, k), -1, np.int32)
    ds = np.full((nq, k), np.inf, np.float32)
    cnt = np.zeros(nq, np.int32)
    for q in range(nq):
        live = np.nonzero(~np.isin(bids[q, :bcnt[q]], dead_ids))[0][:k]
        ids[q, :len(live)], ds[q, :len(live)], cnt[q] = bids[q, live], bds[q, live], len(live)
    return ids, ds, cnt


def check_delete(idx, Q, dead_ids, settings, k=K, dead_from=None):
    """settings: (efSearch, more query parameters, environment) per round.  The before-runs at k' on `idx`, the delete, the
    after-runs at k against the host-filtered lists.  dead_from(before-run of the first setting) -> ids, when given.
    -> the after-runs"""
    before = []
    for ef, params, env in settings:
        idx.setQueryTimeParams(efSearch=ef, **params)
        before.append(run(idx, Q, max(ef, k), env))
    if dead_from is not None:
        dead_ids = dead_from(before[0][0])
    dead_ids = np.asarray(dead_ids, np.int32)
    assert idx.deleteIds(dead_ids) == len(np.unique(dead_ids)) == idx.deletedRows()
    after = []
    for (ef, params, env), (bres, bctr) in zip(settings, before):
        idx.setQueryTimeParams(efSearch=ef, **params)
        res, ctr = run(idx, Q, k, env)
        want = filtered(bres, dead_ids, k)
        same_bits(res, want)
        assert not np.isin(res[0], dead_ids).any()
        assert (res[0][np.arange(k)[None, :] >= res[2][:, None]] == -1).all()
        assert np.isposinf(res[1][np.arange(k)[None, :] >= res[2][:, None]]).all()
        for name, got, w in zip(("ndc", "hops", "hops_up"), ctr, bctr):
            np.testing.assert_array_equal(got, w, err_msg=f"efSearch={ef} {name}")
        after.append(res)
    return after


@pytest.fixture(scope="module")
def data():
    return dict(X=refio.s_lowrank(N, D, 801), Q=refio.s_lowrank(NQ, D, 802), ids=ext_ids(N))


def plain(efs=EFS, **params):
    return [(ef, params, None) for ef in efs]


def random_dead(n, share, seed, ids):
    return ids[np.random.default_rng(seed).permutation(n)[:int(n * share)]]


DELETE_SETS = {
    "random-30-percent": lambda ids: random_dead(N, 0.3, 803, ids),
    "word-edges": lambda ids: ids[[0, 31, 32, 63, 64, N - 1]],
    "all-but-five": lambda ids: np.delete(ids, np.random.default_rng(804).permutation(N)[:5]),
    "all": lambda ids: ids,
}


@pytest.mark.parametrize("which", list(DELETE_SETS))
def test_delete_sets(which, data):
    assert N % 32 != 0
    idx = make_index("l2", "hnsw", data["X"], data["ids"], **HOST)
    after = check_delete(idx, data["Q"], DELETE_SETS[which](data["ids"]), plain())
    if which == "all-but-five":
        assert all((a[2] <= 5).all() for a in after) and (after[2][2] > 0).any()
    if which == "all":
        assert all((a[2] == 0).all() for a in after)
    assert idx.stats()["last_path"] == 4 and idx.dataQty() == N
    idx.close()


def test_every_querys_nearest_row_is_deleted(data):
    """the filter acts on every query: rank 0 of every before-list goes"""
    idx = make_index("l2", "hnsw", data["X"], data["ids"], **HOST)
    first = {}

    def nearest(before):
        first["ids"] = before[0][:, 0].copy()
        return np.unique(first["ids"])

    after = check_delete(idx, data["Q"], None, plain((40, 4, 200)), dead_from=nearest)
    assert (after[0][0][:, 0] != first["ids"]).all()
    idx.close()


PATHS = {
    # the two LDS kernels
    "one-wave": ("l2", HOST, [(40, {}, {"NMSLIB_HNSW_MW": "0"}), (200, {}, {"NMSLIB_HNSW_MW": "0"})], 4),
    "multi-wave": ("l2", HOST, [(40, {}, {"NMSLIB_HNSW_MW": "2"}), (200, {}, {"NMSLIB_HNSW_MW": "2"})], 4),
    "old": ("l2", HOST, plain((4, 40), algoType="old"), 4),
    "hbm-array": ("l2", HOST, plain((1100,), algoType="v1merge"), 4),
    "old-by-ef": ("l2", HOST, plain((1100,)), 4),
    "gpu-builder": ("l2", GPU, plain(), 4),
    "cosinesimil": ("cosinesimil", HOST, plain(), 4),
    "l2sqr_sift": ("l2sqr_sift", HOST, plain(), 4),
    "f16": ("l2", dict(HOST, gpu_rows="f16"), plain(), 5),
    "f16-rerank-20": ("l2", dict(HOST, gpu_rows="f16"), plain(EFS, gpu_rerank=20), 5),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_paths(path, data):
    space, build, settings, last_path = PATHS[path]
    if space == "l2sqr_sift":
        X, Q = refio.s_sift_like(N, 805), refio.s_sift_like(NQ, 806)
    else:
        X, Q = data["X"], data["Q"]
    idx = make_index(space, "hnsw", X, data["ids"], **build)
    assert idx.graphBuilder() == (2 if build is GPU else 1)
    check_delete(idx, Q, random_dead(N, 0.3, 807, data["ids"]), settings)
    assert idx.stats()["last_path"] == last_path
    idx.close()


@pytest.mark.parametrize("load_data", [True, False], ids=["with-data", "graph-only"])
def test_a_loaded_graph(load_data, data, tmp_path):
    src = make_index("l2", "hnsw", data["X"], data["ids"], **HOST)
    path = str(tmp_path / "saved.idx")
    src.save(path, save_data=True)
    src.close()
    idx = nz.Index.load(path, load_data=load_data)
    assert idx.graphBuilder() == 0 and idx.dataQty() == N
    check_delete(idx, data["Q"], random_dead(N, 0.3, 816, data["ids"]), plain())
    idx.close()


def test_fewer_rows_than_the_search_returns():
    """50 rows at efSearch = 200: the walk writes fewer than k' entries, nothing behind them is read"""
    X, Q = refio.s_gauss(50, 8, 808), refio.s_gauss(NQ, 8, 809)
    ids = ext_ids(50)
    idx = make_index("l2", "hnsw", X, ids, M=4, efConstruction=20, indexThreadQty=1)
    after = check_delete(idx, Q, ids[::3], plain((200,)))
    assert (after[0][2] == K).all()
    idx.close()


def test_an_index_without_tombstones_answers_as_before(data):
    """a twin on which no delete entry is ever called; also after deleteIds([]) and a delete of ids no row carries"""
    a = make_index("l2", "hnsw", data["X"], data["ids"], **HOST)
    twin = make_index("l2", "hnsw", data["X"], data["ids"], **HOST)
    for step in (lambda: a.deletedRows(), lambda: a.deleteIds([]), lambda: a.deleteIds([1, 2, 3, 4, 6, -5])):
        assert step() == 0
        for ef in EFS + (1100,):
            for i in (a, twin):
                i.setQueryTimeParams(efSearch=ef)
            (ra, ca), (rt, ct) = run(a, data["Q"], K), run(twin, data["Q"], K)
            same_bits(ra, rt)
            for x, y in zip(ca, ct):
                np.testing.assert_array_equal(x, y)
    assert a.stats()["hbm_bytes"] == twin.stats()["hbm_bytes"]           # no bitset was made
    a.close()
    twin.close()


def test_slices_of_a_large_batch():
    """70 000 queries: both sides of the cut at 65 536, results and counters at their offsets"""
    n, nq_small, nq_big, ef = 200, 1024, 70000, 32
    X, Q = refio.s_lowrank(n, 8, 810), refio.s_lowrank(nq_small, 8, 811)
    ids = ext_ids(n)
    dead = random_dead(n, 0.3, 812, ids)
    assert len(dead) == 60
    idx = make_index("l2", "hnsw", X, ids, M=8, efConstruction=40, indexThreadQty=1)
    idx.setQueryTimeParams(efSearch=ef)
    before, bctr = run(idx, Q, ef)
    assert idx.deleteIds(dead) == 60
    src = np.arange(nq_big) % nq_small
    big = np.ascontiguousarray(Q[src])
    res, ctr = run(idx, big, K)
    want = filtered(before, dead, K)
    same_bits(res, tuple(w[src] for w in want))
    for name, got, w in zip(("ndc", "hops", "hops_up"), ctr, bctr):
        assert got.shape == (nq_big,)
        np.testing.assert_array_equal(got, w[src], err_msg=name)
    idx.close()


def test_device_entry_batch_delete_batch_on_a_foreign_stream(data):
    """batch, delete, batch on one side stream and no host synchronisation in between: the first batch's buffers hold the
    unfiltered answer, the second's the filtered one.  The stream is kept busy while the three calls are made: 100 passes
    that read and write a 256 MB tensor take no less than 6.4 ms at the 8 TB/s of HBM3E, a batch of this shape under 1 ms
    (tests/test_gpu_device_entry.py), so the first batch has not started when the delete is called."""
    import torch
    X, Q, ids = data["X"], data["Q"], data["ids"]
    idx = make_index("l2", "hnsw", X, ids, **HOST)
    idx.setQueryTimeParams(efSearch=40)
    unfiltered = idx.knnQueryBatch(Q, K)
    before = idx.knnQueryBatch(Q, 40)
    dead = np.unique(unfiltered[0][:, 0])
    a = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()

    def busy(qbuf):
        for _ in range(100):
            a.add_(1.0)

    first = enqueue_knn(idx, Q, K, stream, before=busy)
    assert idx.deleteIds(dead) == len(dead)
    second = enqueue_knn(idx, Q, K, stream)
    stream.synchronize()
    same_bits(first.result(), unfiltered)
    same_bits(second.result(), filtered(before, dead, K))
    idx.close()


def test_append_after_delete():
    n0, n1, d = 2000, 2500, 16
    build = dict(GPU, gpu_build_batch=256)
    X, Q = refio.s_lowrank(n1, d, 813), refio.s_lowrank(NQ, d, 814)
    ids = ext_ids(n1)
    dead = random_dead(n0, 0.15, 815, ids)                       # 300 ids, all of old rows
    assert len(dead) == 300
    ids[n0:n0 + 100] = dead[:100]                                # 100 new rows come under deleted ids
    dead_pos = np.nonzero(np.isin(ids[:n0], dead))[0]
    # the appended index: build, delete, add
    a = make_index("l2", "hnsw", X[:n0], ids[:n0], gpu_append=1, **build)
    assert a.deleteIds(dead) == 300
    a.addDenseBatch(X[n0:], ids[n0:])
    a.finalize()
    st = a.stats()
    assert st["rows_appended"] == 500 and a.graphBuilder() == 2 and a.deletedRows() == 300, st
    # the twin: the same rows marked (host state, before any row of the second part exists), then the cut build of all rows
    twin = nz.Index("l2", "hnsw")
    twin.addDenseBatch(X[:n0], ids[:n0])
    assert twin.deleteIds(dead) == 300
    twin.addDenseBatch(X[n0:], ids[n0:])
    twin.buildIndex(gpu_build_cut=n0, **build)
    assert twin.deletedRows() == 300 and twin.stats()["rows_appended"] == 0
    # the same graph without tombstones, under ids that are positions: the before-run
    clean = make_index("l2", "hnsw", X, None, gpu_build_cut=n0, **build)
    for ef in (20, 64):
        for i in (a, twin, clean):
            i.setQueryTimeParams(efSearch=ef)
        for queries in (Q, X[n0:n0 + 100]):
            (bpos, bds, bcnt), bctr = run(clean, queries, max(ef, K))
            wpos, wds, wcnt = filtered((bpos, bds, bcnt), dead_pos, K)
            want = (np.where(wpos >= 0, ids[np.maximum(wpos, 0)], -1).astype(np.int32), wds, wcnt)
            (ra, ca), (rt, ct) = run(a, queries, K), run(twin, queries, K)
            same_bits(ra, want)
            same_bits(rt, want)
            for x, y, z in zip(ca, ct, bctr):
                np.testing.assert_array_equal(x, z)
                np.testing.assert_array_equal(y, z)
            assert not np.isin(ra[0], dead[100:]).any()          # the 200 ids that no live row carries
            if queries is not Q:
                # a new row under a deleted id is live: where the clean graph finds it first, so does this one
                found = bpos[:, 0] == np.arange(n0, n0 + 100)
                assert found.any()
                np.testing.assert_array_equal(ra[0][found, 0], ids[n0:n0 + 100][found])
                assert (ra[1][found, 0] == 0).all()
    for i in (a, twin, clean):
        i.close()


def test_poisoned_workspaces_give_the_same_bits(tmp_path):
    assert "NMSLIB_GPU_POISON" not in os.environ, "this process must run without the poison fill"
    want = delete_poison_child.run_all()
    out = tmp_path / "poison.npz"
    env = dict(os.environ, NMSLIB_GPU_POISON="255")
    # (one attempt: a non-zero exit, a death by signal or the time limit fails the test)
    r = subprocess.run([sys.executable, delete_poison_child.__file__, str(out)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"child exit {r.returncode}\n{r.stdout[-4000:]}"
    with np.load(out) as z:
        got = {name: z[name] for name in z.files}
    assert sorted(got) == sorted(want)
    differ = [name for name in sorted(want) if not np.array_equal(got[name], want[name])]
    assert not differ, differ
