"""-m gpu: nmslib_gpu_consolidate on a resident HNSW graph.

The yardstick of the repair is exact: the graph is saved before the delete and after the consolidate, and a numpy
restatement of the rule of DESIGN.md 4.6c applied to the first file must give the second -- every list with its order.
The rows there have small integer entries, so every distance is exact in any summation order."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import refio
from tests.consolidate_ref import adj, assert_same_graph, parse_regular_index, reachability, restate
from tests.gpuutil import enqueue_knn, make_index, same_bits

from . import consolidate_poison_child

pytestmark = pytest.mark.gpu

K, NQ = 10, 70
HOST = dict(M=8, efConstruction=60, indexThreadQty=1)
GPU = dict(M=8, efConstruction=60, gpu_build=1)


def ext_ids(n):
    """external ids that are no positions"""
    return (5 * np.arange(n) + 7).astype(np.int32)


def int_rows(n, d, seed):
    return np.random.default_rng(seed).integers(-8, 9, (n, d)).astype(np.float32)


# ---- the graph of a saved index, both file formats ----
def graph_of(idx, tmp_path, name):
    path = str(tmp_path / name)
    idx.save(path, save_data=True)
    raw = open(path, "rb").read(4)
    g = refio.parse_optimized_index(path) if struct.unpack("<I", raw)[0] == 1 else parse_regular_index(path)
    g["path"] = path
    return g


def check_rule(space, X, build, dead_pos, tmp_path):
    """build, save, delete, consolidate, save; the restatement of the first file is the second
    -> the consolidated index, the parsed first file, the old positions of the live rows"""
    n = len(X)
    ids = ext_ids(n)
    idx = make_index(space, "hnsw", X, ids, **build)
    before = graph_of(idx, tmp_path, "before.idx")
    dead_pos = np.asarray(dead_pos)
    assert idx.deleteIds(ids[dead_pos]) == len(dead_pos)
    hbm = idx.stats()["hbm_bytes"]
    delaunay = build.get("delaunay_type", 2)
    want, want_repaired = restate(before, X, dead_pos, build["efConstruction"], delaunay)
    removed, repaired = idx.consolidate()
    assert removed == len(dead_pos) and repaired == want_repaired and repaired > 0
    assert idx.dataQty() == n - len(dead_pos) and idx.deletedRows() == 0
    assert idx.stats()["hbm_bytes"] < hbm
    after = graph_of(idx, tmp_path, "after.idx")
    assert_same_graph(after, want)
    live = np.setdiff1d(np.arange(n), dead_pos)
    for p in (0, len(live) // 2, len(live) - 1):
        np.testing.assert_array_equal(idx.getDataPoint(p), X[live[p]])
    check_answers(idx, space, X, ids, live)
    print(f"{space} {build}: {repaired} lists repaired; (empty lists, unreachable on level 0) before {reachability(before)} "
          f"after {reachability(after)}")
    dat = np.fromfile(after["path"] + ".dat", np.uint8)
    assert len(dat) == 8 + len(live) * (8 + 16 + (132 if space == "l2sqr_sift" else 4 * X.shape[1]))
    return idx, before, live


def check_answers(idx, space, X, ids, live):
    """every answer names a live row by its id, with the distance of that very row (u8: through the compacted norms)"""
    Q = X[live[:NQ]]
    idx.setQueryTimeParams(efSearch=200)
    rid, rd, cnt = idx.knnQueryBatch(Q, K)
    assert (cnt == K).all()
    pos_of = {int(i): p for p, i in enumerate(ids)}
    pos = np.vectorize(pos_of.__getitem__)(rid)
    assert np.isin(pos, live).all()
    d2 = ((X[pos].astype(np.int64) - Q[:, None, :].astype(np.int64)) ** 2).sum(2)
    np.testing.assert_array_equal(rd, d2.astype(np.float32))     # (l2 on the optimized index answers with squared distances)


def random_dead(n, share, seed):
    return np.sort(np.random.default_rng(seed).permutation(n)[:int(n * share)])


def largest_pool(g, dead_pos):
    """the most distinct live one-hop candidates any level-0 list has"""
    dead = np.zeros(g["n"], bool)
    dead[dead_pos] = True
    best = 0
    for u in np.nonzero(~dead)[0]:
        lst = adj(g, u, 0)
        if dead[lst].any():
            cand = set()
            for d in lst[dead[lst]]:
                cand |= {int(w) for w in adj(g, int(d), 0) if not dead[w]}
            best = max(best, len(cand - set(lst.tolist()) - {int(u)}))
    return best


RULE_CASES = {
    "host-built": ("l2", (3000, 16), HOST, 0.3),
    "gpu-built": ("l2", (3000, 16), GPU, 0.3),
    "l2sqr_sift": ("l2sqr_sift", (3000, 128), HOST, 0.3),
    "gpu-built-post-1": ("l2", (3000, 16), dict(GPU, post=1), 0.3),    # (maxM0 becomes the longest union)
    "gpu-built-post-2": ("l2", (3000, 16), dict(GPU, post=2), 0.3),
    "M40-half-deleted": ("l2", (2000, 8), dict(M=40, efConstruction=100, indexThreadQty=1), 0.5),
    "delaunay_type-0": ("l2", (3000, 16), dict(HOST, delaunay_type=0), 0.3),
    "delaunay_type-1": ("l2", (3000, 16), dict(HOST, delaunay_type=1), 0.3),
}


@pytest.mark.parametrize("case", list(RULE_CASES))
def test_the_rule_exactly(case, tmp_path):
    space, (n, d), build, share = RULE_CASES[case]
    X = refio.s_sift_like(n, 921) if space == "l2sqr_sift" else int_rows(n, d, 922)
    dead = random_dead(n, share, 923)
    idx, before, _ = check_rule(space, X, build, dead, tmp_path)
    assert idx.graphBuilder() == (2 if build.get("gpu_build") == 1 else 1)
    if case in ("host-built", "M40-half-deleted"):               # the cut to P candidates is exercised
        assert largest_pool(before, dead) > max(build["efConstruction"], 2 * build["M"])
    idx.close()


def test_the_rule_at_the_word_edges(tmp_path):
    n = 3000
    assert n % 32 != 0
    check_rule("l2", int_rows(n, 16, 924), HOST, np.array([0, 31, 32, 63, 64, n - 1]), tmp_path)[0].close()


def test_the_entry_point_and_the_whole_top_level_are_deleted(tmp_path):
    n = 3000
    X = int_rows(n, 16, 925)
    probe = make_index("l2", "hnsw", X, **HOST)
    g = graph_of(probe, tmp_path, "probe.idx")
    probe.close()
    top = np.nonzero(g["levels"] == g["maxlevel"])[0]
    assert g["enterpoint"] in top and g["maxlevel"] >= 2
    dead = np.union1d(top, random_dead(n, 0.1, 926))
    idx, before, live = check_rule("l2", X, HOST, dead, tmp_path)
    after = refio.parse_optimized_index(str(tmp_path / "after.idx"))
    assert after["maxlevel"] == before["levels"][live].max() < before["maxlevel"]
    idx.setQueryTimeParams(efSearch=40)
    assert (idx.knnQueryBatch(X[live[:NQ]], K)[2] == K).all()
    idx.close()


# ---- the device state ----
def run(idx, Q, k=K):
    res = idx.knnQueryBatch(Q, k)
    return res, tuple(x.copy() for x in idx.read_counters(len(Q)))


def assert_same_answers(a, b, Q, settings):
    for ef, params in settings:
        for i in (a, b):
            i.setQueryTimeParams(efSearch=ef, **params)
        (ra, ca), (rb, cb) = run(a, Q), run(b, Q)
        same_bits(ra, rb)
        for name, x, y in zip(("ndc", "hops", "hops_up"), ca, cb):
            np.testing.assert_array_equal(x, y, err_msg=f"efSearch={ef} {params} {name}")


SETTINGS = [(4, {}), (40, {}), (200, {}), (40, dict(algoType="old"))]


@pytest.mark.parametrize("space", ["l2", "cosinesimil"])
def test_the_resident_index_answers_as_the_index_loaded_from_its_file(space, tmp_path):
    """cosinesimil: the resident rows are normalised by a kernel, whose sums round differently from the file writer's on the
    host; the file of a consolidated graph therefore carries the rows the device holds"""
    n = 3000
    X, Q, ids = refio.s_lowrank(n, 16, 931), refio.s_lowrank(NQ, 16, 932), ext_ids(n)
    idx = make_index(space, "hnsw", X, ids, **HOST)
    # every query's nearest rows go
    idx.setQueryTimeParams(efSearch=200)
    near = np.unique(idx.knnQueryBatch(Q, K)[0])
    dead = np.union1d(near, ids[random_dead(n, 0.2, 933)]).astype(np.int32)
    marked = idx.deleteIds(dead)
    assert marked == len(dead)
    idx.setQueryTimeParams(efSearch=4)
    tomb = idx.knnQueryBatch(Q, K)
    assert (tomb[2] < K).any()                                   # the tombstone search runs out of live results
    assert idx.consolidate()[0] == marked
    resident = idx.stats()["hbm_bytes"]
    res = idx.knnQueryBatch(Q, K)
    assert (res[2] == K).all() and not np.isin(res[0], dead).any()
    assert idx.stats()["last_path"] == 4 and idx.stats()["hbm_bytes"] == resident   # (no bitset came back)
    path = str(tmp_path / "c.idx")
    idx.save(path, save_data=True)
    loaded = nz.Index.load(path)
    assert loaded.dataQty() == n - marked
    assert_same_answers(idx, loaded, Q, SETTINGS)
    loaded.close()
    idx.close()


def test_the_fp16_copy_is_compacted(tmp_path):
    n = 3000
    X, Q, ids = refio.s_lowrank(n, 16, 934), refio.s_lowrank(NQ, 16, 935), ext_ids(n)
    biggest = int(np.argmax(np.abs(X).max(1)))
    dead = np.setdiff1d(random_dead(n, 0.3, 936), [biggest])     # the row that fixes the copy's scale stays
    idx = make_index("l2", "hnsw", X, ids, gpu_rows="f16", **HOST)
    assert idx.deleteIds(ids[dead]) == len(dead)
    r16 = idx.stats()["hbm_bytes"]
    assert idx.consolidate()[0] == len(dead)
    assert idx.stats()["hbm_bytes"] < r16
    path = str(tmp_path / "c.idx")
    idx.save(path, save_data=True)
    loaded = nz.Index.load(path)
    for ef in (4, 40, 200):
        idx.setQueryTimeParams(efSearch=ef)
        loaded.setQueryTimeParams(efSearch=ef, gpu_rows="f16")
        same_bits(idx.knnQueryBatch(Q, K), loaded.knnQueryBatch(Q, K))
        assert idx.stats()["last_path"] == 5 and loaded.stats()["last_path"] == 5
    loaded.close()
    idx.close()


def test_two_equal_indexes_give_equal_files_and_poison_changes_nothing(tmp_path):
    assert "NMSLIB_GPU_POISON" not in os.environ, "this process must run without the poison fill"
    want = consolidate_poison_child.run_all()
    again = consolidate_poison_child.run_all()
    assert sorted(want) == sorted(again)
    assert not [name for name in sorted(want) if not np.array_equal(want[name], again[name])]
    out = tmp_path / "poison.npz"
    env = dict(os.environ, NMSLIB_GPU_POISON="255")
    # (one attempt: a non-zero exit, a death by signal or the time limit fails the test)
    r = subprocess.run([sys.executable, consolidate_poison_child.__file__, str(out)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"child exit {r.returncode}\n{r.stdout[-4000:]}"
    with np.load(out) as z:
        got = {name: z[name] for name in z.files}
    assert sorted(got) == sorted(want)
    differ = [name for name in sorted(want) if not np.array_equal(got[name], want[name])]
    assert not differ, differ


# ---- lifecycle ----
def test_delete_consolidate_delete_consolidate(tmp_path):
    n = 3000
    X, ids = int_rows(n, 16, 941), ext_ids(n)
    idx = make_index("l2", "hnsw", X, ids, **HOST)
    g0 = graph_of(idx, tmp_path, "g0.idx")
    first = random_dead(n, 0.2, 942)
    assert idx.deleteIds(ids[first]) == len(first)
    g1, r1 = restate(g0, X, first, 60, 2)
    assert idx.consolidate() == (len(first), r1)
    live1 = np.setdiff1d(np.arange(n), first)
    second = random_dead(len(live1), 0.2, 943)                   # positions of the consolidated index
    assert idx.deleteIds(ids[live1[second]]) == len(second)
    g2, r2 = restate(g1, X[live1], second, 60, 2)
    assert idx.consolidate() == (len(second), r2)
    assert idx.consolidate() == (0, 0)
    assert_same_graph(graph_of(idx, tmp_path, "g2.idx"), g2)
    idx.close()


def test_rows_added_after_a_consolidate_are_appended():
    n0, n1, d = 2000, 2500, 16
    X, Q, ids = refio.s_lowrank(n1, d, 944), refio.s_lowrank(NQ, d, 945), ext_ids(n1)
    dead = random_dead(n0, 0.3, 946)
    idx = make_index("l2", "hnsw", X[:n0], ids[:n0], gpu_append=1, gpu_build_batch=256, **GPU)
    assert idx.deleteIds(ids[dead]) == len(dead)
    idx.setQueryTimeParams(efSearch=64)
    idx.knnQueryBatch(Q, K)
    hbm = idx.stats()["hbm_bytes"]
    assert idx.consolidate()[0] == len(dead)
    idx.addDenseBatch(X[n0:], ids[n0:])
    idx.finalize()
    st = idx.stats()
    assert st["rows_appended"] == n1 - n0 and st["rows"] == n1 - len(dead) and idx.graphBuilder() == 2, st
    assert st["hbm_bytes"] < hbm
    res = idx.knnQueryBatch(np.r_[Q, X[n0:n0 + 30]], K)
    assert (res[2] == K).all() and not np.isin(res[0], ids[dead]).any()
    np.testing.assert_array_equal(res[0][NQ:, 0], ids[n0:n0 + 30])   # a new row finds itself
    live = np.setdiff1d(np.arange(n1), dead)
    exact = make_index("l2", "seq_search", X[live], ids[live])
    truth = exact.knnQueryBatch(Q, K + 22)
    assert refio.recall_nmslib(res[0][:NQ], truth[0], truth[1], K) >= 0.95
    exact.close()
    idx.close()


def test_a_batch_in_flight_on_a_foreign_stream_sees_the_old_index():
    """batch, delete, consolidate with no host synchronisation in between: the batch's buffers hold the answer of the index
    as it was.  The stream is kept busy while the calls are made (100 passes over a 256 MB tensor take no less than 6.4 ms
    at the 8 TB/s of HBM3E, a batch of this shape under 1 ms), so the batch has not started when the consolidate is called."""
    import torch
    n = 3000
    X, Q, ids = refio.s_lowrank(n, 16, 951), refio.s_lowrank(NQ, 16, 952), ext_ids(n)
    idx = make_index("l2", "hnsw", X, ids, **HOST)
    idx.setQueryTimeParams(efSearch=40)
    unfiltered = idx.knnQueryBatch(Q, K)
    dead = np.unique(unfiltered[0][:, :3])
    a = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()

    def busy(qbuf):
        for _ in range(100):
            a.add_(1.0)

    first = enqueue_knn(idx, Q, K, stream, before=busy)
    assert idx.deleteIds(dead) == len(dead)
    assert idx.consolidate()[0] == len(dead)
    second = enqueue_knn(idx, Q, K, stream)
    stream.synchronize()
    same_bits(first.result(), unfiltered)
    got = second.result()
    assert (got[2] == K).all() and not np.isin(got[0], dead).any()
    idx.close()


def test_brute_force_results_do_not_change():
    n = 3000
    X, Q, ids = refio.s_lowrank(n, 16, 953), refio.s_lowrank(NQ, 16, 954), ext_ids(n)
    idx = make_index("l2", "brute_force", X, ids)
    dead = random_dead(n, 0.3, 955)
    assert idx.deleteIds(ids[dead]) == len(dead)
    before = idx.knnQueryBatch(Q, K)
    assert idx.consolidate() == (len(dead), 0)
    assert idx.dataQty() == n - len(dead)
    same_bits(idx.knnQueryBatch(Q, K), before)
    idx.close()


# ---- quality ----
# the spread (max - min) of the recall at efSearch = 128 of three fresh builds over the live rows in three row orders, as
# measured on an MI355X (1.0000 / 0.9998 / 1.0000; the test measures it again and uses what it measures):
# S_MEASURED = 0.0002        (m = 0.00042 with r = 0.9999; all legs: DESIGN.md 4.6c)


def test_recall_against_the_tombstone_search_and_a_fresh_build(tmp_path):
    n, d, nq, share = 20000, 32, 1000, 0.3
    build = dict(M=16, efConstruction=100, gpu_build=1)
    X, Q, ids = refio.s_lowrank(n, d, 961), refio.s_lowrank(nq, d, 962), np.arange(n, dtype=np.int32)
    dead = random_dead(n, share, 963)
    live = np.setdiff1d(np.arange(n), dead)
    exact = make_index("l2", "seq_search", X[live], ids[live])
    truth = exact.knnQueryBatch(Q, K + 22)
    exact.close()

    def recall(idx, ef):
        idx.setQueryTimeParams(efSearch=ef)
        return refio.recall_nmslib(idx.knnQueryBatch(Q, K)[0], truth[0], truth[1], K)

    idx = make_index("l2", "hnsw", X, ids, **build)
    assert idx.deleteIds(ids[dead]) == len(dead)
    a = {ef: recall(idx, ef) for ef in (10, 128)}                # the tombstone search
    assert idx.consolidate()[0] == len(dead)
    b = {ef: recall(idx, ef) for ef in (10, 128)}                # the consolidated graph
    print(f"consolidated graph: (empty lists, unreachable on level 0) {reachability(graph_of(idx, tmp_path, 'b.idx'))}")
    idx.close()
    c = []
    for seed in (964, 965, 966):                                 # fresh builds over the live rows, three row orders
        order = np.random.default_rng(seed).permutation(len(live))
        fresh = make_index("l2", "hnsw", X[live][order], ids[live][order], **build)
        print(f"fresh graph: (empty lists, unreachable on level 0) {reachability(graph_of(fresh, tmp_path, 'c.idx'))}")
        c.append({ef: recall(fresh, ef) for ef in (10, 128)})
        fresh.close()
    s = max(x[128] for x in c) - min(x[128] for x in c)
    r = a[128]
    m = max(2 * s, 3 * np.sqrt(2 * r * (1 - r) / (nq * K)))
    print(f"tombstone {a}  consolidated {b}  fresh {c}  s = {s:.5f}  m = {m:.5f}")
    assert b[10] >= a[10], (a, b)
    assert b[128] >= a[128] - m, (a, b, s, m)
