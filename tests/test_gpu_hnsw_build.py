"""-m gpu: batched HNSW construction on the GPU (index parameter gpu_build=1).

The batched build is not the reference's insertion schedule (a batch is searched against the graph
before the batch), so the reference's graph is no yardstick for it.  Its own rule is: the exact check is
tests/test_gpu_hnsw_build_exact.py, which compares the built graph list for list with a sequential
restatement of the batched rule on inputs whose f32 arithmetic is exact.  This file holds what that
check does not reach -- production-like float data, large graphs, angulardist -- to the structural
invariants of Hnsw::add / addFriendlevel, to determinism and to search quality: recall of the GPU-built
graph must be on par with the reference-order host build (which test_cabi_cpu.py proves equal to the
reference's graph) at the same parameters."""
import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import refio
from tests.gpuutil import make_index

pytestmark = pytest.mark.gpu


def graph_of(idx, tmp_path, name):
    p = str(tmp_path / name)
    idx.save(p, save_data=False)
    return refio.parse_optimized_index(p)


def check_invariants(g, M, maxM, maxM0):
    n = g["n"]
    l0 = g["links0"]
    cnt = l0[:, 0]
    assert cnt.max() <= maxM0 and cnt.min() >= (1 if n > 1 else 0)
    cols = np.arange(1, maxM0 + 1)[None, :]
    valid = cols <= cnt[:, None]
    nb = l0[:, 1:]
    assert nb[valid].min() >= 0 and nb[valid].max() < n
    assert not (valid & (nb == np.arange(n)[:, None])).any()              # no self links
    srt = np.sort(np.where(valid, nb, -1 - cols), axis=1)                  # distinct fillers
    assert not (np.diff(srt, axis=1) == 0).any()                           # no duplicates
    # upper levels
    levels, up_off, up = g["levels"], g["up_off"], g["up_links"]
    assert g["maxlevel"] == levels.max() and levels[g["enterpoint"]] == g["maxlevel"]
    for i in np.nonzero(levels > 0)[0]:
        blk = up[up_off[i]:up_off[i] + levels[i] * (maxM + 1)].reshape(levels[i], maxM + 1)
        for l in range(levels[i]):
            c = blk[l, 0]
            assert 0 <= c <= maxM
            ids = blk[l, 1:1 + c]
            assert len(set(ids.tolist())) == c and i not in ids
            assert (levels[ids] >= l + 1).all()                            # neighbours live on that level


@pytest.mark.parametrize("space", ["l2", "cosinesimil", "l2sqr_sift"])
def test_gpu_build_invariants_and_recall_small(space, tmp_path):
    n, nq, k = 20000, 500, 10
    if space == "l2sqr_sift":
        X, Q = refio.s_sift_like(n, 61), refio.s_sift_like(nq, 62)
    else:
        X, Q = refio.s_lowrank(n, 64, 61), refio.s_lowrank(nq, 64, 62)
    bf = make_index(space, "brute_force", X)
    ei, ed, _ = bf.knnQueryBatch(Q, 2 * k)
    bf.close()
    rec = {}
    for mode in (0, 1):
        # (the host side single-threaded: deterministic, and the reference's own graph)
        idx = make_index(space, "hnsw", X, M=16, efConstruction=100, gpu_build=mode,
                         **({"indexThreadQty": 1} if mode == 0 else {}))
        if mode == 1:
            if space != "l2sqr_sift":      # (u8 indices are saved in the reference's non-optimized format)
                g = graph_of(idx, tmp_path, f"g_{space}.idx")
                check_invariants(g, 16, 16, 32)
            assert idx.stats()["build_seconds"] > 0
        idx.setQueryTimeParams(efSearch=64)
        ids, ds, _ = idx.knnQueryBatch(Q, k)
        rec[mode] = refio.recall_nmslib(ids, ei, ed, k, integer=(space == "l2sqr_sift"))
        idx.close()
    print("recall host/gpu build:", rec)
    assert rec[1] >= rec[0] - 0.01, rec
    assert space == "l2sqr_sift" or rec[1] >= 0.95, rec     # (uniform-ish u8 data is hard at ef=64 for both)


def test_gpu_build_is_deterministic_and_reloadable(tmp_path):
    X, Q = refio.s_lowrank(6000, 32, 71), refio.s_lowrank(64, 32, 72)
    a = make_index("l2", "hnsw", X, M=8, efConstruction=60, gpu_build=1, gpu_build_batch=256)
    b = make_index("l2", "hnsw", X, M=8, efConstruction=60, gpu_build=1, gpu_build_batch=256)
    ga, gb = graph_of(a, tmp_path, "a.idx"), graph_of(b, tmp_path, "b.idx")
    np.testing.assert_array_equal(ga["links0"], gb["links0"])
    np.testing.assert_array_equal(ga["up_links"], gb["up_links"])
    check_invariants(ga, 8, 8, 16)
    ids, ds, _ = a.knnQueryBatch(Q, 10)
    c = nz.Index.load(str(tmp_path / "a.idx"), load_data=False)
    ids2, ds2, _ = c.knnQueryBatch(Q, 10)
    np.testing.assert_array_equal(ids, ids2)
    np.testing.assert_array_equal(ds, ds2)
    for i in (a, b, c):
        i.close()


@pytest.mark.parametrize("space,dim", [("l2", 32), ("cosinesimil", 48)])
def test_gpu_build_same_graph_with_either_search_kernel(space, dim, tmp_path, monkeypatch):
    """the construction's search step runs the workgroup-per-query kernel (stored rows as queries, any level); the
    one-wave kernel (NMSLIB_HNSW_MW=0) must produce the same candidates, hence the same graph, bit for bit"""
    X = refio.s_lowrank(8000, dim, 171)
    graphs = []
    for mw in ("0", "1"):
        monkeypatch.setenv("NMSLIB_HNSW_MW", mw)
        idx = make_index(space, "hnsw", X, M=8, efConstruction=80, gpu_build=1, gpu_build_batch=512)
        graphs.append(graph_of(idx, tmp_path, f"mw{mw}.idx"))
        idx.close()
    assert graphs[0]["up_links"].size > 0      # (several levels: the search step ran above level 0 too)
    np.testing.assert_array_equal(graphs[0]["links0"], graphs[1]["links0"])
    np.testing.assert_array_equal(graphs[0]["up_links"], graphs[1]["up_links"])


def test_gpu_build_tiny_and_delaunay0():
    X = refio.s_gauss(40, 8, 81)
    idx = make_index("l2", "hnsw", X, M=4, efConstruction=20, gpu_build=1)
    idx.setQueryTimeParams(efSearch=40)
    ids, ds, cnt = idx.knnQueryBatch(X, 1)
    assert (ids[:, 0] == np.arange(40)).all() and (cnt == 1).all()
    idx.close()
    one = make_index("l2", "hnsw", X[:1], M=4, efConstruction=20, gpu_build=1)
    ids, ds, cnt = one.knnQueryBatch(X[:3], 5)
    assert (cnt == 1).all() and (ids[:, 0] == 0).all()
    one.close()
    X, Q = refio.s_lowrank(5000, 32, 82), refio.s_lowrank(100, 32, 83)
    bf = make_index("l2", "brute_force", X)
    ei, ed, _ = bf.knnQueryBatch(Q, 20)
    bf.close()
    idx = make_index("l2", "hnsw", X, M=12, efConstruction=80, delaunay_type=0, gpu_build=1)
    idx.setQueryTimeParams(efSearch=80)
    ids, _, _ = idx.knnQueryBatch(Q, 10)
    assert refio.recall_nmslib(ids, ei, ed, 10) >= 0.9
    idx.close()


@pytest.mark.parametrize("space", ["l1", "linf", "angulardist", "negdotprod"])
def test_gpu_build_other_spaces_recall_on_par_with_host_build(space):
    n, nq, k = 8000, 200, 10
    X, Q = refio.s_lowrank(n, 48, 93), refio.s_lowrank(nq, 48, 94)
    bf = make_index(space, "brute_force", X)
    ei, ed, _ = bf.knnQueryBatch(Q, 2 * k)
    bf.close()
    rec = {}
    for mode in (0, 1):
        idx = make_index(space, "hnsw", X, M=12, efConstruction=80, gpu_build=mode,
                         **({"indexThreadQty": 1} if mode == 0 else {}))
        idx.setQueryTimeParams(efSearch=60)
        ids, _, _ = idx.knnQueryBatch(Q, k)
        rec[mode] = refio.recall_nmslib(ids, ei, ed, k)
        idx.close()
    assert rec[1] >= rec[0] - 0.02, rec


def test_gpu_build_edge_cases_duplicates_large_ef_large_m():
    # duplicate rows (zero distances, ties everywhere), efConstruction above the LDS-table range, M near the cap
    rng = np.random.default_rng(5)
    base = rng.standard_normal((300, 16)).astype(np.float32)
    X = np.concatenate([base, base[:200], base[:100]])                 # 600 rows, many exact duplicates
    idx = make_index("l2", "hnsw", X, M=30, efConstruction=400, gpu_build=1)        # maxM0 = 60 (limit 62)
    idx.setQueryTimeParams(efSearch=100)
    ids, ds, cnt = idx.knnQueryBatch(base[:50], 3)
    assert (cnt == 3).all() and np.allclose(ds[:, 0], 0.0)
    for q in range(50):                                                # the three copies of row q come first
        assert set(ids[q].tolist()) <= {q, q + 300, q + 500} if q < 100 else True
    idx.close()
    for n in (2, 3, 17):                                               # tiny graphs
        idx = make_index("cosinesimil", "hnsw", base[:n], M=4, efConstruction=10, gpu_build=1)
        ids, ds, cnt = idx.knnQueryBatch(base[:n], min(n, 2))
        assert (ids[:, 0] == np.arange(n)).all()
        idx.close()
    with pytest.raises(nz.NmslibError):
        make_index("l2", "hnsw", base, M=8, efConstruction=2000, gpu_build=1)


def test_gpu_build_hub_targets_many_requests_deterministic(tmp_path):
    """more than 32 reverse-link requests on one target in one batch, and rows whose insertion order has
    locality.  300 near-identical rows arrive together (one batch holds 250 of them): without batch-mate visibility
    they would all link to their common old neighbour only and most of them would be unreachable.  The requests are
    sorted by (target, new node) on the device and all applied, earlier batch-mates are candidates like in sequential
    insertion: two builds are identical, and recall / self-reachability inside the cluster are on par with the
    reference-order host build (measured: GPU 0.966 / 0.95, host 0.917 / 0.84 at efSearch=100; without batch-mates the
    GPU build gave 0.64)."""
    rng = np.random.default_rng(9)
    base = rng.standard_normal((4000, 24)).astype(np.float32)
    cluster = (base[7][None, :] + 1e-3 * rng.standard_normal((300, 24))).astype(np.float32)   # 300 rows around row 7
    X = np.concatenate([base, cluster])
    Qc = cluster[:128]
    bf = make_index("l2", "brute_force", X)
    ei, ed, _ = bf.knnQueryBatch(Qc, 32)
    bf.close()
    graphs, rec, selfhit = [], {}, {}
    for name, kw in (("gpu0", dict(gpu_build=1)), ("gpu1", dict(gpu_build=1)), ("host", dict(gpu_build=0, indexThreadQty=1))):
        idx = make_index("l2", "hnsw", X, M=8, efConstruction=100, **kw)
        if name != "host":
            graphs.append(graph_of(idx, tmp_path, f"{name}.idx"))
        idx.setQueryTimeParams(efSearch=100)
        ids, ds, cnt = idx.knnQueryBatch(Qc, 10)
        rec[name] = refio.recall_nmslib(ids, ei, ed ** 2, 10)
        selfhit[name] = float((ids[:, 0] == 4000 + np.arange(128)).mean())
        idx.close()
    np.testing.assert_array_equal(graphs[0]["links0"], graphs[1]["links0"])
    np.testing.assert_array_equal(graphs[0]["up_links"], graphs[1]["up_links"])
    check_invariants(graphs[0], 8, 8, 16)
    assert rec["gpu0"] >= rec["host"] - 0.02 and rec["gpu0"] >= 0.9, rec
    assert selfhit["gpu0"] >= selfhit["host"] - 0.05, selfhit


def test_c5_graph_quality_1m_768_cosine_vs_reference_graph():
    """C5 (HNSW cosinesimil, 768-D): 1M x 768 S-768 rows (rank-64 latent: a hard set -- the REFERENCE's own graph reaches
    recall@10 = 0.44 at efSearch=128, tests/golden/c5_ref_1m768.json, produced by tools/c5_recall.py from the real
    reference).  The GPU-built graph must match that graph's recall at equal efSearch on the same 512 queries."""
    import json
    import os
    from tools.c5_recall import s_768
    ref = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "c5_ref_1m768.json")))
    n, dim, nq, k = ref["n"], ref["dim"], ref["nq"], ref["k"]
    X, Q = s_768(n, dim, 46, ref["rank"], ref["noise"]), s_768(nq, dim, 47, ref["rank"], ref["noise"])
    bf = make_index("cosinesimil", "seq_search", X)
    gi, gd, _ = bf.knnQueryBatch(Q, k + 22)
    bf.close()
    idx = make_index("cosinesimil", "hnsw", X, M=ref["M"], efConstruction=ref["efC"], gpu_build=1)
    got = {}
    for ef in (128, 512, 1000):
        idx.setQueryTimeParams(efSearch=ef)
        ids, _, _ = idx.knnQueryBatch(Q, k)
        got[ef] = refio.recall_nmslib(ids, gi, gd, k)
    idx.close()
    for ef, r in got.items():
        assert r >= ref["recall"][str(ef)] - 0.001, (got, ref["recall"])
