"""-m gpu: the batched GPU builder beyond its first corner -- lists of up to four words per lane (M, maxM <= 127,
maxM0 <= 254), selection heuristic 1 (delaunay_type=1) and the post-processing (post=1, 2) -- and
Index.graphBuilder(), which tells which builder made the graph.

Like tests/test_gpu_hnsw_build.py: the batched build is not the reference's insertion schedule, so here, on Gaussian
float rows at 8000 nodes, it is held to the structural invariants of Hnsw::add / addFriendlevel, to determinism and to
search quality on par with the host one-thread build (the reference's own graph, tests/test_golden_v4.py).  Where the
schedule IS the reference's (batches of one node, efConstruction >= n, no distance ties) the graphs must be equal.  The
exact check of the batched rule itself -- wide lists, heuristic 1 and both post modes with batches of many nodes, list
order included -- is tests/test_gpu_hnsw_build_exact.py.

One data set (iid Gaussian, D = 32: lists fill up to maxM0) and one build per configuration, shared by the tests."""
import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import refio
from tests.gpuutil import make_index
from tests.test_gpu_hnsw_build import check_invariants, graph_of

pytestmark = pytest.mark.gpu

# n: the smallest of 5000 / 8000 / 12000 at which the M = 64 graph has level-0 lists longer than 126 entries (the host
# build has 1 / 4 / 5 such lists; heuristic 2 prunes most full lists well below maxM0 = 128)
N, D, NQ, K, EFC = 8000, 32, 128, 10, 120
CONFIGS = {
    "m64": dict(M=64),
    "m100": dict(M=100),
    "d1": dict(M=16, delaunay_type=1),
    "p0": dict(M=16),
    "p1": dict(M=16, post=1),
    "p2": dict(M=16, post=2),
}


@pytest.fixture(scope="module")
def data():
    X, Q = refio.s_gauss(N, D, 71), refio.s_gauss(NQ, D, 72)
    bf = make_index("l2", "brute_force", X)
    ei, ed, _ = bf.knnQueryBatch(Q, 2 * K)
    bf.close()
    return X, Q, ei, ed


def recall_at_60(idx, data):
    _, Q, ei, ed = data
    idx.setQueryTimeParams(efSearch=60)
    ids, _, _ = idx.knnQueryBatch(Q, K)
    return refio.recall_nmslib(ids, ei, ed ** 2, K)      # (hnsw over l2 reports squared distances)


@pytest.fixture(scope="module")
def built(data, tmp_path_factory):
    """name -> {builder, graph, file bytes, recall@10 at efSearch=60} of the GPU build of CONFIGS[name], built once"""
    cache, tmp = {}, tmp_path_factory.mktemp("wide")

    def get(name):
        if name not in cache:
            idx = make_index("l2", "hnsw", data[0], efConstruction=EFC, gpu_build=1, **CONFIGS[name])
            path = tmp / f"{name}.idx"
            g = graph_of(idx, tmp, f"{name}.idx")
            cache[name] = dict(builder=idx.graphBuilder(), graph=g, raw=path.read_bytes(), path=str(path),
                               recall=recall_at_60(idx, data))
            idx.close()
        return cache[name]
    return get


def level0_sets(g):
    return [set(row[1:1 + row[0]].tolist()) for row in g["links0"]]


def upper_sets(g, maxM):
    return [set(blk[1:1 + blk[0]].tolist()) for blk in g["up_links"].reshape(-1, maxM + 1)]


# ---- 1: which builder ran ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m64", "m100", "d1", "p1", "p2"])
def test_gpu_builder_serves_wide_lists_heuristic1_and_post(built, name):
    assert built(name)["builder"] == 2


def test_builder_selection_rules(data, built):
    X = data[0][:600]
    cases = [
        (dict(M=64), 2),                                   # auto mode, default threads: the concurrent build -> GPU
        (dict(M=64, indexThreadQty=1), 1),                 # the reference's sequential order -> host
        (dict(M=64, gpu_build=0), 1),
        (dict(M=16, delaunay_type=3, gpu_build=1), 1),     # heuristic 3 stays on the host
        (dict(M=128, gpu_build=1), 1),                     # beyond four words per lane
        (dict(M=16, maxM=130, gpu_build=1), 1),
        (dict(M=100, maxM0=255, gpu_build=1), 1),
        (dict(M=127, gpu_build=1), 2),                     # the last size the GPU builder takes
    ]
    for params, want in cases:
        idx = make_index("l2", "hnsw", X, efConstruction=EFC, **params)
        assert idx.graphBuilder() == want, params
        ids, _, _ = idx.knnQueryBatch(X[:8], 1)
        assert ids[:, 0].tolist() == list(range(8)), params
        idx.close()
    loaded = nz.Index.load(built("m64")["path"], load_data=False)
    assert loaded.graphBuilder() == 0
    loaded.close()
    bf = make_index("l2", "brute_force", X)
    assert bf.graphBuilder() == 0
    bf.close()


# ---- 2: invariants of the wide graphs ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,M", [("m64", 64), ("m100", 100)])
def test_wide_list_invariants(built, name, M):
    g = built(name)["graph"]
    assert (g["maxM"], g["maxM0"]) == (M, 2 * M)
    check_invariants(g, M, M, 2 * M)      # no self links, no repeats, lengths, levels of neighbours, entry point, no empty list
    cnt = g["links0"][:, 0]
    print(name, "level-0 lists longer than 126:", int((cnt > 126).sum()), "longest:", int(cnt.max()))
    assert (cnt > 126).any()              # the four-words-per-lane form really carries data


# ---- 3: determinism ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m64", "p2"])
def test_two_builds_give_identical_files(data, built, name, tmp_path):
    idx = make_index("l2", "hnsw", data[0], efConstruction=EFC, gpu_build=1, **CONFIGS[name])
    p = tmp_path / "again.idx"
    idx.save(str(p), save_data=False)
    idx.close()
    assert p.read_bytes() == built(name)["raw"]


# ---- 4: quality against the reference's graph -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m64", "m100", "d1", "p1", "p2"])
def test_recall_on_par_with_host_one_thread_build(data, built, name):
    host = make_index("l2", "hnsw", data[0], efConstruction=EFC, gpu_build=0, indexThreadQty=1, **CONFIGS[name])
    assert host.graphBuilder() == 1
    rec_host = recall_at_60(host, data)
    host.close()
    rec_gpu = built(name)["recall"]
    print(name, "recall@10 efSearch=60: host one-thread", rec_host, "gpu", rec_gpu)
    assert rec_gpu >= rec_host - 0.02, (name, rec_host, rec_gpu)


# ---- 5: structure of the post-processed graphs ------------------------------------------------------------------
def test_post1_keeps_the_forward_graphs_lists(built):
    g1, gp = built("p0")["graph"], built("p1")["graph"]
    assert g1["maxM0"] == 32 and 1 <= gp["maxM0"] <= 64           # maxM0 becomes the longest union of two lists
    cnt = gp["links0"][:, 0]
    assert cnt.max() == gp["maxM0"]
    fwd, post = level0_sets(g1), level0_sets(gp)
    assert all(len(s) == c for s, c in zip(post, cnt))            # no repeats
    missing = [i for i in range(1, N) if not fwd[i] <= post[i]]   # (node 0 keeps the second graph's list, hnsw.cc:281)
    assert not missing, missing[:10]
    assert any(post[i] != fwd[i] for i in range(1, N))            # the second graph added something
    check_invariants(gp, 16, 16, gp["maxM0"])


def test_post2_ranks_the_union_again(built):
    g1, gp = built("p0")["graph"], built("p2")["graph"]
    assert gp["maxM0"] == 32
    check_invariants(gp, 16, 16, 32)
    fwd, post = level0_sets(g1), level0_sets(gp)
    changed = sum(a != b for a, b in zip(fwd, post))
    print("post=2: nodes whose level-0 list differs from the forward graph's:", changed, "of", N)
    assert changed > 0                                            # a post pass that does nothing would leave G1


# ---- 6: the selection itself, where the batched schedule is the sequential one ----------------------------------
def test_delaunay1_tiny_index_equals_host_lists():
    M = 16
    X = refio.s_gauss(M + 1, D, 91)
    lists = {}
    for mode in (0, 1):
        idx = make_index("l2", "hnsw", X, M=M, efConstruction=32, delaunay_type=1, gpu_build=mode,
                         **({"indexThreadQty": 1} if mode == 0 else {}))
        assert idx.graphBuilder() == 1 + mode
        lists[mode] = level0_sets(_graph(idx))
        idx.close()
    assert lists[0] == lists[1]


def _graph(idx):
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "g.idx")
        idx.save(p, save_data=False)
        return refio.parse_optimized_index(p)


@pytest.mark.parametrize("params", [dict(delaunay_type=1), dict(delaunay_type=1, post=2), dict(delaunay_type=2, post=2),
                                    dict(delaunay_type=0, post=2), dict(delaunay_type=2, post=1)],
                         ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()))
def test_one_node_batches_equal_the_host_graph(params):
    """gpu_build_div larger than n: every batch is one node, i.e. the reference's sequential insertion.  With
    efConstruction >= n every search returns all nodes of its level, and iid floats have no distance ties, so the GPU
    builder must select exactly the host builder's (= the reference's) neighbours: M = 4 over 60 rows makes the
    lists overflow, so heuristic 1 / 2, the shrink step and the post pass all decide something.  Lists as sets."""
    X = refio.s_gauss(60, 8, 92)
    graphs = {}
    for mode in (0, 1):
        idx = make_index("l2", "hnsw", X, M=4, efConstruction=64, gpu_build=mode, **params,
                         **({"indexThreadQty": 1} if mode == 0 else {"gpu_build_div": 1 << 20}))
        assert idx.graphBuilder() == 1 + mode
        graphs[mode] = _graph(idx)
        idx.close()
    h, g = graphs[0], graphs[1]
    assert (g["maxM0"], g["maxlevel"], g["enterpoint"]) == (h["maxM0"], h["maxlevel"], h["enterpoint"])
    np.testing.assert_array_equal(g["levels"], h["levels"])
    assert (h["links0"][:, 0] >= 8).any()                       # full lists: the shrink step ran
    assert level0_sets(g) == level0_sets(h)
    assert g["up_links"].size > 0 and upper_sets(g, 4) == upper_sets(h, 4)


# ---- 7: every search kernel walks a GPU-built wide graph --------------------------------------------------------
def test_search_kernels_agree_on_gpu_built_wide_graph(data, built, monkeypatch):
    _, Q, ei, ed = data
    idx = nz.Index.load(built("m64")["path"], load_data=False)
    got = {}
    for mw in ("0", "2"):
        monkeypatch.setenv("NMSLIB_HNSW_MW", mw)
        idx.setQueryTimeParams(efSearch=60)
        got[mw] = idx.knnQueryBatch(Q, K)
    monkeypatch.delenv("NMSLIB_HNSW_MW")
    idx.setQueryTimeParams(efSearch=60, algoType="old")
    got["old"] = idx.knnQueryBatch(Q, K)
    idx.close()
    np.testing.assert_array_equal(got["0"][0], got["2"][0])
    np.testing.assert_array_equal(got["0"][1], got["2"][1])
    np.testing.assert_array_equal(got["0"][0], got["old"][0])
    assert refio.recall_nmslib(got["old"][0], ei, ed ** 2, K) == pytest.approx(built("m64")["recall"])
