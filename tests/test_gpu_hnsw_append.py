"""-m gpu: rows added after a GPU build go into the resident graph (index parameter gpu_append=1).

The yardstick is exact.  With the same parameters

    build(X[:n0]) -> add X[n0:] -> finalize     ==     build(X, gpu_build_cut=n0)

bit for bit: both run the same batches over the same graph states (gpu_build_cut only forces a batch boundary at n0).  So
the appended index is compared with the cut build in its saved graph, its search results and its work counters; where
no graph can be compared (l2sqr_sift, chained appends) recall is held to a fresh full build's."""
import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import refio
from tests.gpuutil import make_index

pytestmark = pytest.mark.gpu

K = 10
BUILD = dict(M=8, efConstruction=60, gpu_build=1, gpu_build_batch=256)
N0, N1, D = 3000, 4000, 32
GRAPH_KEYS = ("links0", "up_links", "levels", "maxlevel", "enterpoint")


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


def assert_same_graph(a, b):
    assert a["n"] == b["n"]
    for key in GRAPH_KEYS:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def add_rows(idx, X, lo, hi, ext=None):
    """rows [lo, hi) of X under the ids a build of all of X gives them"""
    ids = np.arange(lo, hi, dtype=np.int32) if ext is None else ext[lo:hi]
    if X.dtype == np.uint8:
        idx.addUInt8Batch(X[lo:hi], ids)
    else:
        idx.addDenseBatch(X[lo:hi], ids)


def appended(space, X, cuts, ext=None, **params):
    """build X[:cuts[0]], then one add + finalize per further cut; -> index, the stats after every finalize"""
    idx = make_index(space, "hnsw", X[:cuts[0]], None if ext is None else ext[:cuts[0]], gpu_append=1, **params)
    stats = [idx.stats()]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        add_rows(idx, X, lo, hi, ext)
        idx.finalize()
        stats.append(idx.stats())
    return idx, stats


def search(idx, Q, efs=(20, 64), k=K):
    """ids, distances and the work counters of Q at every efSearch"""
    out = {}
    for ef in efs:
        idx.setQueryTimeParams(efSearch=ef)
        ids, ds, cnt = idx.knnQueryBatch(Q, k)
        ndc, hops, hops_up = idx.read_counters(len(Q)) or (None, None, None)    # (row shards: no counters on the handle)
        out[ef] = dict(ids=ids, ds=ds, cnt=cnt, ndc=ndc, hops=hops, hops_up=hops_up)
    return out


def assert_same_search(a, b, counters=True):
    assert a.keys() == b.keys()
    for ef in a:
        for key in ("ids", "ds", "cnt") + (("ndc", "hops", "hops_up") if counters else ()):
            np.testing.assert_array_equal(a[ef][key], b[ef][key], err_msg=f"efSearch={ef} {key}")


def recall(idx, Q, truth, ef=64, integer=False):
    idx.setQueryTimeParams(efSearch=ef)
    ids, _, _ = idx.knnQueryBatch(Q, K)
    return refio.recall_nmslib(ids, truth[0], truth[1], K, integer=integer)


@pytest.fixture(scope="module")
def data():
    return {"l2": refio.s_lowrank(N1, D, 301), "cosinesimil": refio.s_lowrank(N1, D, 302), "Q": refio.s_lowrank(64, D, 303)}


@pytest.fixture(scope="module")
def cut_l2(data, tmp_path_factory):
    """the l2 cut build several tests compare with: its graph and its answers (never modified)"""
    c = make_index("l2", "hnsw", data["l2"], gpu_build_cut=N0, **BUILD)
    ref = dict(graph=graph_of(c, tmp_path_factory.mktemp("cut"), "cut.idx"), search=search(c, data["Q"]),
               hbm=c.stats()["hbm_bytes"])
    c.close()
    return ref


@pytest.mark.parametrize("space", ["l2", "cosinesimil"])
def test_append_equals_the_cut_build(space, data, cut_l2, tmp_path):
    X, Q = data[space], data["Q"]
    a, st = appended(space, X, (N0, N1), **BUILD)
    assert st[0]["rows_appended"] == 0 and st[0]["rows_uploaded"] == N0, st[0]
    assert st[1]["rows_appended"] == N1 - N0 == st[1]["rows_uploaded"], st[1]
    assert st[1]["rows"] == N1 and a.dataQty() == N1 and a.graphBuilder() == 2
    if space == "l2":
        want_graph, want_search, want_hbm = cut_l2["graph"], cut_l2["search"], cut_l2["hbm"]
    else:   # (cosine: rows normalised in place -- normalising the old ones a second time would change distances' bits)
        c = make_index(space, "hnsw", X, gpu_build_cut=N0, **BUILD)
        want_graph, want_search, want_hbm = graph_of(c, tmp_path, "cut.idx"), search(c, Q), c.stats()["hbm_bytes"]
        c.close()
    assert want_graph["up_links"].size > 0                    # several levels
    assert_same_search(search(a, Q), want_search)
    assert st[1]["hbm_bytes"] == want_hbm                       # exact-fit growth: what a build of N1 rows allocates
    assert_same_graph(graph_of(a, tmp_path, "app.idx"), want_graph)
    a.close()


def test_tiny_starts(tmp_path):
    X = refio.s_gauss(40, 8, 81)
    P = dict(M=4, efConstruction=20, gpu_build=1)
    a, st = appended("l2", X, (1, 2, 40), **P)
    assert [s["rows_appended"] for s in st] == [0, 1, 38]
    assert a.dataQty() == 40
    a.setQueryTimeParams(efSearch=40)
    ids, _, cnt = a.knnQueryBatch(X, 1)
    assert (ids[:, 0] == np.arange(40)).all() and (cnt == 1).all()
    a.close()
    b, st = appended("l2", X, (1, 40), **P)
    assert st[1]["rows_appended"] == 39
    c = make_index("l2", "hnsw", X, gpu_build_cut=1, **P)
    assert_same_graph(graph_of(b, tmp_path, "b.idx"), graph_of(c, tmp_path, "c.idx"))
    b.close()
    c.close()


def test_top_level_promotion_inside_the_append(tmp_path):
    n0, n1 = 50, 4000
    X = refio.s_lowrank(n1, 16, 311)
    P = dict(M=4, efConstruction=40, gpu_build=1)
    a, st = appended("l2", X, (n0, n1), **P)
    assert st[1]["rows_appended"] == n1 - n0
    c = make_index("l2", "hnsw", X, gpu_build_cut=n0, **P)
    ga, gc = graph_of(a, tmp_path, "a.idx"), graph_of(c, tmp_path, "c.idx")
    # the precondition: levels are the stream's, not the data's -- an appended node raises the top level
    assert gc["levels"][n0:].max() > gc["levels"][:n0].max()
    check_invariants(ga, 4, 4, 8)
    assert ga["enterpoint"] >= n0
    assert_same_graph(ga, gc)
    a.close()
    c.close()


def test_l2sqr_sift_append():
    n0, n1 = 4500, 6000
    U, UQ = refio.s_sift_like(n1, 321), refio.s_sift_like(64, 322)
    a, st = appended("l2sqr_sift", U, (n0, n1), **BUILD)
    assert st[1]["rows_appended"] == n1 - n0 == st[1]["rows_uploaded"] and a.graphBuilder() == 2
    c = make_index("l2sqr_sift", "hnsw", U, gpu_build_cut=n0, **BUILD)
    assert_same_search(search(a, UQ), search(c, UQ))
    assert st[1]["hbm_bytes"] == c.stats()["hbm_bytes"]
    bf = make_index("l2sqr_sift", "brute_force", U)
    ei, ed, _ = bf.knnQueryBatch(UQ, 2 * K)
    bf.close()
    fresh = make_index("l2sqr_sift", "hnsw", U, **BUILD)
    rec = dict(append=recall(a, UQ, (ei, ed), integer=True), fresh=recall(fresh, UQ, (ei, ed), integer=True))
    print("recall@10 efSearch=64:", rec)
    assert rec["append"] >= rec["fresh"] - 0.01, rec
    for i in (a, c, fresh):
        i.close()


def test_chained_appends_are_deterministic_and_keep_recall(tmp_path):
    cuts = (2000, 2500, 4000, 4007)
    X, Q = refio.s_lowrank(cuts[-1], D, 331), refio.s_lowrank(64, D, 332)
    ext = (7 * np.arange(cuts[-1]) + 3).astype(np.int32)
    a, sa = appended("l2", X, cuts, ext, **BUILD)
    b, sb = appended("l2", X, cuts, ext, **BUILD)
    assert [s["rows_appended"] for s in sa] == [0, 500, 1500, 7] == [s["rows_appended"] for s in sb]
    ga, gb = graph_of(a, tmp_path, "a.idx"), graph_of(b, tmp_path, "b.idx")
    assert_same_graph(ga, gb)
    assert ga["n"] == cuts[-1]
    check_invariants(ga, 8, 8, 16)
    bf = make_index("l2", "brute_force", X, ext)
    ei, ed, _ = bf.knnQueryBatch(Q, 2 * K)
    bf.close()
    fresh = make_index("l2", "hnsw", X, ext, **BUILD)
    rec = dict(append=recall(a, Q, (ei, ed)), fresh=recall(fresh, Q, (ei, ed)))
    print("recall@10 efSearch=64:", rec)
    assert rec["append"] >= rec["fresh"] - 0.01, rec
    ids, _, _ = a.knnQueryBatch(Q, K)
    assert ((ids - 3) % 7 == 0).all() and ids.max() > cuts[0] * 7        # external ids, appended rows among them
    self_ids, _, _ = a.knnQueryBatch(X[cuts[-1] - 7:], 1)
    np.testing.assert_array_equal(self_ids[:, 0], ext[cuts[-1] - 7:])     # the last seven rows are found under their ids
    for i in (a, b, fresh):
        i.close()


@pytest.mark.parametrize("boost", [1.0, 8.0], ids=["same-scale", "new-rows-move-the-scale"])
def test_append_with_the_fp16_copy(boost, data):
    """gpu_rows=f16: the copy grows with the rows.  boost = 8: the appended rows hold the largest element, so the copy's one
    power-of-two scale changes and the old rows are packed again (on the device) -- as a build of all rows packs them."""
    X, Q = data["l2"].copy(), data["Q"]
    X[N0:] *= np.float32(boost)
    a, st = appended("l2", X, (N0, N1), gpu_rows="f16", **BUILD)
    assert st[1]["rows_appended"] == N1 - N0 == st[1]["rows_uploaded"]
    got = search(a, Q)
    assert a.stats()["last_path"] == 5
    c = make_index("l2", "hnsw", X, gpu_build_cut=N0, gpu_rows="f16", **BUILD)
    assert_same_search(got, search(c, Q))
    assert c.stats()["last_path"] == 5
    grew = st[1]["hbm_bytes"] - st[0]["hbm_bytes"]
    assert grew >= (N1 - N0) * (D * 4 + D * 2), (grew, st)        # the new rows' share of the f32 rows and of the copy
    assert st[1]["hbm_bytes"] == c.stats()["hbm_bytes"]
    a.close()
    c.close()


def test_save_and_load_after_an_append(data, cut_l2, tmp_path):
    X, Q = data["l2"], data["Q"]
    a, _ = appended("l2", X, (N0, N1), **BUILD)
    path = str(tmp_path / "app.idx")
    a.save(path, save_data=False)
    g = refio.parse_optimized_index(path)
    assert g["n"] == N1
    np.testing.assert_array_equal(g["ids"], np.arange(N1))
    loaded = nz.Index.load(path, load_data=False)
    assert loaded.graphBuilder() == 0
    assert_same_search(search(loaded, Q), search(a, Q))
    assert_same_search(search(loaded, Q), cut_l2["search"])
    a.close()
    loaded.close()


@pytest.mark.parametrize("params", [dict(gpu_build=1), dict(gpu_build=1, gpu_append=1, post=1),
                                    dict(gpu_append=1, indexThreadQty=1), dict(gpu_build=1, gpu_append=1, gpu_shards=2)],
                         ids=["no-gpu_append", "post1", "host-builder", "two-shards"])
def test_fallbacks_rebuild_in_full_as_before(params):
    n0, n1 = 1500, 2000
    X, Q = refio.s_lowrank(n1, 16, 341), refio.s_lowrank(64, 16, 342)
    P = dict(M=8, efConstruction=40, **params)
    idx = make_index("l2", "hnsw", X[:n0], **P)
    idx.knnQueryBatch(Q, K)
    assert idx.stats()["rows_appended"] == 0
    add_rows(idx, X, n0, n1)
    idx.finalize()
    st = idx.stats()
    assert st["rows_appended"] == 0 and st["rows_uploaded"] == n1 and st["rows"] == n1, st
    fresh = make_index("l2", "hnsw", X, **P)
    assert_same_search(search(idx, Q), search(fresh, Q), counters=st["shards"] == 1)
    assert idx.graphBuilder() == fresh.graphBuilder()
    idx.close()
    fresh.close()


def test_create_index_first_then_add_query_add_query(data, cut_l2):
    """lib.zig's order: nmslib_create_index on the empty index, rows afterwards.  The first finalize builds in full, the
    second one appends."""
    X, Q = data["l2"], data["Q"]
    idx = nz.Index("l2", "hnsw")
    idx.buildIndex(gpu_append=1, **BUILD)
    idx.addDenseBatch(X[:N0])
    idx.setQueryTimeParams(efSearch=20)
    ids, _, _ = idx.knnQueryBatch(Q, K)
    st = idx.stats()
    assert st["rows_appended"] == 0 and st["rows_uploaded"] == N0 and ids.max() < N0, st
    add_rows(idx, X, N0, N1)
    got = search(idx, Q)
    st = idx.stats()
    assert st["rows_appended"] == N1 - N0 == st["rows_uploaded"] and idx.graphBuilder() == 2, st
    assert_same_search(got, cut_l2["search"])
    idx.close()


@pytest.mark.parametrize("second", [dict(M=6, efConstruction=40, indexThreadQty=1),
                                    dict(M=6, efConstruction=40, indexThreadQty=1, gpu_defer=1),
                                    dict(M=8, efConstruction=60, delaunay_type=3, indexThreadQty=1, gpu_defer=1)],
                         ids=["other-M", "other-M-deferred", "same-M-deferred"])
def test_second_create_index_onto_the_host_builder_after_an_append(second, data, tmp_path):
    """nmslib_create_index again replaces the appended graph: what is saved afterwards is the host builder's graph, list
    for list, not lists fetched from the device where the appended graph (or nothing, deferred) lives."""
    n0, n1 = 800, 1200
    X, Q = data["l2"][:n1], data["Q"]
    idx, st = appended("l2", X, (n0, n1), **BUILD)
    assert st[1]["rows_appended"] == n1 - n0 and idx.graphBuilder() == 2
    idx.buildIndex(**second)
    assert idx.graphBuilder() == 1
    got = graph_of(idx, tmp_path, "second.idx")
    fresh = make_index("l2", "hnsw", X, **second)
    want = graph_of(fresh, tmp_path, "fresh.idx")
    assert_same_graph(got, want)
    np.testing.assert_array_equal(got["up_off"], want["up_off"])
    assert_same_search(search(idx, Q), search(fresh, Q))
    assert idx.stats()["rows_appended"] == 0
    idx.close()
    fresh.close()
