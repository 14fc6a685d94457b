"""-m gpu: an HNSW batch above 65536 queries goes through knn_device in slices; every slice writes its results and its
work counters at its own offset.  Row i of such a batch must be the answer to query i % 1024 of a 1024-query batch, bit
for bit (ids, distances, counts, ndc / hops / hops_up), on each of the three search paths."""
import numpy as np
import pytest

from tests import refio
from tests.gpuutil import make_index

pytestmark = pytest.mark.gpu

N, D, K = 1500, 16, 10
NQ_SMALL, NQ_BIG = 1024, 65536 + 100


@pytest.fixture(scope="module")
def index_and_queries():
    X, Q = refio.s_lowrank(N, D, 501), refio.s_lowrank(NQ_SMALL, D, 502)
    assert len(np.unique(Q, axis=0)) == NQ_SMALL
    idx = make_index("l2", "hnsw", X, M=8, efConstruction=40, indexThreadQty=1)
    yield idx, Q, np.ascontiguousarray(np.tile(Q, (NQ_BIG // NQ_SMALL + 1, 1))[:NQ_BIG])
    idx.close()


# (32, v1merge): LDS visited table + the overflow list; (32, old): SearchOld; (1100, v1merge): the HBM-array kernel
@pytest.mark.parametrize("ef,algo", [(32, "v1merge"), (32, "old"), (1100, "v1merge")])
def test_sliced_batch_equals_the_small_batch(index_and_queries, ef, algo):
    idx, Q, big = index_and_queries
    idx.setQueryTimeParams(efSearch=ef, algoType=algo)
    ids, ds, cnt = idx.knnQueryBatch(Q, K)
    counters = idx.read_counters(NQ_SMALL)
    assert (cnt == K).all()
    bids, bds, bcnt = idx.knnQueryBatch(big, K)
    bcounters = idx.read_counters(NQ_BIG)
    src = np.arange(NQ_BIG) % NQ_SMALL
    np.testing.assert_array_equal(bids, ids[src])
    np.testing.assert_array_equal(bds.view(np.uint32), ds.view(np.uint32)[src])
    np.testing.assert_array_equal(bcnt, cnt[src])
    for name, got, want in zip(("ndc", "hops", "hops_up"), bcounters, counters):
        assert got.shape == (NQ_BIG,)
        np.testing.assert_array_equal(got, want[src], err_msg=name)


# ---- the inner slices (hnsw_search.cpp's workspace budget), cut at 100 queries through NMSLIB_HNSW_SLICE_MAXQ ----
@pytest.fixture(scope="module")
def index_with_deleted_rows():
    idx = make_index("l2", "hnsw", refio.s_lowrank(N, D, 501), M=8, efConstruction=40, indexThreadQty=1)
    dead = np.random.default_rng(503).permutation(N)[:N * 3 // 10].astype(np.int32)
    assert idx.deleteIds(dead) == len(dead)
    yield idx
    idx.close()


def answer(idx, Q):
    ids, ds, cnt = idx.knnQueryBatch(Q, K)
    return (ids, np.ascontiguousarray(ds).view(np.uint32), cnt) + tuple(c.copy() for c in idx.read_counters(len(Q)))


INNER = [
    # (deleted rows, ef, algo, gpu_rows)
    (False, 32, "old", "f32"),        # SearchOld's slices
    (False, 1100, "v1merge", "f32"),  # the HBM-array kernel's slices
    (True, 32, "v1merge", "f32"),     # two stages over the LDS kernels
    (True, 32, "old", "f32"),         # two stages over SearchOld, sliced again
    (True, 1100, "v1merge", "f32"),   # two stages over the HBM-array kernel, sliced again
    (True, 32, "v1merge", "f16"),     # two stages over the fp16 walk and its re-rank
]


@pytest.mark.parametrize("nq", [100, 101, 250])  # one full slice; a tail of one; two slices and a tail of 50
@pytest.mark.parametrize("deleted,ef,algo,rows", INNER)
def test_inner_slices_equal_the_uncut_batch(index_and_queries, index_with_deleted_rows, monkeypatch, deleted, ef, algo, rows,
                                            nq):
    idx, Q = (index_with_deleted_rows if deleted else index_and_queries[0]), index_and_queries[1][:nq]
    idx.setQueryTimeParams(efSearch=ef, algoType=algo, gpu_rows=rows)
    try:
        monkeypatch.delenv("NMSLIB_HNSW_SLICE_MAXQ", raising=False)
        want = answer(idx, Q)
        assert idx.stats()["last_path"] == (5 if rows == "f16" else 4)
        monkeypatch.setenv("NMSLIB_HNSW_SLICE_MAXQ", "100")
        got = answer(idx, Q)
    finally:
        idx.setQueryTimeParams(gpu_rows="f32")
    for name, g, w in zip(("ids", "distance bits", "counts", "ndc", "hops", "hops_up"), got, want):
        assert g.shape[0] == nq
        np.testing.assert_array_equal(g, w, err_msg=name)
