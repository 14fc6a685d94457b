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
