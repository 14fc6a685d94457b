"""-m gpu: rows deleted from an exact-scan index (brute_force / seq_search; nmslib_gpu_delete_ids).

A delete marks the index dirty; the next use prepares it again over the live rows and their ids, in position order.  So
the index is, bit for bit, the one a caller gets by adding only the live rows under the same ids -- that second index is
the oracle: k-NN (ids, distances, counts), range results at two radii and last_path are equal."""
import numpy as np
import pytest

from tests import refio
from tests.gpuutil import expect_path, make_index, same_bits

pytestmark = pytest.mark.gpu

K = 10


def ext_ids(n):
    return (3 * np.arange(n) + 11).astype(np.int32)


def answers(idx, Q, k=K):
    """k-NN of the batch, the path it took, and two range queries around the first query's neighbours"""
    knn = idx.knnQueryBatch(Q, k)
    path = idx.stats()["last_path"]
    d = knn[1][0][:knn[2][0]]
    radii = (float(d[len(d) // 2]), float(d[-1]) * 1.0001) if len(d) else (1.0, 2.0)
    ranges = [idx.rangeQueryFill(Q[0], r, 64) for r in radii]
    return knn, path, ranges


def assert_same_index(got, want):
    same_bits(got[0], want[0])
    assert got[1] == want[1], (got[1], want[1])
    for (gi, gd), (wi, wd) in zip(got[2], want[2]):
        np.testing.assert_array_equal(gi, wi)
        np.testing.assert_array_equal(gd.view(np.uint32), wd.view(np.uint32))


def deleted_vs_live_only(space, X, Q, dead_pos, method="seq_search", calls=1, k=K):
    """-> (answers of the index after the delete, its path before the delete)"""
    ids = ext_ids(len(X))
    dead_pos = np.asarray(dead_pos)
    live = np.setdiff1d(np.arange(len(X)), dead_pos)
    idx = make_index(space, method, X, ids)
    idx.knnQueryBatch(Q, k)                                        # (resident and prepared with all rows first)
    path_before = idx.stats()["last_path"]
    marked = sum(idx.deleteIds(part) for part in np.array_split(ids[dead_pos], calls))
    assert marked == len(dead_pos) == idx.deletedRows() and idx.dataQty() == len(X)
    got = answers(idx, Q, k)
    assert idx.stats()["rows_uploaded"] == len(live) and idx.stats()["rows"] == len(X)
    assert not np.isin(got[0][0], ids[dead_pos]).any()
    for ri, _ in got[2]:
        assert not np.isin(ri, ids[dead_pos]).any()
    idx.close()
    oracle = make_index(space, method, X[live], ids[live])
    want = answers(oracle, Q, k)
    oracle.close()
    assert_same_index(got, want)
    return got, path_before


@pytest.fixture(scope="module")
def rows():
    return refio.s_lowrank(70000, 16, 851), refio.s_lowrank(300, 16, 852)


@pytest.mark.parametrize("space,fast", [("l2", 1), ("l1", 6)])
def test_fast_path_on_both_sides(rows, space, fast):
    X, Q = rows
    dead = np.random.default_rng(853).permutation(70000)[:4000]
    got, before = deleted_vs_live_only(space, X, Q, dead)
    assert before == fast and got[1] == fast


@pytest.mark.parametrize("space,fast", [("l2", 1), ("l1", 6)])
def test_deletion_takes_the_index_off_the_fast_path(rows, space, fast):
    """66 000 rows, 1000 deleted: the live count falls below the fast paths' 65 536 rows"""
    X, Q = rows
    dead = np.random.default_rng(854).permutation(66000)[:1000]
    got, before = deleted_vs_live_only(space, X[:66000], Q, dead)
    assert before == fast and got[1] == 0


def test_l2sqr_sift():
    X, Q = refio.s_sift_like(3000, 855), refio.s_sift_like(70, 856)
    deleted_vs_live_only("l2sqr_sift", X, Q, np.random.default_rng(857).permutation(3000)[:900], method="brute_force")


def test_fewer_live_rows_than_k():
    X, Q = refio.s_gauss(40, 8, 858), refio.s_gauss(7, 8, 859)
    got, _ = deleted_vs_live_only("l2", X, Q, np.random.default_rng(860).permutation(40)[:35])
    ids, ds, cnt = got[0]
    assert (cnt == 5).all() and (ids[:, 5:] == -1).all() and np.isposinf(ds[:, 5:]).all()


def test_a_delete_in_two_calls_equals_a_delete_in_one():
    X, Q = refio.s_lowrank(3000, 24, 861), refio.s_lowrank(70, 24, 862)
    dead = np.random.default_rng(863).permutation(3000)[:700]
    one, _ = deleted_vs_live_only("l2", X, Q, dead, calls=1)
    two, _ = deleted_vs_live_only("l2", X, Q, dead, calls=2)
    assert_same_index(two, one)


def test_delete_then_add_then_query():
    """the update sequence: rows deleted, new rows added under the same ids; equal to an index of the live rows in order"""
    X, Q = refio.s_lowrank(3200, 24, 864), refio.s_lowrank(70, 24, 865)
    ids = ext_ids(3200)
    dead = np.random.default_rng(866).permutation(3000)[:200]
    ids[3000:] = ids[dead]                                        # the 200 new rows carry the deleted ids
    idx = make_index("l2", "seq_search", X[:3000], ids[:3000])
    idx.knnQueryBatch(Q, K)
    assert idx.deleteIds(ids[dead]) == 200
    idx.addDenseBatch(X[3000:], ids[3000:])
    assert idx.deletedRows() == 200 and idx.dataQty() == 3200
    got = answers(idx, Q)
    new_first = idx.knnQueryBatch(X[3000:3070], 1)
    np.testing.assert_array_equal(new_first[0][:, 0], ids[3000:3070])      # a new row is found under its id, distance 0
    assert (new_first[1][:, 0] == 0).all()
    idx.close()
    live = np.setdiff1d(np.arange(3200), dead)
    oracle = make_index("l2", "seq_search", X[live], ids[live])
    assert_same_index(got, answers(oracle, Q))
    oracle.close()
