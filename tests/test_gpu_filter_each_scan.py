"""-m gpu: one filter per query in a batch, on an exact-scan index (brute_force / seq_search;
nmslib_gpu_knn_query_batch_filtered_each).

The yardstick (tests/filter_each_util.py) is the single-filter entry, one call per filter group over that group's queries:
ids, distances, counts and the routes (the child's path) are equal bit for bit.  On integer-grid rows, where every f32
distance is exact, numpy over the allowed live rows ordered by (distance, position) is a second, independent check."""
import numpy as np
import pytest

from tests import refio
from tests.filter_each_util import each, per_group, same_batch, take
from tests.gpuutil import make_index, same_bits
from tests.test_gpu_filter_hnsw import exact_distances, grid_rows, subset_oracle
from tests.test_gpu_filter_scan import _Filtered, ext_ids, rows_of

pytestmark = pytest.mark.gpu


def interleaved(nq, n_filters):
    return (np.arange(nq) % (n_filters + 1) - 1).astype(np.int32)


def four_filters(idx, n, seed):
    """50 %, one row, none, all"""
    masks = [np.random.default_rng(seed).random(n) < 0.5, np.arange(n) == 777, np.zeros(n, bool), np.ones(n, bool)]
    return [idx.makeFilter(m) for m in masks], masks


def close_all(filters, idx):
    for f in set(filters):
        f.close()
    idx.close()


@pytest.mark.parametrize("method", ["brute_force", "seq_search"])
@pytest.mark.parametrize("space", ["l2", "cosinesimil", "l2sqr_sift"])
def test_small_index(space, method):
    n = 3000
    X, Q = rows_of(space, n, 16, 1401), rows_of(space, 70, 16, 1402)
    idx = make_index(space, method, X, ext_ids(n))
    filters, masks = four_filters(idx, n, 1403)
    fq = interleaved(70, len(filters))
    for k in (10, 1, 16):                                          # (rows of 40, 4 and 64 bytes go back to the caller's order)
        want = per_group(idx, filters, fq, Q, k)
        got = each(idx, filters, fq, Q, k)
        same_batch(got, want)
        assert got[1] is None                                      # (no work counters after an exact scan)
        assert (got[0][2][fq == 1] == 1).all() and (got[0][2][fq == 2] == 0).all()   # k above a filter's row count
        order = np.argsort(fq, kind="stable")                      # plan order: no permutation is launched
        same_batch(each(idx, filters, fq[order], np.ascontiguousarray(Q[order]), k), take(got, order))
    # the same filter under two indices, and a batch of unfiltered queries only
    twice = each(idx, [filters[0], filters[3], filters[0]], (np.arange(70) % 3).astype(np.int32), Q, 10)
    same_bits(tuple(x[2::3] for x in twice[0]), idx.knnQueryBatchFiltered(filters[0], np.ascontiguousarray(Q[2::3]), 10))
    none = each(idx, filters, np.full(70, -1, np.int32), Q, 10)
    same_bits(none[0], idx.knnQueryBatch(Q, 10))
    close_all(filters, idx)


@pytest.mark.parametrize("method", ["brute_force", "seq_search"])
def test_equals_numpy_on_grid_rows(method):
    n = 3000
    X, Q = grid_rows("l2", n, 16, 1410), grid_rows("l2", 70, 16, 1411)
    X[2000] = X[17]                                                # a planted tie: order by position
    Q[1] = X[17]
    ids = ext_ids(n)
    dist = exact_distances("l2", X, Q)
    idx = make_index("l2", method, X, ids)
    filters, masks = four_filters(idx, n, 1412)
    masks[0][[17, 2000]] = True
    filters[0].close()
    filters[0] = idx.makeFilter(masks[0])
    fq = interleaved(70, len(filters))
    assert fq[1] == 0
    for k in (10, 1):
        got, _, _ = each(idx, filters, fq, Q, k)
        for g in range(-1, len(filters)):
            sel = np.nonzero(fq == g)[0]
            pos = np.arange(n) if g < 0 else np.nonzero(masks[g])[0]
            oi, od, oc = subset_oracle(dist[sel], pos, ids, k)
            # (l2 on an exact-scan index is the distance, not its square: the order is the same, the integers are compared)
            np.testing.assert_array_equal(got[0][sel], oi)
            np.testing.assert_array_equal(got[2][sel], oc)
            np.testing.assert_array_equal(np.where(oi >= 0, np.rint(got[1][sel].astype(np.float64) ** 2), np.inf), od)
    close_all(filters, idx)


def test_a_group_on_the_fast_path_next_to_one_off_it():
    """70 000 x 16 l2: 300 queries under a filter of 95 % of the rows (the fast path: at least 256 queries on at least 64k
    rows), 10 under one of 2 %, interleaved"""
    n = 70000
    X, Q = refio.s_lowrank(n, 16, 1420), refio.s_lowrank(310, 16, 1421)
    rng = np.random.default_rng(1422)
    idx = make_index("l2", "seq_search", X, ext_ids(n))
    filters = [idx.makeFilter(rng.random(n) < 0.95), idx.makeFilter(rng.random(n) < 0.02)]
    assert filters[0].allowed >= 65536
    fq = np.zeros(310, np.int32)
    fq[15::31] = 1                                                 # 10 of them
    assert (fq == 1).sum() == 10
    want = per_group(idx, filters, fq, Q, 10)
    got = each(idx, filters, fq, Q, 10)
    same_batch(got, want)
    assert (got[2][fq == 0] == 1).all() and (got[2][fq == 1] == 0).all()
    st = idx.stats()
    assert st["last_path"] == 9 and st["fast_tiles"] == 0          # the statistics describe the group that ran last
    # ... and when that group is the one on the fast path they point into its child: gone with the filter
    both = [filters[1], filters[0]]
    got = each(idx, both, 1 - fq, Q, 10)
    same_bits(got[0], want[0])
    assert idx.stats()["fast_tiles"] > 0
    filters[0].close()
    st = idx.stats()
    assert (st["fast_tiles"], st["fast_tiles_precise"], st["fast_tiles_fallback"]) == (0, 0, 0), st
    filters[1].close()
    idx.close()


def test_both_filters_gather_again_after_a_delete():
    n = 2000
    X, Q = refio.s_gauss(n, 24, 1430), refio.s_gauss(30, 24, 1431)
    ids = ext_ids(n)
    idx = make_index("l2", "seq_search", X, ids)
    masks = [np.arange(n) % 2 == 0, np.arange(n) % 3 == 0]
    filters = [idx.makeFilter(m) for m in masks]
    fq = interleaved(30, 2)
    first = each(idx, filters, fq, Q, 10)
    dead = np.unique(first[0][0][:, 0])                            # every query's nearest row under its filter
    assert idx.deleteIds(dead) == len(dead)
    want = per_group(idx, filters, fq, Q, 10)
    for f, m in zip(filters, masks):
        assert f.allowed == int((m & ~np.isin(ids, dead)).sum())
    again = [idx.makeFilter(m) for m in masks]                     # (gathered after the delete: the same children)
    got = each(idx, filters, fq, Q, 10)
    same_batch(got, want)
    same_batch(each(idx, again, fq, Q, 10), want)
    assert not np.isin(got[0][0], dead).any()
    close_all(filters + again, idx)


def test_groups_beyond_32768_queries_are_cut():
    n, nq_small, big = 200, 1000, 40000
    X, Q = refio.s_gauss(n, 8, 1440), refio.s_gauss(nq_small, 8, 1441)
    idx = make_index("l2", "seq_search", X, ext_ids(n))
    filters = [idx.makeFilter(np.arange(n) % 2 == 0), idx.makeFilter(np.arange(n) % 5 == 0)]
    small = [idx.knnQueryBatchFiltered(f, Q, 10) for f in filters]
    src = np.arange(big + 5) % nq_small
    fq = np.zeros(big + 5, np.int32)
    at = np.array([3, 20000, 32767, 32768, 40004])
    fq[at] = 1
    got, _, routes = each(idx, filters, fq, np.ascontiguousarray(Q[src]), 10)
    zero = fq == 0
    same_bits(tuple(x[zero] for x in got), tuple(x[src[zero]] for x in small[0]))
    same_bits(tuple(x[at] for x in got), tuple(x[src[at]] for x in small[1]))
    assert len(np.unique(routes)) == 1
    close_all(filters, idx)


def test_the_device_entry_on_a_foreign_stream():
    """tests.gpuutil.knn_on_stream through the new entry: unaligned buffers, sentinels around the outputs"""
    from tests.gpuutil import knn_on_stream
    n = 2000
    X, Q = rows_of("l2", n, 24, 1450), rows_of("l2", 9, 24, 1451)
    idx = make_index("l2", "seq_search", X, ext_ids(n))
    filters = [idx.makeFilter(np.arange(n) % 3 != 0), idx.makeFilter(np.arange(n) % 7 == 0)]
    fq = np.array([1, 0, -1, 1, 0, -1, 0, 0, 1], np.int32)
    want = each(idx, filters, fq, Q, 10)[0]

    class Each:
        def knn_device(self, *args):
            idx.knn_device_each_filtered(filters, fq, *args)

    same_bits(knn_on_stream(Each(), Q, 10, q_off=1, out_off=3), want)
    nocnt = knn_on_stream(Each(), Q, 10, counts=False)
    np.testing.assert_array_equal(nocnt[0], want[0])
    assert _Filtered is not None
    close_all(filters, idx)
