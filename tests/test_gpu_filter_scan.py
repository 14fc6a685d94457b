"""-m gpu: filtered k-NN on an exact-scan index (brute_force / seq_search; nmslib_gpu_filter_*).

A filter on such an index is the index of the allowed live rows alone, gathered and prepared in HBM.  So the oracle is a
second index built from only those rows under the same ids, as in tests/test_gpu_scan_delete.py: ids, distances and counts
are equal bit for bit, and so is the path the batch took."""
import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import refio
from tests.gpuutil import FLOAT_SPACES, knn_on_stream, make_index, same_bits

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 2


def ext_ids(n):
    return (3 * np.arange(n) + 11).astype(np.int32)


def rows_of(space, n, d, seed):
    return refio.s_sift_like(n, seed) if space == "l2sqr_sift" else refio.s_gauss(n, d, seed)


def words_of(mask, garbage=False):
    """the mask as uint32 words; garbage: every bit at or beyond len(mask) set, and one more word of ones behind"""
    n = len(mask)
    bits = np.zeros((n + 31) // 32 * 32, bool)
    bits[:n] = mask
    if garbage:
        bits[n:] = True
    w = np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)
    return np.r_[w, np.uint32(0xFFFFFFFF)] if garbage else w


def oracle_answers(space, X, ids, allowed_pos, Q, ks, method="seq_search"):
    """the batch on an index of the rows at allowed_pos alone -> {k: (ids, dists, counts)}, the last batch's path"""
    o = make_index(space, method, X[allowed_pos], ids[allowed_pos])
    out = {k: o.knnQueryBatch(Q, k) for k in ks}
    path = o.stats()["last_path"]
    o.close()
    return out, path


def check_filter(idx, flt, space, X, ids, allowed_pos, Q, ks, method="seq_search"):
    want, path = oracle_answers(space, X, ids, allowed_pos, Q, ks, method)
    for k in ks:
        got = idx.knnQueryBatchFiltered(flt, Q, k)
        same_bits(got, want[k])
        assert (got[2] == min(k, len(allowed_pos))).all()
    assert idx.stats()["last_path"] == path
    assert flt.allowed == len(allowed_pos) and flt.hbm_bytes > 0


def empty_answer(idx, flt, Q, k):
    ids, ds, cnt = idx.knnQueryBatchFiltered(flt, Q, k)
    assert (cnt == 0).all() and (ids == -1).all() and np.isposinf(ds).all()


@pytest.mark.parametrize("D", [1, 7, 128, 129])
@pytest.mark.parametrize("space", FLOAT_SPACES)
def test_filters_on_every_dense_float_space(space, D):
    n = 2000
    X, Q = rows_of(space, n, D, 1201), rows_of(space, 9, D, 1202)
    X[1501] = X[40]                                              # a planted duplicate: both allowed, order by position
    ids = ext_ids(n)
    idx = make_index(space, "seq_search", X, ids)
    before = idx.knnQueryBatch(Q, 10)
    hbm, mem = idx.stats()["hbm_bytes"], nz.lib().nmslib_index_memory_usage(idx.h)
    every_third = np.arange(n) % 3 == 1                          # holds 40 and 1501
    masks = {"all": np.ones(n, bool), "one": np.arange(n) == 777, "third": every_third,
             "few": np.isin(np.arange(n), [5, 40, 1501, 1999])}   # k = 10 > 4 allowed rows
    for name, mask in masks.items():
        flt = idx.makeFilter(mask)
        check_filter(idx, flt, space, X, ids, np.nonzero(mask)[0], Q, (1, 10))
        flt.close()
    if space != "negdotprod" and D > 1:                           # (the row itself is its nearest row, twice)
        dup = idx.makeFilter(every_third)
        got = idx.knnQueryBatchFiltered(dup, X[40:41], 2)
        np.testing.assert_array_equal(got[0][0], ids[[40, 1501]])
        assert got[1][0][0] == got[1][0][1]
        dup.close()
    none = idx.makeFilter(np.zeros(n, bool))
    assert none.allowed == 0
    empty_answer(idx, none, Q, 10)
    none.close()
    # the index itself is what it was: same bits, same accounting
    same_bits(idx.knnQueryBatch(Q, 10), before)
    assert idx.stats()["hbm_bytes"] == hbm and nz.lib().nmslib_index_memory_usage(idx.h) == mem
    idx.close()


@pytest.mark.parametrize("n", [2047, 2048])
def test_l2sqr_sift(n):
    X, Q = refio.s_sift_like(n, 1203), refio.s_sift_like(9, 1204)
    ids = ext_ids(n)
    idx = make_index("l2sqr_sift", "brute_force", X, ids)
    for mask in (np.ones(n, bool), np.arange(n) % 3 == 0, np.arange(n) == n - 1):
        flt = idx.makeFilter(mask)
        check_filter(idx, flt, "l2sqr_sift", X, ids, np.nonzero(mask)[0], Q, (1, 10), method="brute_force")
        flt.close()
    idx.close()


@pytest.mark.parametrize("n", [33, 64, 65])
def test_the_last_bit_and_garbage_beyond_it(n):
    """words given directly: the last row allowed, every bit at or beyond n set as well, one more word behind"""
    X, Q = refio.s_gauss(n, 7, 1205), refio.s_gauss(5, 7, 1206)
    ids = ext_ids(n)
    idx = make_index("l2", "seq_search", X, ids)
    mask = np.zeros(n, bool)
    mask[[0, 31, 32, n - 1]] = True
    flt = idx.makeFilter(words_of(mask, garbage=True))
    check_filter(idx, flt, "l2", X, ids, np.nonzero(mask)[0], Q, (1, 10))
    flt.close()
    idx.close()


def test_the_fast_path_runs_over_the_allowed_rows():
    """100 000 x 32 l2, 70 000 rows allowed, 256 queries: the filter's index takes the fast path, as its oracle does"""
    n = 100000
    X, Q = refio.s_lowrank(n, 32, 1207), refio.s_lowrank(256, 32, 1208)
    ids = ext_ids(n)
    allowed = np.sort(np.random.default_rng(1209).permutation(n)[:70000])
    mask = np.zeros(n, bool)
    mask[allowed] = True
    idx = make_index("l2", "seq_search", X, ids)
    flt = idx.makeFilter(mask)
    check_filter(idx, flt, "l2", X, ids, allowed, Q, (10,))
    st = idx.stats()
    assert st["last_path"] == 1 and st["fast_tiles"] > 0, st
    tiles = st["fast_tiles"]
    assert flt.hbm_bytes >= 70000 * 32 * 4
    # the statistics of that batch pointed into the filter's workspaces: once the filter is gone they read nothing of it
    flt.close()
    st = idx.stats()
    assert (st["fast_tiles"], st["fast_tiles_precise"], st["fast_tiles_fallback"]) == (0, 0, 0), st
    # ... nor after the filter's index was prepared again (a delete), nor after a filter destroyed behind an unfiltered batch
    flt = idx.makeFilter(mask)
    idx.knnQueryBatchFiltered(flt, Q, 10)
    assert idx.stats()["fast_tiles"] == tiles
    assert idx.deleteIds(ids[allowed[:1]]) == 1
    idx.knnQueryBatchFiltered(flt, Q[:8], 10)                    # gathers again; a small batch: the adaptive path
    assert idx.stats()["last_path"] == 0 and idx.stats()["fast_tiles"] == 0
    idx.knnQueryBatchFiltered(flt, Q, 10)
    unf = idx.knnQueryBatch(Q, 10)
    own = idx.stats()
    assert own["last_path"] == 1 and own["fast_tiles"] == tiles
    flt.close()
    assert idx.stats() == own                                    # the index's own flags stay
    same_bits(idx.knnQueryBatch(Q, 10), unf)
    idx.close()


def test_k_beyond_the_selection_kernels():
    n = 2000
    X, Q = refio.s_gauss(n, 16, 1210), refio.s_gauss(5, 16, 1211)
    ids = ext_ids(n)
    mask = np.arange(n) % 3 == 0                                  # 667 rows
    idx = make_index("l2", "seq_search", X, ids)
    flt = idx.makeFilter(mask)
    check_filter(idx, flt, "l2", X, ids, np.nonzero(mask)[0], Q, (600,))
    assert idx.stats()["last_path"] == 5
    flt.close()
    idx.close()


def test_delete_add_and_consolidate_under_a_filter():
    n = 2000
    X, Q = refio.s_gauss(n + 100, 24, 1212), refio.s_gauss(9, 24, 1213)
    ids = ext_ids(n + 100)
    mask = np.arange(n) % 2 == 0
    allowed = np.nonzero(mask)[0]
    idx = make_index("l2", "seq_search", X[:n], ids[:n])
    flt = idx.makeFilter(mask)
    first = idx.knnQueryBatchFiltered(flt, Q, 10)
    # delete every query's nearest allowed row and one row the filter does not allow: the next batch gathers again
    dead = np.unique(np.r_[first[0][:, 0], ids[1]])
    assert idx.deleteIds(dead) == len(dead)
    live = allowed[~np.isin(ids[allowed], dead)]
    check_filter(idx, flt, "l2", X, ids, live, Q, (10,))
    assert not np.isin(idx.knnQueryBatchFiltered(flt, Q, 10)[0], dead).any()
    # rows added afterwards are not allowed, whatever they are: the queries themselves go in
    idx.addDenseBatch(np.r_[Q, X[n + 9:]], ids[n:])
    assert idx.dataQty() == n + 100
    check_filter(idx, flt, "l2", X, ids, live, Q, (10,))
    unf = idx.knnQueryBatch(Q, 1)
    np.testing.assert_array_equal(unf[0][:, 0], ids[n:n + 9])     # (the unfiltered batch does find them)
    # a consolidate that removes rows moves positions: the filter is refused, a new one works
    removed, _ = idx.consolidate()
    assert removed == len(dead)
    with pytest.raises(nz.NmslibError) as ei:
        idx.knnQueryBatchFiltered(flt, Q, 10)
    assert ei.value.code == INVALID_ARGUMENT and "stale" in str(ei.value), ei.value
    assert flt.allowed == 0
    flt.close()
    other = make_index("l2", "seq_search", X[:n], ids[:n])
    foreign = other.makeFilter(mask)
    with pytest.raises(nz.NmslibError) as ei:
        idx.knnQueryBatchFiltered(foreign, Q, 10)
    assert ei.value.code == INVALID_ARGUMENT and "another index" in str(ei.value), ei.value
    foreign.close()
    other.close()
    keep = np.setdiff1d(np.arange(n + 100), np.nonzero(np.isin(ids[:n], dead))[0])
    Xc, idc = np.r_[X[:n], Q, X[n + 9:]][keep], ids[keep]
    mask2 = np.arange(len(keep)) % 2 == 1
    again = idx.makeFilter(mask2)
    check_filter(idx, again, "l2", Xc, idc, np.nonzero(mask2)[0], Q, (10,))
    again.close()
    idx.close()


def test_a_consolidate_without_deleted_rows_and_a_reset():
    n = 300
    X, Q = refio.s_gauss(n, 8, 1214), refio.s_gauss(5, 8, 1215)
    ids = ext_ids(n)
    mask = np.arange(n) % 2 == 0
    idx = make_index("l2", "seq_search", X, ids)
    flt = idx.makeFilter(mask)
    assert idx.consolidate() == (0, 0)                           # nothing removed: positions keep their meaning
    check_filter(idx, flt, "l2", X, ids, np.nonzero(mask)[0], Q, (10,))
    idx.reset()
    idx.addDenseBatch(X, ids)
    idx.buildIndex()
    with pytest.raises(nz.NmslibError) as ei:
        idx.knnQueryBatchFiltered(flt, Q, 10)
    assert ei.value.code == INVALID_ARGUMENT and "stale" in str(ei.value), ei.value
    flt.close()
    idx.close()


class _Filtered:
    """what tests.gpuutil.knn_on_stream calls, routed through the filtered device entry"""

    def __init__(self, idx, flt):
        self.idx, self.flt = idx, flt

    def knn_device(self, *args):
        self.idx.knn_device_filtered(self.flt, *args)


@pytest.mark.parametrize("space,n", [("l2", 2000), ("l2sqr_sift", 2047)])
def test_the_device_entry_on_a_foreign_stream(space, n):
    """unaligned buffers, sentinels around the outputs, with and without counts: the host entry's bits"""
    X, Q = rows_of(space, n, 24, 1216), rows_of(space, 9, 24, 1217)
    ids = ext_ids(n)
    mask = np.arange(n) % 3 != 0
    idx = make_index(space, "seq_search", X, ids)
    flt = idx.makeFilter(mask)
    want = idx.knnQueryBatchFiltered(flt, Q, 10)
    got = knn_on_stream(_Filtered(idx, flt), Q, 10, q_off=1, out_off=3)
    same_bits(got, want)
    nocnt = knn_on_stream(_Filtered(idx, flt), Q, 10, counts=False)
    np.testing.assert_array_equal(nocnt[0], want[0])
    flt.close()
    idx.close()
