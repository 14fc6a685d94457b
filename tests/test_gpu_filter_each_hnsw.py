"""-m gpu: one filter per query in a batch, on an HNSW index (nmslib_gpu_knn_query_batch_filtered_each).

The yardstick (tests/filter_each_util.py) is the single-filter entry, one call per filter group over that group's queries:
ids, distances, counts, ndc / hops / hops_up and the routes are equal bit for bit.  On top of it two independent checks
without tolerances: numpy over the allowed live rows on integer-grid rows (the subset segment), and tests/inwalk_ref.py's
search over the saved graph (the in-walk segment)."""
import ctypes as C

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import batched_ref as br
from tests import inwalk_ref as ir
from tests import refio
from tests.filter_each_util import each, per_group, plan_order, same_batch, take
from tests.gpuutil import CNT_SENTINEL, ID_SENTINEL, make_index, same_bits
from tests.test_gpu_filter_hnsw import GPU, HOST, WALKS, exact_distances, ext_ids, grid_rows, subset_oracle

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT = 2
N, D, EF, NQ = 6000, 16, 64, 70


def mask_of(n, pos):
    m = np.zeros(n, bool)
    m[pos] = True
    return m


def mixed_filters(idx, n, seed):
    """-> filters, masks: 50 % (walk), 64 rows (= max(ef, k): subset), 65 rows (walk, counts below k), 40 rows (subset, 64
    keys), 100 rows under scan_rows (128 keys), 4096 rows under scan_rows (the LDS maximum), all rows, no rows, and the first
    filter again under another index"""
    rng = np.random.default_rng(seed)
    order = rng.permutation(n)
    masks = [rng.random(n) < 0.5, mask_of(n, order[:64]), mask_of(n, order[100:165]), mask_of(n, order[200:240]),
             mask_of(n, order[300:400]), mask_of(n, order[:4096]), np.ones(n, bool), np.zeros(n, bool)]
    scan = [0, 0, 0, 0, 4096, 4096, 0, 0]
    filters = [idx.makeFilter(m, scan_rows=s) for m, s in zip(masks, scan)]
    return filters + [filters[0]], masks + [masks[0]]


def interleaved(nq, n_filters):
    """-1, 0, 1, .., n_filters - 1, -1, ..: no two neighbours share a filter"""
    return (np.arange(nq) % (n_filters + 1) - 1).astype(np.int32)


def close_all(filters, idx):
    for f in set(filters):
        f.close()
    idx.close()


# ---- mixed routes in one batch -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(WALKS))
def test_mixed_routes(name):
    space, build, qparams, walk_path = WALKS[name]
    if space == "l2sqr_sift":
        X, Q = refio.s_sift_like(N, 1301), refio.s_sift_like(NQ, 1302)
    else:
        X, Q = refio.s_lowrank(N, D, 1301), refio.s_lowrank(NQ, D, 1302)
    idx = make_index(space, "hnsw", X, ext_ids(N), **build)
    idx.setQueryTimeParams(efSearch=EF, **qparams)
    filters, masks = mixed_filters(idx, N, 1303)
    fq = interleaved(NQ, len(filters))
    for k in (10, 1):
        want = per_group(idx, filters, fq, Q, k)
        got = each(idx, filters, fq, Q, k)
        same_batch(got, want)
        assert set(np.unique(got[2])) == {walk_path, 7}            # (the unfiltered path is the walk's)
        assert (got[2][fq == -1] == walk_path).all() and (got[2][fq == 1] == 7).all() and (got[2][fq == 2] == walk_path).all()
        if k == 10:
            assert (got[0][2][fq == 2] < k).any() and (got[0][2][fq == 7] == 0).all()
            assert (got[1][0][fq == 5] == 4096).all() and (got[1][0][fq == 3] == 40).all()   # ndc of the scans: their m
        # the same batch in plan order (no permutation is launched) and reversed
        for order in (plan_order(fq, got[2]), np.arange(NQ)[::-1]):
            again = each(idx, filters, fq[order], np.ascontiguousarray(Q[order]), k)
            same_batch(again, take(got, order))
    close_all(filters, idx)


def test_subset_segment_equals_numpy():
    """integer-grid rows, on which every f32 distance is exact: lists of 0, 1, 40, 64, 100 and 4096 rows in one launch"""
    n, d = 4200, 8
    X, Q = grid_rows("l2", n, d, 1310), grid_rows("l2", 42, d, 1311)
    ids = ext_ids(n)
    dist = exact_distances("l2", X, Q)
    idx = make_index("l2", "hnsw", X, ids, M=6, efConstruction=30, gpu_build=1)
    idx.setQueryTimeParams(efSearch=64)
    order = np.random.default_rng(1312).permutation(n)
    lists = [np.sort(order[:m]) for m in (0, 1, 40, 64, 100, 4096)]
    filters = [idx.makeFilter(mask_of(n, pos), scan_rows=4096) for pos in lists]
    fq = (np.arange(len(Q)) % len(filters)).astype(np.int32)
    for k in (10, 1, 70):
        got, ctr, routes = each(idx, filters, fq, Q, k)
        assert (routes == 7).all()
        for g, pos in enumerate(lists):
            sel = np.nonzero(fq == g)[0]
            same_bits(tuple(x[sel] for x in got), subset_oracle(dist[sel], pos, ids, k))
            assert (ctr[0][sel] == len(pos)).all() and (ctr[1][sel] == 0).all() and (ctr[2][sel] == 0).all()
    close_all(filters, idx)


# ---- the filter inside the walk ----------------------------------------------------------------------------------------
def test_inwalk_segment(tmp_path, monkeypatch):
    X, Q = br.make_rows("d16", N), br.make_rows("d16", NQ, seed=12)
    br.check_exact_inputs("l2", X)
    ids = ir.ext_ids(N)
    k = 10
    idx = make_index("l2", "hnsw", X, ids, indexThreadQty=1, **ir.BUILD)
    p = str(tmp_path / "g.idx")
    idx.save(p, save_data=False)
    g = refio.parse_index(p)
    masks = [np.arange(N) % 8 == 0, np.arange(N) % 8 == 1, mask_of(N, np.arange(40) * 149)]
    assert masks[0].sum() == 750 and masks[1].sum() == 750
    filters = [idx.makeFilter(m) for m in masks]
    fq = interleaved(NQ, len(filters))
    monkeypatch.delenv("NMSLIB_HNSW_SLICE_MAXQ", raising=False)
    idx.setQueryTimeParams(efSearch=EF, gpu_inwalk=1)
    want = per_group(idx, filters, fq, Q, k)
    got = each(idx, filters, fq, Q, k)
    same_batch(got, want)
    assert set(np.unique(got[2])) == {4, 7, 8}
    assert (got[2][fq == 0] == 8).all() and (got[2][fq == 1] == 8).all() and (got[2][fq == 2] == 7).all()
    assert (got[0][2][(fq == 0) | (fq == 1)] == k).all()
    for f in (0, 1):                                               # the rule, restated in Python over the saved graph
        sel = np.nonzero(fq == f)[0]
        res, ctr, _ = ir.search("l2", X, Q[sel], g, k, EF, masks[f], ids)
        same_bits(tuple(x[sel] for x in got[0]), res)
        for nm, a, b in zip(("ndc", "hops", "hops_up"), got[1], ctr):
            np.testing.assert_array_equal(a[sel], b, err_msg=nm)
    # slices of 7 queries: a slice's slots start where its queries do
    monkeypatch.setenv("NMSLIB_HNSW_SLICE_MAXQ", "7")
    same_batch(each(idx, filters, fq, Q, k), got)
    monkeypatch.delenv("NMSLIB_HNSW_SLICE_MAXQ")
    # the two stages on the same batch are left with fewer than k
    idx.setQueryTimeParams(efSearch=EF, gpu_inwalk=0)
    two = each(idx, filters, fq, Q, k)
    same_batch(two, per_group(idx, filters, fq, Q, k))
    assert set(np.unique(two[2])) == {4, 7}
    assert (two[0][2][(fq == 0) | (fq == 1)] < k).any()
    monkeypatch.setenv("NMSLIB_HNSW_SLICE_MAXQ", "7")
    same_batch(each(idx, filters, fq, Q, k), two)
    close_all(filters, idx)


@pytest.mark.parametrize("inwalk", [0, 1])
def test_tombstones(inwalk):
    """every query's nearest allowed row is deleted: the tombstones apply to every query, the unfiltered ones included"""
    X, Q = refio.s_lowrank(N, D, 1320), refio.s_lowrank(NQ, D, 1321)
    idx = make_index("l2", "hnsw", X, ext_ids(N), **GPU)
    idx.setQueryTimeParams(efSearch=EF, gpu_inwalk=inwalk)
    filters, masks = mixed_filters(idx, N, 1322)
    fq = interleaved(NQ, len(filters))
    first = each(idx, filters, fq, Q, 10)
    dead = np.unique(first[0][0][:, 0])
    dead = dead[dead >= 0]
    assert idx.deleteIds(dead) == len(dead)
    want = per_group(idx, filters, fq, Q, 10)
    got = each(idx, filters, fq, Q, 10)
    same_batch(got, want)
    assert not np.isin(got[0][0], dead).any()
    assert set(np.unique(got[2])) == ({8, 7} if inwalk else {4, 7})
    order = plan_order(fq, got[2])
    same_batch(each(idx, filters, fq[order], np.ascontiguousarray(Q[order]), 10), take(got, order))
    close_all(filters, idx)


# ---- degenerate batches ------------------------------------------------------------------------------------------------
def test_degenerate_batches():
    n = 2000
    X, Q = refio.s_lowrank(n, D, 1330), refio.s_lowrank(NQ, D, 1331)
    idx = make_index("l2", "hnsw", X, ext_ids(n), **HOST)
    idx.setQueryTimeParams(efSearch=EF)
    flt = idx.makeFilter(np.arange(n) % 2 == 0)
    none = np.full(NQ, -1, np.int32)
    plain = idx.knnQueryBatch(Q, 10)
    pctr = idx.read_counters(NQ)
    for filters in ([], [flt]):                                    # n_filters = 0, and a filter no query uses
        got, ctr, routes = each(idx, filters, none, Q, 10)
        same_bits(got, plain)
        for a, b in zip(ctr, pctr):
            np.testing.assert_array_equal(a, b)
        assert (routes == 4).all()
    one = idx.knnQueryBatchFiltered(flt, Q, 10)
    octr = idx.read_counters(NQ)
    got, ctr, routes = each(idx, [flt], np.zeros(NQ, np.int32), Q, 10)
    same_bits(got, one)
    for a, b in zip(ctr, octr):
        np.testing.assert_array_equal(a, b)
    assert (routes == 4).all()
    empty = idx.knnQueryBatchEachFiltered([flt], np.zeros(0, np.int32), Q[:0], 10, return_routes=True)
    assert [len(x) for x in empty] == [0, 0, 0, 0]
    close_all([flt], idx)


# ---- the cut at 65 536 queries -----------------------------------------------------------------------------------------
def test_slices_of_a_large_batch():
    """70 000 queries drawn from 1024: the batch is cut in plan order, results and counters land at the caller's offsets"""
    n, nq_small, nq_big, ef = 200, 1024, 70000, 32
    X, Q = refio.s_lowrank(n, 8, 1340), refio.s_lowrank(nq_small, 8, 1341)
    idx = make_index("l2", "hnsw", X, ext_ids(n), M=8, efConstruction=40, indexThreadQty=1)
    idx.setQueryTimeParams(efSearch=ef)
    rng = np.random.default_rng(1342)
    masks = [rng.random(n) < 0.5, rng.random(n) < 0.6, mask_of(n, rng.permutation(n)[:20])]
    assert masks[0].sum() > ef and masks[1].sum() > ef
    filters = [idx.makeFilter(m) for m in masks]
    small = per_group(idx, filters, np.arange(nq_small) % 4 - 1, Q, 10)
    assert set(np.unique(small[2])) == {4, 7}
    q = np.arange(nq_big)
    src = q % nq_small                                             # (1024 is a multiple of 4: src keeps the filter)
    got = each(idx, filters, (q % 4 - 1).astype(np.int32), np.ascontiguousarray(Q[src]), 10)
    assert got[1][0].shape == (nq_big,)
    same_batch(got, take(small, src))
    close_all(filters, idx)


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_stale_and_foreign_filters_are_named_and_nothing_is_written():
    n = 1000
    X, Q = refio.s_lowrank(n, D, 1350), refio.s_lowrank(8, D, 1351)
    idx = make_index("l2", "hnsw", X, ext_ids(n), **GPU)
    other = make_index("l2", "hnsw", X[:500], ext_ids(500), **GPU)
    good = idx.makeFilter(np.arange(n) % 2 == 0)
    foreign = other.makeFilter(np.arange(500) % 2 == 0)
    fq = np.zeros(8, np.int32)
    ids = np.full((8, 10), ID_SENTINEL, np.int32)
    ds = np.full((8, 10), np.nan, np.float32)
    cnt = np.full(8, CNT_SENTINEL, np.int32)
    routes = np.full(8, CNT_SENTINEL, np.int32)

    def refused(filters, j):
        hs = (C.c_void_p * len(filters))(*[f.h.value for f in filters])
        rc = nz.lib().nmslib_gpu_knn_query_batch_filtered_each(idx.h, hs, len(filters), fq.ctypes.data, Q.ctypes.data, 8, D, 10,
                                                               ids.ctypes.data, ds.ctypes.data, cnt.ctypes.data,
                                                               routes.ctypes.data)
        assert rc == INVALID_ARGUMENT
        assert f"filters[{j}]" in nz.last_error_detail(idx.alloc)
        assert (ids == ID_SENTINEL).all() and np.isnan(ds).all() and (cnt == CNT_SENTINEL).all()
        assert (routes == CNT_SENTINEL).all()

    refused([good, good, foreign], 2)                              # (no query uses it: every entry is checked)
    with pytest.raises(nz.NmslibError) as e:
        idx.knnQueryBatchEachFiltered([good, foreign], fq, Q, 10)
    assert e.value.code == INVALID_ARGUMENT and "filters[1]" in str(e.value) and "another index" in str(e.value)
    assert idx.deleteIds(ext_ids(n)[:1]) == 1 and idx.consolidate()[0] == 1
    fresh = idx.makeFilter(np.arange(n - 1) % 2 == 0)
    refused([fresh, good], 1)
    with pytest.raises(nz.NmslibError) as e:
        idx.knnQueryBatchEachFiltered([fresh, good], fq, Q, 10)
    assert e.value.code == INVALID_ARGUMENT and "filters[1]" in str(e.value) and "stale" in str(e.value)
    same_bits(idx.knnQueryBatchEachFiltered([fresh], fq, Q, 10), idx.knnQueryBatchFiltered(fresh, Q, 10))
    foreign.close()
    other.close()
    close_all([good, fresh], idx)


# ---- the device entry --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [True, False])
def test_device_entry_on_its_own_stream(counts):
    """knn_on_stream's pattern: a fresh stream, nothing waited for before the call; filter_of_query is overwritten as soon as
    the call has returned"""
    import torch
    n, k = 3000, 10
    X, Q = refio.s_lowrank(n, D, 1360), refio.s_lowrank(NQ, D, 1361)
    idx = make_index("l2", "hnsw", X, ext_ids(n), **GPU)
    idx.setQueryTimeParams(efSearch=EF)
    rng = np.random.default_rng(1362)
    filters = [idx.makeFilter(rng.random(n) < 0.5), idx.makeFilter(mask_of(n, rng.permutation(n)[:30])),
               idx.makeFilter(rng.random(n) < 0.3)]
    fq = interleaved(NQ, len(filters))
    want = each(idx, filters, fq, Q, k)
    staged = torch.from_numpy(Q).cuda().reshape(-1)
    torch.cuda.current_stream().synchronize()
    stream = torch.cuda.Stream()
    guard = 64
    qbuf = torch.empty(NQ * D, dtype=torch.float32, device="cuda")
    d_ids = torch.empty(NQ * k + guard, dtype=torch.int32, device="cuda")
    d_ds = torch.empty(NQ * k + guard, dtype=torch.float32, device="cuda")
    d_cnt = torch.empty(NQ + guard, dtype=torch.int32, device="cuda")
    routes = np.full(NQ, CNT_SENTINEL, np.int32)
    mine = fq.copy()
    with torch.cuda.stream(stream):
        qbuf.copy_(staged)
        d_ids.fill_(ID_SENTINEL)
        d_ds.fill_(float("nan"))
        d_cnt.fill_(CNT_SENTINEL)
        idx.knn_device_each_filtered(filters, mine, qbuf.data_ptr(), NQ, D, k, d_ids.data_ptr(), d_ds.data_ptr(),
                                     d_cnt.data_ptr() if counts else None, stream.cuda_stream, routes=routes)
        mine[:] = 99                                               # (the entry has read it)
    np.testing.assert_array_equal(routes, want[2])                 # (known when the call returns)
    assert idx.stats()["last_path"] == 9
    stream.synchronize()
    h_ids, h_ds, h_cnt = d_ids.cpu().numpy(), d_ds.cpu().numpy(), d_cnt.cpu().numpy()
    assert (h_ids[NQ * k:] == ID_SENTINEL).all() and np.isnan(h_ds[NQ * k:]).all() and (h_cnt[NQ:] == CNT_SENTINEL).all()
    if counts:
        same_bits((h_ids[:NQ * k].reshape(NQ, k), h_ds[:NQ * k].reshape(NQ, k), h_cnt[:NQ]), want[0])
    else:
        assert (h_cnt == CNT_SENTINEL).all()
        np.testing.assert_array_equal(h_ids[:NQ * k].reshape(NQ, k), want[0][0])
        np.testing.assert_array_equal(h_ds[:NQ * k].view(np.uint32), want[0][1].reshape(-1).view(np.uint32))
    for a, b in zip(idx.read_counters(NQ), want[1]):
        np.testing.assert_array_equal(a, b)
    close_all(filters, idx)


def test_device_batches_back_to_back_while_the_table_block_grows():
    """2 filters and 8 queries, then 5 filters and NQ queries under another filter_of_query, on one fresh stream with nothing
    waited for in between, on an index whose staging block does not exist yet: the second call waits for the first one's copy
    and replaces the block.  Results and routes equal a twin index's, batch by batch"""
    import torch
    n, k = 3000, 10
    X, Q = refio.s_lowrank(n, D, 1370), refio.s_lowrank(NQ, D, 1371)
    rng = np.random.default_rng(1372)
    masks = [rng.random(n) < 0.5, mask_of(n, rng.permutation(n)[:30]), rng.random(n) < 0.3, rng.random(n) < 0.7,
             mask_of(n, rng.permutation(n)[:50])]
    batches = [(2, 8, interleaved(8, 2)), (5, NQ, interleaved(NQ, 5)[::-1].copy())]
    twin = make_index("l2", "hnsw", X, ext_ids(n), **GPU)
    twin.setQueryTimeParams(efSearch=EF)
    twin_filters = [twin.makeFilter(m) for m in masks]
    want = [each(twin, twin_filters[:nf], fq, Q[:nq], k) for nf, nq, fq in batches]
    idx = make_index("l2", "hnsw", X, ext_ids(n), **GPU)
    idx.setQueryTimeParams(efSearch=EF)
    filters = [idx.makeFilter(m) for m in masks]
    staged = torch.from_numpy(Q).cuda().reshape(-1)
    torch.cuda.current_stream().synchronize()
    stream = torch.cuda.Stream()
    guard = 64
    outs = [(torch.empty(nq * k + guard, dtype=torch.int32, device="cuda"),
             torch.empty(nq * k + guard, dtype=torch.float32, device="cuda"),
             torch.empty(nq + guard, dtype=torch.int32, device="cuda")) for _, nq, _ in batches]
    routes = [np.full(nq, CNT_SENTINEL, np.int32) for _, nq, _ in batches]
    with torch.cuda.stream(stream):
        for (nf, nq, fq), (d_ids, d_ds, d_cnt), r in zip(batches, outs, routes):
            d_ids.fill_(ID_SENTINEL)
            d_ds.fill_(float("nan"))
            d_cnt.fill_(CNT_SENTINEL)
            mine = fq.copy()
            idx.knn_device_each_filtered(filters[:nf], mine, staged.data_ptr(), nq, D, k, d_ids.data_ptr(), d_ds.data_ptr(),
                                         d_cnt.data_ptr(), stream.cuda_stream, routes=r)
            mine[:] = 99                                           # (the entry has read it)
    stream.synchronize()
    for (nf, nq, fq), (d_ids, d_ds, d_cnt), r, w in zip(batches, outs, routes, want):
        h_ids, h_ds, h_cnt = d_ids.cpu().numpy(), d_ds.cpu().numpy(), d_cnt.cpu().numpy()
        assert (h_ids[nq * k:] == ID_SENTINEL).all() and np.isnan(h_ds[nq * k:]).all() and (h_cnt[nq:] == CNT_SENTINEL).all()
        same_bits((h_ids[:nq * k].reshape(nq, k), h_ds[:nq * k].reshape(nq, k), h_cnt[:nq]), w[0])
        np.testing.assert_array_equal(r, w[2], err_msg="routes")
    close_all(filters, idx)
    close_all(twin_filters, twin)
