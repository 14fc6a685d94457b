"""-m gpu: batched range queries on the exact scan (nmslib_gpu_range_query_batch*).

Two yardsticks.  The single entry nmslib_range_query_fill is existing code the batch must equal bit for bit: ids, distance
bits, counts, padding, totals.  And planted answers (tests/test_gpu_range_edges.py: rows of small integers whose distances
are exact in any summation order) are known from the construction alone.  The tile, the bound of the batched dimension and
the slice sizes come from the plan's restatement tests/range_batch_plan_ref.py.  External ids are 3 * position + 11; every
host call goes through batch_guarded (sentinels behind the buffers)."""
import zlib

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import range_batch_plan_ref as rbp
from tests.gpuutil import (CNT_SENTINEL, FLOAT_SPACES, ID_SENTINEL, _GUARD, _offset_buffer, close_rel, enqueue_knn,
                           expect_path, make_index, range_fill_guarded, same_bits)
from tests.test_gpu_range_edges import BLOCK, PASS, bits, ext_ids, grid_pool, pattern_mask, planted

pytestmark = pytest.mark.gpu

T = rbp.QUERY_TILE
SPACE_INCOMPATIBLE = 5


def batch_guarded(idx, Q, radii, cap, counts=True, totals=True):
    """One nmslib_gpu_range_query_batch whose four outputs go on for _GUARD sentinel elements -> ids [Q, cap], dists
    [Q, cap], counts [Q], totals [Q] (the sentinels where an output was passed as NULL)"""
    Q = np.ascontiguousarray(Q)
    nq = len(Q)
    r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float64), (nq,)))
    ids = np.full(nq * cap + _GUARD, ID_SENTINEL, np.int32)
    ds = np.full(nq * cap + _GUARD, np.nan, np.float32)
    cnt = np.full(nq + _GUARD, CNT_SENTINEL, np.int32)
    tot = np.full(nq + _GUARD, CNT_SENTINEL, np.int32)
    nz._check(nz.lib().nmslib_gpu_range_query_batch(idx.h, Q.ctypes.data, nq, Q.shape[1], r.ctypes.data, cap,
                                                    ids.ctypes.data if cap else None, ds.ctypes.data if cap else None,
                                                    cnt.ctypes.data if counts else None, tot.ctypes.data if totals else None),
              idx.alloc)
    assert (ids[nq * cap:] == ID_SENTINEL).all() and np.isnan(ds[nq * cap:]).all(), "written outside ids / dists"
    assert (cnt[nq:] == CNT_SENTINEL).all() and (tot[nq:] == CNT_SENTINEL).all(), "written outside counts / totals"
    return ids[:nq * cap].reshape(nq, cap), ds[:nq * cap].reshape(nq, cap), cnt[:nq], tot[:nq]


def dist64(space, X, q):
    """the space's distance of every row to q in float64"""
    x, y = X.astype(np.float64), q.astype(np.float64)
    if space == "l2sqr_sift":
        return ((x - y) ** 2).sum(1)
    if space == "l2":
        return np.sqrt(((x - y) ** 2).sum(1))
    if space == "l1":
        return np.abs(x - y).sum(1)
    if space == "linf":
        return np.abs(x - y).max(1)
    if space == "negdotprod":
        return -(x @ y)
    cos = np.clip((x @ y) / (np.linalg.norm(x, axis=1) * np.linalg.norm(y)), -1.0, 1.0)
    return np.arccos(cos) if space == "angulardist" else 1.0 - cos


def radius_of_kind(d, kind):
    """from a query's own sorted distances: kind 0 -> no row, 1 -> one, 2 -> about a dozen, 3 -> every row"""
    s = np.sort(d)
    if kind == 0:
        return float(s[0] - 1.0 - abs(s[0]))
    if kind == 3:
        return float(s[-1] + 1.0 + abs(s[-1]))
    m = 1 if kind == 1 else 12
    return float((s[m - 1] + s[m]) / 2) if m < len(s) else float(s[-1] + 1.0 + abs(s[-1]))


def expect_row(got, q, ids, ds, cap, total=None):
    """row q of a batch answer is the list (ids, ds) cut to cap, then the padding"""
    gi, gd, gc, gt = got
    m = min(len(ids), cap)
    assert gc[q] == m, (q, cap, gc[q], m)
    np.testing.assert_array_equal(gi[q, :m], ids[:m], err_msg=f"query {q} capacity {cap}")
    np.testing.assert_array_equal(bits(gd[q, :m]), bits(ds[:m]), err_msg=f"query {q} capacity {cap}")
    assert (gi[q, m:] == -1).all() and np.isposinf(gd[q, m:]).all(), (q, cap)
    if total is not None:
        assert gt[q] == total, (q, gt[q], total)


def equals_single_entry(idx, Q, radii, caps, n, path=10):
    """every capacity: the batch equals rangeQueryFill per query on the same index; totals = its count at n + 5"""
    full = [range_fill_guarded(idx, Q[q], radii[q], n + 5) for q in range(len(Q))]
    out = None
    for cap in caps:
        got = batch_guarded(idx, Q, radii, cap)
        expect_path(idx, path)
        for q in range(len(Q)):
            ids, ds = range_fill_guarded(idx, Q[q], radii[q], cap)
            expect_row(got, q, ids, ds, cap, len(full[q][0]))
            np.testing.assert_array_equal(ids, full[q][0][:cap])
        out = got
    return full, out


# ---- 1. equals the single entry --------------------------------------------------------------------------------------
def random_case(space, n, D, nq):
    rng = np.random.default_rng(zlib.crc32(f"{space} {n} {D}".encode()))
    if space == "l2sqr_sift":
        return rng.integers(0, 256, (n, 128)).astype(np.uint8), rng.integers(0, 256, (nq, 128)).astype(np.uint8)
    return rng.standard_normal((n, D)).astype(np.float32), rng.standard_normal((nq, D)).astype(np.float32)


@pytest.mark.parametrize("n", [1, 64, 65, 1025, 2049])
@pytest.mark.parametrize("space,D", [(s, D) for s in FLOAT_SPACES for D in (5, 64, 65, 129)] + [("l2sqr_sift", 128)])
def test_equals_the_single_entry(space, D, n):
    X, Q = random_case(space, n, D, T + 1)
    radii = np.array([radius_of_kind(dist64(space, X, Q[q]), q % 4) for q in range(len(Q))])
    ext = ext_ids(n)
    idx = make_index(space, "seq_search", X, ext)
    try:
        c = len(range_fill_guarded(idx, Q[2], radii[2], n + 5)[0])       # the chosen query: about a dozen
        caps = sorted({cap for cap in (1, c - 1, c, c + 1, n + 5) if cap > 0})
        for nq in (1, T - 1, T + 1):
            sel = slice(2, 3) if nq == 1 else slice(0, nq)
            full, got = equals_single_entry(idx, Q[sel], radii[sel], caps, n)
            if nq > 1:
                totals = {len(f[0]) for f in full}
                assert {0, n} <= totals and (n < 2 or 1 in totals) and (n < 64 or any(6 <= t <= 24 for t in totals)), totals
    finally:
        idx.close()


@pytest.mark.parametrize("D", [128, 192, 255])
@pytest.mark.parametrize("space", FLOAT_SPACES)
def test_equals_the_single_entry_full_and_widest_rows(space, D):
    """the kernel variants the dimensions above leave out: two and three full elements per lane, four with a ragged last
    one, for every float space; 321 rows: a second workgroup, its last wave ragged"""
    n = 321
    X, Q = random_case(space, n, D, T + 1)
    radii = np.array([radius_of_kind(dist64(space, X, Q[q]), q % 4) for q in range(len(Q))])
    idx = make_index(space, "seq_search", X, ext_ids(n))
    try:
        full, _ = equals_single_entry(idx, Q, radii, [1, 12, n + 5], n)
        assert {0, n} <= {len(f[0]) for f in full}
    finally:
        idx.close()


@pytest.mark.parametrize("space,D", [("l1", 5), ("cosinesimil", 65), ("l2sqr_sift", 128)])
def test_a_workgroup_takes_a_second_query_tile(space, D):
    """263 173 rows are 1029 workgroups, more than the grid aims at, so the plan gives one query split: with 33 queries
    every workgroup stages a full tile, then a ragged one of a single query over the same LDS.  The radii come from the
    distances of the first 4096 rows: none, about 64 and about 768 matches, and every row."""
    n, nq = PASS + BLOCK + 5, T + 1
    p = rbp.plan(n, D, 1 if space == "l2sqr_sift" else 4, nq, 100)
    assert p.route == 10 and p.slices == 1 and p.grid_y == 1 and rbp.ceil_div(nq, p.query_tile) == 2 and nq % p.query_tile == 1
    X, Q = random_case(space, n, D, nq)
    radii = np.empty(nq)
    for q in range(nq):
        s = np.sort(dist64(space, X[:4096], Q[q]))
        radii[q] = (-1.0 - abs(s[0]), (s[0] + s[1]) / 2, (s[11] + s[12]) / 2, 1e9)[q % 4]
    idx = make_index(space, "seq_search", X, ext_ids(n))
    try:
        full, got = equals_single_entry(idx, Q, radii, [1, 100], n)
        totals = [len(f[0]) for f in full]
        assert totals[0] == 0 and totals[3] == n and totals[nq - 1] == 0 and 1 <= totals[1] < totals[2] < n, totals[:4]
        assert got[3].tolist() == totals
    finally:
        idx.close()


# ---- 2. planted answers, independent of any code ---------------------------------------------------------------------
def word_mask(pattern, n):
    if pattern == "word_edges":      # the last row of a mask word and the first of the next
        return np.isin(np.arange(n) % 64, (63, 0))
    return pattern_mask(pattern, n)


def check_planted_batch(space, n, pattern, seed=0):
    """the grid query repeated; the radii stand on either side of the planted one, in the gaps of the exact distances, and
    (where the space is exact) on attained distances"""
    mask = word_mask(pattern, n)
    q, radius, X, d = planted(space, n, mask, seed)
    pool_d = np.unique(grid_pool(space)[3])
    mids = (pool_d[:-1] + pool_d[1:]) / 2
    below, above = mids[mids < radius], mids[mids > radius]
    radii = [radius, below[len(below) // 2], above[len(above) // 2], pool_d[0] - 1.0, pool_d[-1] + 1.0, above[0]]
    if space != "l2":
        radii += [float(pool_d[pool_d < radius][-1]), float(pool_d[pool_d > radius][0])]     # rows exactly on the radius
    conv = (lambda r: float(int(r))) if space == "l2sqr_sift" else (lambda r: float(np.float32(r)))
    ext = ext_ids(n)
    Q = np.repeat(q[None, :], len(radii), 0)
    idx = make_index(space, "seq_search", X, ext)
    try:
        assert ((d <= conv(radius)) == mask).all()
        c = int(mask.sum())
        for cap in sorted({cap for cap in (1, c, n + 5) if cap > 0}):
            gi, gd, gc, gt = batch_guarded(idx, Q, radii, cap)
            expect_path(idx, 10)
            for j, r in enumerate(radii):
                hit = d <= conv(r)
                m = min(int(hit.sum()), cap)
                assert gt[j] == hit.sum() and gc[j] == m, (j, r, gt[j], hit.sum(), gc[j])
                np.testing.assert_array_equal(gi[j, :m], ext[hit][:m], err_msg=f"radius {r} capacity {cap}")
                if space == "l2":
                    assert close_rel(gd[j, :m], d[hit][:m])
                else:
                    np.testing.assert_array_equal(bits(gd[j, :m]), bits(d[hit][:m]), err_msg=f"radius {r} capacity {cap}")
                assert (gi[j, m:] == -1).all() and np.isposinf(gd[j, m:]).all()
            assert gt[3] == 0 and gt[4] == n
    finally:
        idx.close()


PLANTED_N = (1023, 1024, 1025, 2 * 1024 + 1)
PLANTED_PATTERNS = ("none", "all", "first", "last", "block_edges", "wave_edges", "quad_edges", "half", "word_edges")


@pytest.mark.parametrize("pattern", PLANTED_PATTERNS)
@pytest.mark.parametrize("n", PLANTED_N)
@pytest.mark.parametrize("space", ["l1", "l2sqr_sift"])
def test_planted_answers_exact(space, n, pattern):
    check_planted_batch(space, n, pattern)


@pytest.mark.parametrize("n", PLANTED_N)
@pytest.mark.parametrize("space,pattern", [("l2", "word_edges"), ("linf", "half"), ("negdotprod", "quad_edges")])
def test_planted_answers_other_grid_spaces(space, pattern, n):
    check_planted_batch(space, n, pattern, seed=1)


# ---- 3. slice edges, the scan's second pass ------------------------------------------------------------------------------
def test_three_slices_with_a_ragged_last_one(monkeypatch):
    """NMSLIB_GPU_RANGE_WS_BYTES leaves room for two queries' masks: 5 queries run as slices of 2, 2 and 1"""
    n, nq = 1025, 5
    X, Q = random_case("l1", n, 5, nq)
    radii = np.array([radius_of_kind(dist64("l1", X, Q[q]), (q + 1) % 4) for q in range(nq)])
    idx = make_index("l1", "seq_search", X, ext_ids(n))
    try:
        whole = batch_guarded(idx, Q, radii, 13)
        budget = rbp.budget_for(n, 2) + 7
        assert rbp.slice_sizes(rbp.plan(n, 5, 4, nq, 13, budget), nq) == [2, 2, 1]
        monkeypatch.setenv("NMSLIB_GPU_RANGE_WS_BYTES", str(budget))
        cut = batch_guarded(idx, Q, radii, 13)
        expect_path(idx, 10)
        for a, b in zip(whole, cut):
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))
        equals_single_entry(idx, Q, radii, [13, n + 5], n)
        only = batch_guarded(idx, Q, radii, 0)                            # count only, sliced
        np.testing.assert_array_equal(only[3], whole[3])
        # a bound below one query's masks: the single-query launches
        monkeypatch.setenv("NMSLIB_GPU_RANGE_WS_BYTES", str(rbp.query_bytes(n) - 1))
        equals_single_entry(idx, Q, radii, [13], n, path=11)
    finally:
        idx.close()


def test_the_per_query_scan_crosses_its_second_pass():
    """n = 263 173 = PASS + BLOCK + 5 rows of D = 5, 3 queries: about 9 % of the rows on either side of position 262 144;
    one whose only matches are PASS - 1, PASS, PASS + 3 and n - 1, rows just beyond the radius beside them; none"""
    n = PASS + BLOCK + 5
    rng = np.random.default_rng(21)
    ext = ext_ids(n)
    at = np.array([PASS - 1, PASS, PASS + 3, n - 1])
    beside = np.array([5, PASS - 2, PASS + 1, PASS + 2, n - 2])
    X = rng.integers(1, 4, (n, 5)).astype(np.float32)
    X[at] = [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 1, 0, 0, 1], [0, 0, 0, 0, 2]]
    X[beside] = [[0, 0, 0, 0, 3], [1, 1, 0, 0, 1], [0, 0, 0, 0, 3], [2, 0, 0, 0, 1], [0, 0, 1, 1, 1]]
    Q = np.array([np.full(5, 3), np.zeros(5), np.zeros(5)], np.float32)
    radii = [2.0, 2.0, 0.5]
    D = [np.abs(X.astype(np.float64) - q).sum(1) for q in Q.astype(np.float64)]
    hits = [d <= r for d, r in zip(D, radii)]
    assert hits[0][PASS:].sum() >= 20 and hits[0][:PASS].sum() >= 1000
    assert np.nonzero(hits[1])[0].tolist() == at.tolist() and np.nonzero(hits[2])[0].tolist() == [PASS - 1]
    idx = make_index("l1", "seq_search", X, ext)
    try:
        for cap in (1, 3, 4, 5, int(hits[0].sum()), n + 5):
            got = batch_guarded(idx, Q, radii, cap)
            expect_path(idx, 10)
            for q in range(3):
                expect_row(got, q, ext[hits[q]], D[q][hits[q]], cap, int(hits[q].sum()))
        ids, ds = range_fill_guarded(idx, Q[1], 2.0, 5)
        expect_row(batch_guarded(idx, Q, radii, 5), 1, ids, ds, 5)
    finally:
        idx.close()


# ---- 4. route 11, count only -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["l2", "cosinesimil"])
def test_dimensions_at_and_beyond_the_batched_bound(space):
    n = 300
    for D, path in ((rbp.MAX_DIM, 10), (rbp.MAX_DIM + 1, 11)):
        assert rbp.plan(n, D, 4, 3, 7).route == path
        X, Q = random_case(space, n, D, 3)
        radii = np.array([radius_of_kind(dist64(space, X, Q[q]), (q + 2) % 4) for q in range(3)])
        idx = make_index(space, "seq_search", X, ext_ids(n))
        try:
            full, _ = equals_single_entry(idx, Q, radii, [1, 12, n + 5], n, path)
            only = batch_guarded(idx, Q, radii, 0, counts=False)
            expect_path(idx, path)
            assert only[3].tolist() == [len(f[0]) for f in full] and (only[2] == CNT_SENTINEL).all()
        finally:
            idx.close()


@pytest.mark.parametrize("space", ["l1", "l2sqr_sift"])
def test_count_only(space):
    n = 2049
    X, Q = random_case(space, n, 65, T + 1)
    radii = np.array([radius_of_kind(dist64(space, X, Q[q]), q % 4) for q in range(len(Q))])
    idx = make_index(space, "seq_search", X, ext_ids(n))
    try:
        full = batch_guarded(idx, Q, radii, 16)
        only = batch_guarded(idx, Q, radii, 0)
        np.testing.assert_array_equal(only[3], full[3])
        assert (only[2] == 0).all() and {0, n} <= set(only[3].tolist())
        ids, ds, cnt, tot = idx.rangeQueryBatch(Q, radii, 0)              # the mirror passes ids = dists = NULL
        assert ids.shape == (T + 1, 0) and tot.tolist() == full[3].tolist()
        ids, ds, cnt, tot = idx.rangeQueryBatch(Q[:3], radii[3], 16)      # a scalar radius broadcasts
        assert (tot == n).all() and (cnt == 16).all()
    finally:
        idx.close()


# ---- 5. deletes, consolidate, shards -----------------------------------------------------------------------------------
def test_delete_down_to_one_block_and_consolidate():
    """the delete sequence of tests/test_gpu_range_edges.py under a batch of 3 queries: after every step and after
    consolidate() the batch equals an index built from the live rows alone, the single entry, and the planted answer"""
    n = 2049
    mask = pattern_mask("half", n)
    mask[[0, 1022, 1023, 1024, 1025, n - 1]] = True
    q, radius, X, d = planted("l1", n, mask, seed=5)
    ext = ext_ids(n)
    Q = np.repeat(q[None, :], 3, 0)
    radii = [radius, radius - 1.0, radius + 1.0]
    idx = make_index("l1", "seq_search", X, ext)
    live = np.ones(n, bool)
    rng = np.random.default_rng(71)
    first = np.r_[1023, rng.permutation(np.setdiff1d(np.arange(1, n - 1), [1022, 1023, 1024, 1025]))[:1023]]

    def check():
        want = live & mask
        c, nl = int(want.sum()), int(live.sum())
        oracle = make_index("l1", "seq_search", X[live], ext[live])
        try:
            for cap in sorted({cap for cap in (1, c - 1, c, c + 1, nl + 5) if cap > 0}):
                a, b = batch_guarded(idx, Q, radii, cap), batch_guarded(oracle, Q, radii, cap)
                for x, y in zip(a, b):
                    np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"capacity {cap}")
                expect_row(a, 0, ext[want], d[want], cap, c)
                for j in (1, 2):
                    hit = live & (d <= radii[j])
                    expect_row(a, j, ext[hit], d[hit], cap, int(hit.sum()))
        finally:
            oracle.close()
        equals_single_entry(idx, Q, radii, [c], nl)

    try:
        check()
        for dead, left in ((first, 1025), ([1024], 1024), ([1025], 1023)):
            assert idx.deleteIds(ext[dead]) == len(dead)
            live[dead] = False
            assert live.sum() == left
            check()
        assert idx.consolidate()[0] == n - 1023 and idx.dataQty() == 1023
        check()
    finally:
        idx.close()


def test_three_shards_equal_one():
    """3075 rows in 3 shards of 1025: per query the shards' lists back to back up to the capacity, the totals summed"""
    n = 3075
    rng = np.random.default_rng(81)
    mask = rng.random(n) < 0.125
    mask[[1024, 1025, 2049, 2050, n - 1]] = True
    q, radius, X, d = planted("l1", n, mask, seed=6)
    ext = ext_ids(n)
    Q = np.repeat(q[None, :], 4, 0)
    radii = [radius, radius - 1.0, radius + 50.0, -1.0]
    in0 = int(mask[:1025].sum())                                          # a capacity that ends with shard 0's last match
    one = make_index("l1", "seq_search", X, ext, gpu_shards=1)
    many = make_index("l1", "seq_search", X, ext, gpu_shards=3)
    try:
        assert many.stats()["shards"] == 3 and one.stats()["shards"] == 1
        for cap in (1, in0 - 1, in0, in0 + 1, int(mask.sum()), n + 5, 0):
            a, b = batch_guarded(many, Q, radii, cap), batch_guarded(one, Q, radii, cap)
            expect_path(many, 10)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"capacity {cap}")
            if cap:
                expect_row(a, 0, ext[mask], d[mask], cap, int(mask.sum()))
            assert a[3].tolist()[2:] == [n, 0]
        # the device entry serves one device
        out = np.zeros(8, np.int32)
        r = np.ones(1, np.float64)
        rc = nz.lib().nmslib_gpu_range_query_batch_device(many.h, out.ctypes.data, 1, 4, r.ctypes.data, 0, None, None, None,
                                                          out.ctypes.data, None)
        assert rc == SPACE_INCOMPATIBLE and "one device" in nz.last_error_detail(many.alloc)
    finally:
        one.close()
        many.close()


# ---- 6. the device entry ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["l2", "l2sqr_sift"])
def test_device_entry_between_knn_batches_on_other_streams(space):
    """queries and outputs at odd element offsets, a stream of the caller's; a k-NN batch on a second stream in front of
    it and one on a third behind it"""
    import torch
    n, nq, cap = 2049, T + 1, 9
    X, Q = random_case(space, n, 65, nq)
    radii = np.array([radius_of_kind(dist64(space, X, Q[q]), q % 4) for q in range(nq)])
    idx = make_index(space, "seq_search", X, ext_ids(n))
    try:
        want = batch_guarded(idx, Q, radii, cap)
        knn_alone = [idx.knnQueryBatch(Q[:7], 5), idx.knnQueryBatch(Q[7:20], 3)]
        streams = [torch.cuda.Stream() for _ in range(3)]
        tdt = torch.uint8 if space == "l2sqr_sift" else torch.float32
        staged = torch.from_numpy(np.ascontiguousarray(Q)).cuda().reshape(-1)
        torch.cuda.current_stream().synchronize()
        q_off, out_off = 1, 3
        qraw, qbuf = _offset_buffer(nq * Q.shape[1], tdt, q_off)
        raws = [_offset_buffer(m, dt, out_off)[0] for m, dt in ((nq * cap, torch.int32), (nq * cap, torch.float32),
                                                               (nq, torch.int32), (nq, torch.int32))]
        at = lambda raw, off: raw.data_ptr() + off * raw.element_size()   # noqa: E731
        front = enqueue_knn(idx, Q[:7], 5, streams[0], q_off=3, out_off=1)
        with torch.cuda.stream(streams[1]):
            qbuf.copy_(staged)
            for raw, fill in zip(raws, (ID_SENTINEL, float("nan"), CNT_SENTINEL, CNT_SENTINEL)):
                raw.fill_(fill)
            idx.range_device(at(qraw, q_off), nq, Q.shape[1], radii, cap, *[at(r, out_off) for r in raws],
                             stream=streams[1].cuda_stream)
        expect_path(idx, 10)
        behind = enqueue_knn(idx, Q[7:20], 3, streams[2], q_off=1, out_off=5)
        for s in streams:
            s.synchronize()
        host = [r.cpu().numpy() for r in raws]
        for h, m, sentinel in zip(host, (nq * cap, nq * cap, nq, nq), (ID_SENTINEL, None, CNT_SENTINEL, CNT_SENTINEL)):
            guard = np.r_[h[:out_off], h[out_off + m:]]
            assert np.isnan(guard).all() if sentinel is None else (guard == sentinel).all(), "written outside an output"
        got = [h[out_off:out_off + m] for h, m in zip(host, (nq * cap, nq * cap, nq, nq))]
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g.view(np.uint32), w.reshape(-1).view(np.uint32))
        same_bits(front.result(), knn_alone[0])
        same_bits(behind.result(), knn_alone[1])
    finally:
        idx.close()


# ---- 7. determinism -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["angulardist", "l1"])
def test_the_same_batch_twice_and_in_reverse(space):
    n, nq = 2049, 2 * T + 1
    X, Q = random_case(space, n, 129, nq)
    radii = np.array([radius_of_kind(dist64(space, X, Q[q]), q % 4) for q in range(nq)])
    idx = make_index(space, "seq_search", X, ext_ids(n))
    try:
        a, b = batch_guarded(idx, Q, radii, 20), batch_guarded(idx, Q, radii, 20)
        c = batch_guarded(idx, Q[::-1], radii[::-1], 20)
        for x, y, z in zip(a, b, c):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
            np.testing.assert_array_equal(x.view(np.uint32), z[::-1].view(np.uint32))
    finally:
        idx.close()


# ---- 8. the radii's staging blocks ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("space,D,path,fractional", [("l2", 65, 10, False), ("l2", 257, 11, False),
                                                     ("l2sqr_sift", 128, 10, True)])
def test_device_batches_back_to_back_while_the_radii_blocks_grow(space, D, path, fractional):
    """four device batches of 5, 7, T + 1 and 2T + 1 queries on one stream, nothing waited for in between, on an index whose
    two staging blocks do not exist yet: the third call waits for the first one's copy and replaces its block, the fourth
    does so with the second's (both need more than the quarter of slack).  Every call's outputs equal what a twin index
    answers for that batch alone.  fractional (l2sqr_sift): radii k + 0.75 and -0.25, which the conversion truncates; there
    the twin's single entry is held against its batch as well, and a query that is a row finds that row alone"""
    import torch
    n, cap, off = 2049, 9, 3
    sizes = (5, 7, T + 1, 2 * T + 1)
    cuts = np.r_[0, np.cumsum(sizes)]
    X, Q = random_case(space, n, D, int(cuts[-1]))
    if fractional:
        Q[0] = X[17]                                                      # (distance 0: what a radius of -0.25 reaches as 0)
    radii = np.array([radius_of_kind(dist64(space, X, Q[q]), q % 4) for q in range(len(Q))])
    if fractional:
        radii = np.floor(radii) + 0.75
        assert (radii[0::4] == -0.25).all()
    twin = make_index(space, "seq_search", X, ext_ids(n))
    idx = make_index(space, "seq_search", X, ext_ids(n))
    try:
        want = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert rbp.plan(n, D, 1 if space == "l2sqr_sift" else 4, b - a, cap).route == path
            want.append(batch_guarded(twin, Q[a:b], radii[a:b], cap))
            expect_path(twin, path)
        if fractional:
            equals_single_entry(twin, Q[:12], radii[:12], [cap], n)
            assert want[0][3][0] == 1 and want[0][0][0, 0] == ext_ids(n)[17] and want[0][3][4] == 0
        staged = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
        torch.cuda.current_stream().synchronize()
        lens = [(m * cap, m * cap, m, m) for m in sizes]
        dts = (torch.int32, torch.float32, torch.int32, torch.int32)
        raws = [[_offset_buffer(m, dt, off)[0] for m, dt in zip(ln, dts)] for ln in lens]
        at = lambda raw: raw.data_ptr() + off * raw.element_size()   # noqa: E731
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            for (a, b), out in zip(zip(cuts[:-1], cuts[1:]), raws):
                for raw, fill in zip(out, (ID_SENTINEL, float("nan"), CNT_SENTINEL, CNT_SENTINEL)):
                    raw.fill_(fill)
                idx.range_device(staged[int(a)].data_ptr(), int(b - a), Q.shape[1], radii[a:b], cap, *[at(r) for r in out],
                                 stream=stream.cuda_stream)
        expect_path(idx, path)
        stream.synchronize()
        for out, ln, w in zip(raws, lens, want):
            for raw, m, sentinel, x in zip(out, ln, (ID_SENTINEL, None, CNT_SENTINEL, CNT_SENTINEL), w):
                h = raw.cpu().numpy()
                guard = np.r_[h[:off], h[off + m:]]
                assert np.isnan(guard).all() if sentinel is None else (guard == sentinel).all(), "written outside an output"
                np.testing.assert_array_equal(h[off:off + m].view(np.uint32), x.reshape(-1).view(np.uint32))
    finally:
        idx.close()
        twin.close()
