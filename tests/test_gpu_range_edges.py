"""-m gpu: range search and the big-k exact scan at every block, scan-pass and grid edge.

The selection of range_kernels.hip works in blocks of 1024 rows (256 threads x 4 rows, wave totals through LDS); its
scan kernel walks the block counts 256 at a time with a running carry (a second pass needs more than 262 144 rows); the
dense distance kernel caps its grid at 65 536 workgroups of 4 rows, the sparse and divergence ones at 8192 x 256 rows, the
Levenshtein one at 4096 x 256 rows.  Every case here plants its matches by construction, so the expected answer is known
without a rounding question:
  * grid data: dense rows of small integers (f32: values 0..3, uint8: l2sqr_sift), distances exact in any summation order;
  * continuous data (cosinesimil, angulardist): few matches, the radius in the widest gap of the float64 distances around
    the target rank, and no distance within 1e-5 relative of it;
  * pooled rows (sparse, divergences, strings): row i is pool[perm[i % 61]], the 61 distances come from the helpers
    tests/sparse_ref.py, tests/diverg_ref.py and tests/string_ref.py, the radius lies in a gap of them.
External ids are 3 * position + 11 everywhere; every call goes through range_fill_guarded (sentinels behind the buffers)."""
import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import diverg_ref, sparse_ref, string_ref
from tests.gpuutil import close_rel, expect_path, make_index, range_fill_guarded

pytestmark = pytest.mark.gpu

BLOCK = 1024                     # rows per selection block
PASS = 256 * BLOCK               # rows per pass of the scan kernel = the dense distance kernel's grid, 65 536 x 4 rows
SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2048, PASS - 1, PASS, PASS + 1,
         PASS + BLOCK + 5,       # one scan pass + one block + 5
         2 * PASS + BLOCK + 6)   # two passes + 1030 rows: the carry is added twice
STARRED = (1024, 1025, PASS, PASS + 1, PASS + BLOCK + 5, 2 * PASS + BLOCK + 6)
PATTERNS = ("none", "all", "first", "last", "block_edges", "wave_edges", "quad_edges", "half", "thousandth")
POOL = 61                        # prime: the pooled pattern does not line up with 64, 256 or 1024
CAP_SPARSE = 8192 * 256          # rows one launch of the sparse / divergence distance kernels covers without striding
CAP_LEVEN = 4096 * 256


def ext_ids(n):
    return (3 * np.arange(n) + 11).astype(np.int32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def pattern_mask(pattern, n):
    pos = np.arange(n)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "first":
        return pos == 0
    if pattern == "last":
        return pos == n - 1
    if pattern == "block_edges":     # the last row of every block and the first of the next
        return (pos % BLOCK == BLOCK - 1) | ((pos % BLOCK == 0) & (pos > 0))
    if pattern == "wave_edges":      # a wave holds 64 threads x 4 rows: the last row of one and the first of the next
        return np.isin(pos % BLOCK, (255, 256, 511, 512, 767, 768))
    if pattern == "quad_edges":      # the last row of a thread's four and the first of the next thread's
        return np.isin(pos % 4, (3, 0))
    density = {"half": 0.5, "thousandth": 1e-3}[pattern]
    return np.random.default_rng(n + len(pattern)).random(n) < density


# ---- grid data ------------------------------------------------------------------------------------------------------
def grid_pool(space):
    """-> query, radius, rows [m, D], their exact distances (float64) [m]: members with distance <= radius and members
    beyond it, both kinds with several distinct distances (one of them exactly on the radius where the space is exact)"""
    if space == "l2sqr_sift":
        rng = np.random.default_rng(7)
        q = rng.integers(0, 256, 128).astype(np.uint8)

        def moved(*steps):           # the query with coordinate j moved by t, away from the nearer end of the range
            r = q.astype(np.int64)
            for j, t in steps:
                r[j] += t if r[j] < 128 else -t
            return r
        rows = [moved((8 * t, t)) for t in range(16)]                    # distances t^2; t <= 10 within the radius 100
        rows += [moved((127, 10), (1, 1)), moved((126, 7), (0, 7), (63, 2))]      # 101 and 102: just beyond it
        rows += [rng.integers(0, 256, 128) for _ in range(6)]
        rows = np.array(rows, np.int64)
        d = ((rows - q.astype(np.int64)) ** 2).sum(1).astype(np.float64)
        assert d.max() < 2 ** 24     # exact as float32
        return q, 100.0, rows.astype(np.uint8), d
    V = np.stack(np.meshgrid(*[np.arange(4)] * 4, indexing="ij"), -1).reshape(-1, 4).astype(np.float64)
    q = np.array([1, 2, 0, 3], np.float64)
    if space == "l1":
        d, radius = np.abs(V - q).sum(1), 2.0
    elif space == "linf":
        d, radius = np.abs(V - q).max(1), 1.0
    elif space == "l2":              # the sums of squares are exact integers m: the radius lies between two of them
        m = ((V - q) ** 2).sum(1)
        d, radius = np.sqrt(m), float(np.sqrt(3 + 0.5))
    elif space == "negdotprod":
        q = np.array([1, 2, 1, 3], np.float64)
        V = V[V @ q > 0]             # (a product of 0 would be reported as -0)
        d, radius = -(V @ q), -13.0
    else:
        raise ValueError(space)
    return q.astype(np.float32), radius, V.astype(np.float32), d


def planted(space, n, mask, seed=0):
    """-> query, radius, rows [n, D], expected distances [n]: row i lies within the radius exactly where mask[i]"""
    q, radius, rows, d = grid_pool(space)
    inside, outside = np.nonzero(d <= radius)[0], np.nonzero(d > radius)[0]
    assert len(inside) >= 4 and len(outside) >= 4 and len(np.unique(d[inside])) >= 2
    rng = np.random.default_rng(1000 + seed)
    member = np.where(mask, inside[rng.integers(0, len(inside), n)], outside[rng.integers(0, len(outside), n)])
    return q, radius, rows[member], d[member]


def capacities(c, n):
    return sorted({cap for cap in (1, c - 1, c, c + 1, n + 5) if cap > 0})


def check_range(idx, q, radius, want_ids, want_d, caps, dist_ok):
    """every capacity: min(c, capacity) results, the expected prefix in insertion order, the distances by dist_ok"""
    c = len(want_ids)
    for cap in caps:
        ids, ds = range_fill_guarded(idx, q, radius, cap)
        m = min(c, cap)
        assert len(ids) == m and len(ds) == m, (cap, len(ids), m)
        np.testing.assert_array_equal(ids, want_ids[:m], err_msg=f"capacity {cap}")
        dist_ok(ds, want_d[:m], cap)


def exact_dists(got, want, cap):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"capacity {cap}")


def close_dists(got, want, cap):
    assert close_rel(got, want), f"capacity {cap}"


def close_dists_range_bar(got, want, cap):
    """the bar of test_range_query_matches_oracle_scan"""
    assert close_rel(got, want, atol=1e-5), f"capacity {cap}"


def check_planted(space, n, pattern, seed=0):
    mask = pattern_mask(pattern, n)
    q, radius, X, d = planted(space, n, mask, seed)
    ext = ext_ids(n)
    idx = make_index(space, "seq_search", X, ext)
    try:
        check_range(idx, q, radius, ext[mask], d[mask], capacities(int(mask.sum()), n),
                    close_dists if space == "l2" else exact_dists)
    finally:
        idx.close()


# ---- 1. selection edges, dense ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("space", ["l1", "l2sqr_sift"])
def test_selection_edges_exact(space, n, pattern):
    check_planted(space, n, pattern)


@pytest.mark.parametrize("n", STARRED)
@pytest.mark.parametrize("space,pattern", [("l2", "block_edges"), ("linf", "half"), ("negdotprod", "quad_edges")])
def test_selection_edges_other_grid_spaces(space, pattern, n):
    check_planted(space, n, pattern, seed=1)


def continuous_case(space, n):
    """-> rows, query, radius, float64 distances: about a dozen rows within the radius, which lies in the middle of the
    widest gap between consecutive distances of ranks 6..30"""
    rng = np.random.default_rng(4000 + n)
    X = rng.standard_normal((n, 8)).astype(np.float32)
    q = rng.standard_normal(8).astype(np.float32)
    x, y = X.astype(np.float64), q.astype(np.float64)
    cos = np.clip((x @ y) / (np.linalg.norm(x, axis=1) * np.linalg.norm(y)), -1.0, 1.0)
    d = np.arccos(cos) if space == "angulardist" else 1.0 - cos
    s = np.sort(d)[6:31]
    g = int(np.argmax(np.diff(s)))
    return X, q, float((s[g] + s[g + 1]) / 2), d


@pytest.mark.parametrize("n", STARRED)
@pytest.mark.parametrize("space", ["cosinesimil", "angulardist"])
def test_selection_edges_continuous(space, n):
    X, q, radius, d = continuous_case(space, n)
    # the existing range test's band around the radius must be empty: no row is excused
    assert not (np.abs(d - radius) <= 1e-5 * max(1.0, abs(radius))).any()
    mask = d <= radius
    assert 7 <= mask.sum() <= 31
    ext = ext_ids(n)
    idx = make_index(space, "seq_search", X, ext)
    try:
        check_range(idx, q, radius, ext[mask], d[mask], capacities(int(mask.sum()), n), close_dists_range_bar)
    finally:
        idx.close()


# ---- 2. the grid-stride branch of the dense distance kernel ---------------------------------------------------------
@pytest.mark.parametrize("space", ["l1", "l2sqr_sift"])
def test_rows_behind_the_distance_grid_get_their_own_distances(space):
    """n = 263 173 > 65 536 workgroups x 4 rows.  A query with about 9 % of the rows within the radius on either side of
    position 262 144 goes first; then one whose only matches are 262 143, 262 144, 262 147 and n - 1, with rows just
    beyond the radius beside them: a row that kept an earlier distance, or none, shows.  f32 rows have D = 5 (ragged)."""
    n = PASS + BLOCK + 5
    rng = np.random.default_rng(21)
    ext = ext_ids(n)
    at = np.array([PASS - 1, PASS, PASS + 3, n - 1])
    beside = np.array([5, PASS - 2, PASS + 1, PASS + 2, n - 2])
    if space == "l1":
        X = rng.integers(1, 4, (n, 5)).astype(np.float32)                  # every coordinate >= 1: 5 or more from 0
        X[at] = [[0, 0, 0, 0, 0], [1, 0, 0, 0, 0], [0, 1, 0, 0, 1], [0, 0, 0, 0, 2]]
        X[beside] = [[0, 0, 0, 0, 3], [1, 1, 0, 0, 1], [0, 0, 0, 0, 3], [2, 0, 0, 0, 1], [0, 0, 1, 1, 1]]   # 3 > 2
        q_many, q_few, r_many, r_few = np.full(5, 3, np.float32), np.zeros(5, np.float32), 2.0, 2.0

        def dist(q):
            return np.abs(X.astype(np.float64) - q).sum(1)
    else:
        q_few, r_few, pool, d = grid_pool(space)
        inside, outside = np.nonzero(d <= r_few)[0], np.nonzero(d > r_few)[0]
        member = outside[rng.integers(0, len(outside), n)]
        member[at] = inside[[0, 3, 7, 10]]
        member[beside] = np.nonzero(d == 101)[0][0]
        X = pool[member]
        q_many, r_many = pool[outside[-1]], 0.0                             # the rows that ARE that pool member

        def dist(q):
            return ((X.astype(np.int32) - q.astype(np.int32)) ** 2).sum(1).astype(np.float64)
    idx = make_index(space, "seq_search", X, ext)
    try:
        d = dist(q_many)
        m = d <= r_many
        assert m[PASS:].sum() >= 20 and m[:PASS].sum() >= 1000
        check_range(idx, q_many, r_many, ext[m], d[m], [n + 5], exact_dists)
        d = dist(q_few)
        m = d <= r_few
        assert np.nonzero(m)[0].tolist() == at.tolist()
        check_range(idx, q_few, r_few, ext[m], d[m], capacities(4, n), exact_dists)
    finally:
        idx.close()


# ---- 3. big-k through the same distance kernel --------------------------------------------------------------------
@pytest.mark.parametrize("space", ["l2", "l2sqr_sift"])
def test_big_k_behind_the_distance_grid(space):
    """k = 513 and k = n + 7 over n = 263 173 rows, 2 queries.  Rows 262 114..262 173 are copies of one row that occurs
    nowhere else and is query 0: among equal distances the position decides, on either side of the grid's end.  The
    expected order is the stable sort of the exact sums of squares."""
    n = PASS + BLOCK + 5
    rng = np.random.default_rng(31)
    dup = np.arange(PASS - 30, PASS + 30)
    if space == "l2":
        X = rng.integers(0, 4, (n, 4)).astype(np.float32)
        X[dup] = [0.5, 1.5, 2.5, 0.5]                 # off the grid; differences are multiples of 0.5: sums stay exact
        Q = np.array([X[dup[0]], [3, 0, 1.5, 2]], np.float32)
        sq = [((X.astype(np.float64) - q) ** 2).sum(1) for q in Q.astype(np.float64)]
    else:
        X = rng.integers(0, 256, (n, 128)).astype(np.uint8)
        X[dup] = X[17] ^ 0x80                         # (no other row is that close to it)
        Q = np.stack([X[dup[0]], rng.integers(0, 256, 128).astype(np.uint8)])
        sq = [((X.astype(np.int32) - q) ** 2).sum(1).astype(np.float64) for q in Q.astype(np.int32)]
    assert (sq[0] == 0).sum() == len(dup)
    order = [np.argsort(s, kind="stable") for s in sq]
    ext = ext_ids(n)
    idx = make_index(space, "seq_search", X, ext)
    try:
        for k in (513, n + 7):
            ids, ds, cnt = idx.knnQueryBatch(Q, k)
            expect_path(idx, 5)
            m = min(k, n)
            assert (cnt == m).all()
            assert ids[0, :len(dup)].tolist() == ext[dup].tolist() and (ds[0, :len(dup)] == 0).all()
            assert ds[0, len(dup)] > 0
            for qi in range(2):
                np.testing.assert_array_equal(ids[qi, :m], ext[order[qi][:m]], err_msg=f"k {k} query {qi}")
                if space == "l2":
                    assert close_rel(ds[qi, :m], np.sqrt(sq[qi][order[qi][:m]]))
                else:
                    np.testing.assert_array_equal(bits(ds[qi, :m]), bits(sq[qi][order[qi][:m]]))
            assert (ids[:, m:] == -1).all() and np.isposinf(ds[:, m:]).all()
    finally:
        idx.close()


# ---- 4. the other families at their own grid caps: pooled rows ---------------------------------------------------
def pool_members(n, seed):
    """row i of the index is pool[member[i]], member[i] = perm[i % 61]"""
    return np.random.default_rng(seed).permutation(POOL)[np.arange(n) % POOL]


def gap_radius(d, tol, lo=6, hi=20):
    """The middle of the widest gap between consecutive sorted distances of ranks lo..hi -> radius; asserts that the
    gap is wider than the tolerance tol(|distance|) on both sides."""
    s = np.sort(np.asarray(d, np.float64))
    g = lo + int(np.argmax(np.diff(s[lo:hi + 1])))
    r = (s[g] + s[g + 1]) / 2
    assert s[g + 1] - r > 2 * tol(abs(s[g + 1])) and r - s[g] > 2 * tol(abs(s[g]))
    return float(r)


def check_pooled(idx, q, radius, member, inside, dist_ok):
    """inside [61]: the pool members with d(member, query) <= radius; dist_ok(distances, members): the reported
    d(query, member) of the results; capacities 1, c, n + 5"""
    n = len(member)
    pos = np.nonzero(inside[member])[0]
    c = len(pos)
    assert n // POOL * 3 <= c <= n - n // POOL * 3
    want_ids = ext_ids(n)[pos]
    for cap in (1, c, n + 5):
        ids, ds = range_fill_guarded(idx, q, radius, cap)
        m = min(c, cap)
        assert len(ids) == m
        np.testing.assert_array_equal(ids, want_ids[:m], err_msg=f"capacity {cap}")
        dist_ok(ds, member[pos[:m]])


def sparse_pool():
    """61 distinct rows of 1-3 elements over 10 ids, and a query of 3 elements"""
    rng = np.random.default_rng(41)
    rows, seen = [], set()
    while len(rows) < POOL:
        ids = np.sort(rng.choice(10, size=int(rng.integers(1, 4)), replace=False)).astype(np.uint32)
        vals = rng.uniform(-2, 2, len(ids)).astype(np.float32)
        key = (tuple(ids.tolist()), tuple(vals.tolist()))
        if key not in seen:
            seen.add(key)
            rows.append((ids, vals))
    return rows, (np.array([1, 4, 7], np.uint32), np.array([0.7, -1.3, 0.9], np.float32))


def sparse_csr(rows, member):
    """the CSR triple of pool rows repeated by `member`, without a Python loop over the 2 million rows"""
    ids = np.zeros((POOL, 3), np.uint32)
    vals = np.zeros((POOL, 3), np.float32)
    lens = np.array([len(r[0]) for r in rows])
    for i, (ri, rv) in enumerate(rows):
        ids[i, :len(ri)], vals[i, :len(ri)] = ri, rv
    used = (np.arange(3)[None, :] < lens[:, None])[member]
    return (np.concatenate([[0], np.cumsum(lens[member])]).astype(np.int64), ids[member][used], vals[member][used])


@pytest.mark.parametrize("space", ["l2_sparse", "negdotprod_sparse"])
def test_sparse_behind_the_distance_grid(space):
    n = CAP_SPARSE + 1030
    rows, q = sparse_pool()
    d_row_q = sparse_ref.scan(space, rows, q)
    d_q_row = sparse_ref.scan(space, rows, q, query_right=False)
    radius = gap_radius(d_row_q, lambda v: 1e-5 * v + 1e-6)        # close_rel, the sparse tests' bar
    member = pool_members(n, 42)
    idx = nz.Index(space, "seq_search", data_type="SparseVector")
    try:
        idx.addSparseBatch(sparse_csr(rows, member), ext_ids(n))
        idx.buildIndex()

        def dist_ok(got, mem):
            assert close_rel(got, d_q_row[mem])
        check_pooled(idx, q, radius, member, d_row_q <= np.float32(radius), dist_ok)
    finally:
        idx.close()


@pytest.mark.parametrize("n", [CAP_SPARSE + 1030, CAP_SPARSE + 1030 - 6])
@pytest.mark.parametrize("space", ["kldivfast", "itakurasaitofast", "jsmetrfast", "kldivgenfastrq"])
def test_divergences_behind_the_distance_grid(space, n):
    """D = 4; rows are stored in groups of 64: the two sizes leave the last group partial in two ways"""
    rng = np.random.default_rng(51)
    pool = rng.uniform(0.05, 1.0, (POOL, 4)).astype(np.float32)
    q = rng.uniform(0.05, 1.0, 4).astype(np.float32)
    d_row_q, b_row_q = diverg_ref.scan(space, pool, q)                       # d(row, query): membership
    d_q_row, s_q_row = diverg_ref.formula(space, q[None, :], pool)           # d(query, row): reported
    b_q_row = diverg_ref.bound(s_q_row, 4)
    if not diverg_ref.is_metr(space):                                        # (Jensen-Shannon is symmetric)
        assert (np.abs(d_row_q - d_q_row) > 4 * (b_row_q + b_q_row)).sum() >= POOL - 3     # a swap of the two shows
    s = np.sort(d_row_q)
    g = 6 + int(np.argmax(np.diff(s[6:21])))
    mid = (s[g] + s[g + 1]) / 2
    radius = float(np.sqrt(mid)) if diverg_ref.is_metr(space) else float(mid)
    rc = float(diverg_ref.comparable(space, np.float32(radius)))
    assert (np.abs(d_row_q - rc) > 2 * b_row_q).all()                        # no pool member within its bound of the radius
    member = pool_members(n, 52)
    idx = nz.Index(space, "seq_search")
    try:
        idx.addDenseBatch(pool[member], ext_ids(n))
        idx.buildIndex()

        def dist_ok(got, mem):
            assert diverg_ref.within(space, got, d_q_row[mem], b_q_row[mem]).all()
        check_pooled(idx, q, radius, member, d_row_q <= rc, dist_ok)
    finally:
        idx.close()


def test_leven_behind_the_distance_grid():
    """n = 4096 x 256 + 300.  A query of 5 symbols (one word) and one of 70 (two words: every thread below 300 runs a
    second row on the slice of the multi-word workspace it has used for its first).  With a radius beyond every distance
    the call reports the distance of every row: the rows of the second sweep must equal their pool members."""
    n = CAP_LEVEN + 300
    rng = np.random.default_rng(61)
    alpha = np.frombuffer(b"acgt", np.uint8)
    pool = set()
    while len(pool) < POOL:
        pool.add(bytes(rng.choice(alpha, size=int(rng.integers(1, 13))).tolist()))
    pool = sorted(pool)
    member = pool_members(n, 62)
    ext = ext_ids(n)
    idx = nz.Index("leven", "seq_search", data_type="ObjectAsString", dist_type="Int")
    try:
        idx.addStringBatch([pool[i] for i in member.tolist()], ids=ext)
        idx.buildIndex()
        for qlen in (5, 70):
            q = bytes(rng.choice(alpha, size=qlen).tolist())
            d = np.array([string_ref.levenshtein(r, q) for r in pool], np.float64)
            assert (d == [string_ref.levenshtein(q, r) for r in pool]).all()
            v = np.sort(d)[12]                                    # an attained distance: rows lie exactly on the radius
            assert (d <= v).sum() < POOL
            check_pooled(idx, q, float(v), member, d <= v,
                         lambda got, mem: np.testing.assert_array_equal(bits(got), bits(d[mem])))
            ids, ds = range_fill_guarded(idx, q, 1000.0, n + 5)    # every row
            np.testing.assert_array_equal(ids, ext)
            np.testing.assert_array_equal(bits(ds[CAP_LEVEN:]), bits(d[member[CAP_LEVEN:]]), err_msg="second sweep")
            np.testing.assert_array_equal(bits(ds), bits(d[member]))
    finally:
        idx.close()


# ---- 5. behind deletes, consolidate and shards ----------------------------------------------------------------------
def same_as(idx, other, q, radius, caps):
    """the two indexes answer alike, bit for bit -> the answers"""
    out = []
    for cap in caps:
        a, b = range_fill_guarded(idx, q, radius, cap), range_fill_guarded(other, q, radius, cap)
        np.testing.assert_array_equal(a[0], b[0], err_msg=f"capacity {cap}")
        np.testing.assert_array_equal(bits(a[1]), bits(b[1]), err_msg=f"capacity {cap}")
        out.append(a)
    return out


def test_delete_down_to_one_block_and_consolidate():
    """2049 rows; deletes leave 1025, then 1024, then 1023 live rows (positions 1023 and 1024 among the deleted): each
    time the answers are those of an index built from the live rows alone, and the planted ones; then consolidate()."""
    n = 2049
    mask = pattern_mask("half", n)
    mask[[0, 1022, 1023, 1024, 1025, n - 1]] = True
    q, radius, X, d = planted("l1", n, mask, seed=5)
    ext = ext_ids(n)
    idx = make_index("l1", "seq_search", X, ext)
    live = np.ones(n, bool)
    rng = np.random.default_rng(71)
    first = np.r_[1023, rng.permutation(np.setdiff1d(np.arange(1, n - 1), [1022, 1023, 1024, 1025]))[:1023]]

    def check():
        want = live & mask
        caps = capacities(int(want.sum()), int(live.sum()))
        oracle = make_index("l1", "seq_search", X[live], ext[live])
        try:
            same_as(idx, oracle, q, radius, caps)
        finally:
            oracle.close()
        check_range(idx, q, radius, ext[want], d[want], caps, exact_dists)

    try:
        check()                                                       # (resident and prepared with all rows first)
        for dead, left in ((first, 1025), ([1024], 1024), ([1025], 1023)):
            assert idx.deleteIds(ext[dead]) == len(dead)
            live[dead] = False
            assert live.sum() == left
            check()
        assert idx.consolidate()[0] == n - 1023 and idx.dataQty() == 1023
        check()
    finally:
        idx.close()


@pytest.mark.parametrize("case", ["last_shard_only", "capacity_ends_shard_0", "missing_match_in_shard_2"])
def test_three_shards(case):
    """3075 rows in 3 shards of 1025: the shards are asked in turn, each for what the capacity still lacks"""
    n = 3075
    rng = np.random.default_rng(81)
    mask = rng.random(n) < 0.125
    mask[[1024, 1025, 2049, 2050, n - 1]] = True
    if case == "last_shard_only":
        mask[:2050] = False
        caps = capacities(int(mask.sum()), n)
    elif case == "capacity_ends_shard_0":                 # the capacity is full with the last row of shard 0
        caps = [int(mask[:1025].sum()), int(mask[:1025].sum()) + 1]
    else:
        mask[2050:n - 1] = False                          # the one match capacity c - 1 leaves out is the last row
        mask[2050] = True
        caps = [int(mask.sum()) - 1, int(mask.sum()) - 2, int(mask.sum())]
    q, radius, X, d = planted("l1", n, mask, seed=6)
    ext = ext_ids(n)
    one = make_index("l1", "seq_search", X, ext, gpu_shards=1)
    many = make_index("l1", "seq_search", X, ext, gpu_shards=3)
    try:
        assert many.stats()["shards"] == 3 and one.stats()["shards"] == 1
        same_as(many, one, q, radius, caps)
        check_range(many, q, radius, ext[mask], d[mask], caps, exact_dists)
    finally:
        one.close()
        many.close()


# ---- 6. a declared capacity far beyond the rows ---------------------------------------------------------------------
def test_declared_capacity_beyond_the_rows_asks_for_no_memory():
    """Result.capacity = 2^40 over 1000 rows (the buffers hold 1000 + the sentinels): the 10 matches come back, and the
    index holds no more memory than a row count's worth of workspace on top of what it held"""
    n = 1000
    mask = np.zeros(n, bool)
    mask[np.random.default_rng(91).permutation(n)[:10]] = True
    q, radius, X, d = planted("l1", n, mask, seed=7)
    ext = ext_ids(n)
    idx = make_index("l1", "seq_search", X, ext)
    try:
        before = nz.lib().nmslib_index_memory_usage(idx.h)
        ids, ds = range_fill_guarded(idx, q, radius, n, declared=1 << 40)
        np.testing.assert_array_equal(ids, ext[mask])
        exact_dists(ds, d[mask], n)
        after = nz.lib().nmslib_index_memory_usage(idx.h)
        assert after - before <= 2 * 4 * n, (before, after)
        check_range(idx, q, radius, ext[mask], d[mask], capacities(10, n), exact_dists)     # and the index still serves
    finally:
        idx.close()
