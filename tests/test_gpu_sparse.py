"""-m gpu: exact k-NN, range search and get_distance over sparse vectors against the reference's outputs
(tests/golden/golden_sparse.npz) and the expected-distance helper (tests/sparse_ref.py)."""
import ctypes as C

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import sparse_ref
from tests.golden import gen_golden_sparse as gs
from tests.gpuutil import close_rel
from tests.test_sparse_cpu import GOLDEN

pytestmark = pytest.mark.gpu

HELPER_SPACES = sparse_ref.SPACES  # incl. querynorm_negdotprod_sparse, which the reference's C ABI does not serve


@pytest.fixture(scope="module")
def gsp():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def sparse_index(space, rows, space_params=None, ids=None, **index_params):
    idx = nz.Index(space, "seq_search", data_type="SparseVector", space_params=space_params)
    idx.addSparseBatch(rows, ids)
    idx.buildIndex(**index_params)
    return idx


def zipf_set(seed, n, mean_len, vocab=1 << 20):
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.poisson(mean_len, size=n), 1, None)
    return [gs.zipf_row(rng, int(m), vocab) for m in lens]


@pytest.mark.parametrize("tag,space,sp", gs.SPACES)
def test_knn_matches_reference(gsp, tag, space, sp):
    rows, qs, _ = gs.inputs_main()
    idx = sparse_index(space, rows, sp)
    for k in (10, 100):
        ids, ds, cnt = idx.knnQueryBatch(qs, k)
        np.testing.assert_array_equal(ids, gsp[f"{tag}_k{k}_ids"], err_msg=f"{tag} k={k}")
        np.testing.assert_array_equal(cnt, gsp[f"{tag}_k{k}_cnt"])
        assert close_rel(ds, gsp[f"{tag}_k{k}_dists"])
    idx.close()
    tr, tq = gs.inputs_ties()                      # integer values: exact distances, heavy ties
    idx = sparse_index(space, tr, sp)
    ids, ds, cnt = idx.knnQueryBatch(tq, 10)
    np.testing.assert_array_equal(ids, gsp[f"{tag}_ties_ids"])
    if "angular" in space or "cosine" in space:
        assert close_rel(ds, gsp[f"{tag}_ties_dists"])
    else:
        np.testing.assert_array_equal(ds, gsp[f"{tag}_ties_dists"])
    idx.close()
    yr, yq = gs.inputs_tiny()                      # k = 10 > n = 7
    idx = sparse_index(space, yr, sp)
    ids, ds, cnt = idx.knnQueryBatch(yq, 10)
    np.testing.assert_array_equal(ids, gsp[f"{tag}_tiny_ids"])
    np.testing.assert_array_equal(cnt, gsp[f"{tag}_tiny_cnt"])
    assert close_rel(ds[:, :7], gsp[f"{tag}_tiny_dists"][:, :7]) and np.isinf(ds[:, 7:]).all()
    idx.close()


def range_same_up_to_radius_rows(gi, gd, wi, wd, r):
    """equal, or the first difference is a row on the radius (its distance within 1e-5 relative of it)"""
    if len(gi) == len(wi) and (gi == wi).all():
        return True
    n = min(len(gi), len(wi))
    j = next((t for t in range(n) if gi[t] != wi[t]), n)
    at = [d for d, lst in ((wd, wi), (gd, gi)) for d in ([d[j]] if j < len(lst) else [])]
    return any(abs(float(d) - r) <= 1e-5 * abs(r) + 1e-6 for d in at)


@pytest.mark.parametrize("tag,space,sp", gs.SPACES)
def test_range_and_get_distance_match_reference(gsp, tag, space, sp):
    """The radii are reference distances, so a row lies exactly on each one.  The L1 / L2 / L-inf / dot formulas are
    the reference's bit for bit: same rows.  Angular goes through the device acosf, a few ulp from glibc's: a row on
    the radius may fall on either side (range query)."""
    rows, qs, pairs = gs.inputs_main()
    idx = sparse_index(space, rows, sp)
    radii = gsp[f"{tag}_radii"]
    for cap in gs.RANGE_CAPS:
        want_n = gsp[f"{tag}_range{cap}_n"]
        off = np.concatenate([[0], np.cumsum(want_n)])
        want_i, want_d = gsp[f"{tag}_range{cap}_ids"], gsp[f"{tag}_range{cap}_dists"]
        c = 0
        for qi, q in enumerate(qs):
            for r in radii[qi]:
                a, b = idx.rangeQueryFill(q, r, cap)
                wi, wd = want_i[off[c]:off[c + 1]], want_d[off[c]:off[c + 1]]
                if "angular" in space:
                    assert range_same_up_to_radius_rows(a, b, wi, wd, float(r)), (qi, r)
                else:
                    np.testing.assert_array_equal(a, wi, err_msg=f"query {qi} radius {r}")
                m = min(len(a), len(wi))
                assert close_rel(b[:m][a[:m] == wi[:m]], wd[:m][a[:m] == wi[:m]])
                c += 1
    got = np.array([idx.getDistance(int(a), int(b)) for a, b in pairs], np.float32)
    assert close_rel(got, gsp[f"{tag}_pair_dists"])
    idx.close()


def ids_match_within_ties(got_i, got_d, want_i, want_d):
    """ids equal wherever the distance is unique; inside a group of equal expected distances the same set (a group
    cut by k may hold other members of the group)"""
    for q in range(want_i.shape[0]):
        for v in np.unique(want_d[q]):
            m = want_d[q] == v
            if m.sum() == 1 and v != want_d[q][-1]:
                if got_i[q][m][0] != want_i[q][m][0]:
                    return False
            elif v != want_d[q][-1] and set(got_i[q][m].tolist()) != set(want_i[q][m].tolist()):
                return False
    return True


@pytest.mark.parametrize("space", HELPER_SPACES)
def test_larger_zipf_set_against_helper(space):
    """20 000 Zipf rows (mean 64 elements) over a 2^20 vocabulary, 24 queries (mean 32): the helper's exact scan.
    Smaller than a 50 000 x 300 run on purpose: the numpy helper merges every (row, query) pair on the host, about
    0.3 s per query at this size, and this test runs for all seven spaces.  Ids are compared exactly where the
    expected distances are distinct and as sets inside groups of equal distances; the tie ORDER is pinned by the
    reference fixture (test_knn_matches_reference, the integer-valued tie set)."""
    rows = zipf_set(1, 20000, 64)
    qs = zipf_set(2, 24, 32)
    idx = sparse_index(space, rows)
    ids, ds, cnt = idx.knnQueryBatch(qs, 10)
    pos, dist = sparse_ref.seq_search(space, rows, qs, 10)
    assert close_rel(ds, dist)
    assert ids_match_within_ties(ids, ds, pos, dist)
    exact = np.array([len(np.unique(d)) == 10 for d in dist])
    assert (ids[exact] == pos[exact]).all()
    idx.close()


def test_fill_equals_batch_row_and_mixed_lengths():
    rows = zipf_set(3, 3000, 40, vocab=5000)
    rng = np.random.default_rng(4)
    qs = [gs.zipf_row(rng, m, 5000) for m in (1, 3, 700, 2, 64, 4000, 1, 17)]
    idx = sparse_index("cosinesimil_sparse", rows)
    ids, ds, cnt = idx.knnQueryBatch(qs, 12)
    for i, q in enumerate(qs):
        a, b = idx.knnQuery(q, 12)
        np.testing.assert_array_equal(a, ids[i])
        np.testing.assert_array_equal(b, ds[i])
    pos, dist = sparse_ref.seq_search("cosinesimil_sparse", rows, qs, 12)
    assert close_rel(ds, dist) and ids_match_within_ties(ids, ds, pos, dist)
    idx.close()


@pytest.mark.parametrize("space", ["l2_sparse", "negdotprod_sparse", "angulardist_sparse"])
def test_long_lists_beyond_one_lds_tile(space):
    """queries longer than the LDS tile (4096 elements) are read from HBM; rows of thousands of elements"""
    rng = np.random.default_rng(9)
    rows = [gs.uniform_row(rng, int(m), 0, 60000) for m in rng.integers(1, 9000, size=120)]
    qs = [gs.uniform_row(rng, int(m), 0, 60000) for m in (5000, 9000, 30000, 4096, 4097)]
    idx = sparse_index(space, rows)
    ids, ds, cnt = idx.knnQueryBatch(qs, 15)
    pos, dist = sparse_ref.seq_search(space, rows, qs, 15)
    assert close_rel(ds, dist) and ids_match_within_ties(ids, ds, pos, dist)
    radius = (float(dist[2, 5]) + float(dist[2, 6])) / 2     # between two distances: no boundary row
    r_i, r_d = idx.rangeQueryFill(qs[2], radius, 50)
    want = np.where(sparse_ref.scan(space, rows, qs[2]) <= np.float32(radius))[0][:50]
    np.testing.assert_array_equal(r_i, want)
    idx.close()


@pytest.mark.parametrize("space,n,k", [("l2_sparse", 3000, 1000), ("cosinesimil_sparse", 3000, 1000),
                                       ("l2_sparse", 6000, 5000), ("negdotprod_sparse", 6000, 5000)])
def test_large_k_plans(space, n, k):
    """k = 1000: key buffers too large for a query tile, one query per workgroup (TQ = 1); k = 5000 > 4096: a split
    holds at most 4096 rows and keeps all of them, and the split lists (nsplit * k > 8192) merge through the
    bisection kernel instead of the LDS sort"""
    rows = zipf_set(11, n, 20, vocab=3000)
    qs = zipf_set(12, 5, 15, vocab=3000)
    idx = sparse_index(space, rows)
    ids, ds, cnt = idx.knnQueryBatch(qs, k)
    pos, dist = sparse_ref.seq_search(space, rows, qs, k)
    assert (cnt == min(k, n)).all()
    assert close_rel(ds, dist)
    assert ids_match_within_ties(ids, ds, pos, dist)
    idx.close()


def test_batch_above_the_query_slice():
    """33 000 queries (one slice holds 32 768) on a small index: the second slice lands at its own offset"""
    rows = zipf_set(5, 50, 6, vocab=200)
    rng = np.random.default_rng(6)
    qs = [gs.zipf_row(rng, int(m), 200) for m in rng.integers(1, 6, size=33000)]
    idx = sparse_index("l1_sparse", rows, ids=np.arange(50, dtype=np.int32) + 1000)
    ids, ds, cnt = idx.knnQueryBatch(qs, 5)
    assert (cnt == 5).all()
    pick = [0, 1, 32767, 32768, 32769, 32999]
    pos, dist = sparse_ref.seq_search("l1_sparse", rows, [qs[i] for i in pick], 5)
    np.testing.assert_array_equal(ds[pick], dist)
    np.testing.assert_array_equal(ids[pick], pos + 1000)        # exact distances: (distance, position) order
    idx.close()


def test_determinism_and_memory_usage():
    rows = zipf_set(7, 5000, 30, vocab=20000)
    qs = zipf_set(8, 64, 20, vocab=20000)
    idx = nz.Index("angulardist_sparse", "brute_force", data_type="SparseVector")
    idx.addSparseBatch(rows)
    idx.buildIndex(gpu_defer=1)
    before = nz.lib().nmslib_index_memory_usage(idx.h)
    idx.finalize()
    after = nz.lib().nmslib_index_memory_usage(idx.h)
    nnz = sum(len(r[0]) for r in rows)
    assert after - before >= nnz * 8 + (len(rows) + 1) * 8
    assert idx.stats()["hbm_bytes"] >= nnz * 8
    a = idx.knnQueryBatch(qs, 25)
    b = idx.knnQueryBatch(qs, 25)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    idx.close()


def test_querynorm_argument_order():
    """-QueryNormScalarProduct(p1, p2) normalises by the SECOND argument: k-NN distances are normalised by the query
    (IndexTimeDistance(row, query)), get_distance(a, b) by row b."""
    rows = [([1, 2], [3.0, 4.0]), ([1, 2], [30.0, 40.0]), ([2, 9], [1.0, 1.0])]
    idx = sparse_index("querynorm_negdotprod_sparse", rows)
    ids, ds = idx.knnQuery(([1, 2], [1.0, 0.0]), 3)
    np.testing.assert_array_equal(ids, [1, 0, 2])
    assert close_rel(ds, [-30.0, -3.0, 0.0])
    assert close_rel([idx.getDistance(0, 1)], [-(3 * 30 + 4 * 40) / 50.0])
    assert close_rel([idx.getDistance(1, 0)], [-(3 * 30 + 4 * 40) / 5.0])
    idx.close()


def test_device_batch_entry_refuses_sparse_queries():
    idx = sparse_index("l2_sparse", [([1], [1.0])])
    d = C.c_void_p(1)
    rc = nz.lib().nmslib_gpu_knn_query_batch_device(idx.h, d, 1, 2, 1, d, d, None, None)
    assert rc == 5
    idx.close()
