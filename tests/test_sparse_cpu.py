"""Sparse vectors without a GPU: the fixture against the compiled reference, the expected-distance helper against the
fixture, and the host logic of the C ABI over a sparse index (element rules, data types, stored data, allocator)."""
import ctypes as C
import os

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import orc, sparse_ref
from tests.golden import gen_golden_sparse as gs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_sparse.npz")
SPARSE_NAMES = ("cosinesimil_sparse", "angulardist_sparse", "negdotprod_sparse", "querynorm_negdotprod_sparse",
                "l1_sparse", "l2_sparse", "linf_sparse")


@pytest.fixture(scope="module")
def gsp():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    rows, qs, pairs = gs.inputs_main()
    assert np.array_equal(gs.sha(rows), d["main_rows_sha"]) and np.array_equal(gs.sha(qs), d["main_queries_sha"])
    assert np.array_equal(pairs, d["main_pairs"])
    tr, tq = gs.inputs_ties()
    assert np.array_equal(gs.sha(tr), d["ties_rows_sha"]) and np.array_equal(gs.sha(tq), d["ties_queries_sha"])
    return d


def helper_name(space, sp):
    return sparse_ref.LP[sp["p"]] if sp else space


@pytest.mark.skipif(not os.path.exists(orc.REF_LIB), reason="oracle/_ref not built (make -C oracle ref)")
def test_fixture_equals_live_reference(gsp):
    live = gs.run_reference()
    assert sorted(live) == sorted(gsp)
    for key in live:
        np.testing.assert_array_equal(live[key], gsp[key], err_msg=key)


@pytest.mark.parametrize("tag,space,sp", gs.SPACES)
def test_helper_distances_equal_fixture_bits(gsp, tag, space, sp):
    """Every distance the reference reported (k-NN at k=100, get_distance pairs, tie set) recomputed by the helper
    for the same (row, query) pair, bit for bit."""
    name = helper_name(space, sp)
    rows, qs, pairs = gs.inputs_main()
    R = sparse_ref.csr(rows)
    ids, dists = gsp[f"{tag}_k100_ids"], gsp[f"{tag}_k100_dists"]
    for qi, q in enumerate(qs):
        d = sparse_ref.scan(name, R, q)
        np.testing.assert_array_equal(d[ids[qi]], dists[qi], err_msg=f"{tag} query {qi}")
    got = np.array([sparse_ref.distance(name, rows[a], rows[b]) for a, b in pairs], np.float32)
    np.testing.assert_array_equal(got, gsp[f"{tag}_pair_dists"])
    tr, tq = gs.inputs_ties()
    _, td = sparse_ref.seq_search(name, tr, tq, 10)
    np.testing.assert_array_equal(td, gsp[f"{tag}_ties_dists"])


def test_helper_l1_linf_agree_with_the_oracle_formula():
    rows, qs, _ = gs.inputs_main()
    for space in ("l1_sparse", "linf_sparse"):
        for r in rows[:40]:
            assert sparse_ref.distance(space, r, qs[0]) == sparse_ref.distance_oracle(space, r, qs[0])


# ---- C-ABI host logic -----------------------------------------------------------------------------------------------
def elems(ids, vals):
    return nz.sparse_vector(np.asarray(ids, np.uint32), np.asarray(vals, np.float32))


def create(space, method="seq_search", data_type=1, space_params=None):
    L = nz.lib()
    a = nz.TrackingAllocator()
    h = C.c_void_p()
    sp = nz.Params(a, **space_params) if space_params else None
    rc = L.nmslib_index_create(space.encode(), sp.h if sp else None, method.encode(), data_type, 0, a.ref(), C.byref(h))
    if sp:
        sp.free()
    return rc, h, a


@pytest.mark.parametrize("space", SPARSE_NAMES)
@pytest.mark.parametrize("method", ["seq_search", "brute_force"])
def test_sparse_spaces_are_created(space, method):
    rc, h, a = create(space, method)
    assert rc == 0
    nz.lib().nmslib_index_destroy(h)
    assert len(a.live) == 0


@pytest.mark.parametrize("p", [1.0, 2.0, -1.0])
def test_lp_sparse_p_served(p):
    rc, h, a = create("lp_sparse", space_params={"p": p})
    assert rc == 0
    nz.lib().nmslib_index_destroy(h)


@pytest.mark.parametrize("space,method,params", [
    ("cosinesimil_sparse_fast", "seq_search", None), ("negdotprod_sparse_fast", "seq_search", None),
    ("cosinesimil_sparse_bin_fast", "seq_search", None), ("jaccard_sparse", "seq_search", None),
    ("sparse_dense_fusion", "seq_search", None), ("lp_sparse", "seq_search", {"p": 3.0}),
    ("lp_sparse", "seq_search", None), ("l2", "seq_search", None),
    ("cosinesimil_sparse", "hnsw", None), ("l2_sparse", "hnsw", None), ("negdotprod_sparse", "hnsw", None)])
def test_unserved_sparse_configurations_are_space_incompatible(space, method, params):
    rc, h, a = create(space, method, space_params=params)
    assert rc == 5
    msg = nz.last_error_detail(a)
    assert msg
    assert len(a.live) == 0


def test_lp_sparse_p3_message_names_p():
    rc, h, a = create("lp_sparse", space_params={"p": 3.0})
    assert rc == 5 and "p = 1, 2 and -1" in nz.last_error_detail(a)


def test_sparse_space_with_dense_data_type_is_refused():
    rc, h, a = create("l2_sparse", data_type=0)
    assert rc == 5


def test_element_rules_and_data_modes():
    L = nz.lib()
    rc, h, a = create("cosinesimil_sparse")
    assert rc == 0
    good = elems([1, 5, 9], [1, 2, 3])
    unsorted = elems([5, 1], [1, 2])
    dup = elems([3, 3], [1, 2])
    for bad in (unsorted, dup):
        assert L.nmslib_add_data_point(h, bad.ctypes.data, len(bad), 0) == 7
        assert "Invalid sparse elements" in nz.last_error_detail(a)
    assert L.nmslib_add_data_point_batch(h, unsorted.ctypes.data, 1, 2, None, np.array([2], np.uint64).ctypes.data) == 7
    assert L.nmslib_add_data_point_batch(h, good.ctypes.data, 1, 3, None, np.array([0], np.uint64).ctypes.data) == 7
    ptrs = (C.c_void_p * 1)(dup.ctypes.data)
    assert L.nmslib_add_data_point_batch_pointers(h, 1, ptrs, 1, 2, None, np.array([2], np.uint64).ctypes.data) == 7
    assert L.nmslib_data_qty(h) == 0                      # nothing of a refused batch is stored
    # dense / uint8 data into a sparse index
    X = np.ones((2, 4), np.float32)
    dptrs = (C.c_void_p * 2)(X[0].ctypes.data, X[1].ctypes.data)
    assert L.nmslib_add_data_point_batch_pointers(h, 0, dptrs, 2, 4, None, None) == 5
    assert L.nmslib_add_data_point_batch_pointers(h, 2, dptrs, 2, 4, None, None) == 5
    U = np.ones((2, 128), np.uint8)
    assert L.nmslib_add_data_point_batch_uint8(h, U.ctypes.data, 2, 128, None) == 5
    # valid rows through all three entries
    assert L.nmslib_add_data_point(h, good.ctypes.data, len(good), 100) == 0
    el, counts = nz.sparse_rows([([2, 4], [1.5, -2.0]), ([7], [0.25])])
    ids = np.array([101, 102], np.int32)
    assert L.nmslib_add_data_point_batch(h, el.ctypes.data, 2, 2, ids.ctypes.data, counts.ctypes.data) == 0
    r = elems([0, 1, 2, 3], [4, 3, 2, 1])
    ptrs = (C.c_void_p * 1)(r.ctypes.data)
    four, rid = np.array([4], np.uint64), np.array([103], np.int32)
    assert L.nmslib_add_data_point_batch_pointers(h, 1, ptrs, 1, 4, rid.ctypes.data, four.ctypes.data) == 0
    assert L.nmslib_data_qty(h) == 4
    L.nmslib_index_destroy(h)
    assert len(a.live) == 0


def test_sparse_pointer_batch_into_dense_index_stays_refused():
    L = nz.lib()
    rc, h, a = create("l2", data_type=0)
    assert rc == 0
    e = elems([1, 2], [1, 1])
    ptrs = (C.c_void_p * 1)(e.ctypes.data)
    assert L.nmslib_add_data_point_batch_pointers(h, 1, ptrs, 1, 2, None, np.array([2], np.uint64).ctypes.data) == 5
    L.nmslib_index_destroy(h)


def test_stored_rows_borrow_and_metadata():
    L = nz.lib()
    idx = nz.Index("l2_sparse", "seq_search", data_type="SparseVector")
    rows = [(np.array([3, 8, 20], np.uint32), np.array([1, -2, 0.5], np.float32)),
            (np.array([1], np.uint32), np.array([7], np.float32)),
            (np.array([0, 1, 2, 3, 4], np.uint32), np.arange(5, dtype=np.float32))]
    idx.addSparseBatch(rows, ids=[10, 11, 12])
    indptr = np.array([0, 2, 3], np.int64)
    idx.addSparseBatch((indptr, np.array([5, 6, 9], np.uint32), np.array([1, 2, 3], np.float32)))  # CSR triple
    assert idx.dataQty() == 5
    for i, (ids, vals) in enumerate(rows):
        gi, gv = idx.getDataPoint(i)
        np.testing.assert_array_equal(gi, ids)
        np.testing.assert_array_equal(gv, vals)
    gi, gv = idx.getDataPoint(3)
    np.testing.assert_array_equal(gi, [5, 6])
    n = C.c_size_t()
    assert L.nmslib_get_data_point_size(idx.h, 0, C.byref(n)) == 0 and n.value == 3 * 8
    small = np.empty(8, np.uint8)
    assert L.nmslib_get_data_point_fill(idx.h, 0, small.ctypes.data, 8) == 4
    p, sz, fn = C.c_void_p(), C.c_size_t(), C.c_void_p()
    assert L.nmslib_borrow_data_sparse(idx.h, 2, C.byref(p), C.byref(sz), C.byref(fn)) == 0
    assert sz.value == 5                                             # elements, nmslib_c.cpp:1339-1340
    got = np.frombuffer(C.string_at(p, sz.value * 8), nz.SPARSE_ELEM)
    np.testing.assert_array_equal(got["id"], rows[2][0])
    np.testing.assert_array_equal(got["value"], rows[2][1])
    C.CFUNCTYPE(None, C.c_void_p)(fn.value)(p)
    assert L.nmslib_borrow_data_dense(idx.h, 0, C.byref(p), C.byref(sz), C.byref(fn)) == 5
    assert L.nmslib_borrow_data_sparse(idx.h, 9, C.byref(p), C.byref(sz), C.byref(fn)) == 2
    assert idx.getSpaceType() == "l2_sparse" and idx.getMethod() == "seq_search"
    assert nz.lib().nmslib_index_memory_usage(idx.h) == 0            # not created yet
    idx.close()
    assert len(idx.alloc.live) == 0


def test_dense_borrow_sparse_on_dense_index_still_refused():
    idx = nz.Index("l2", "seq_search")
    idx.addDenseBatch(np.eye(4, dtype=np.float32))
    p, sz, fn = C.c_void_p(), C.c_size_t(), C.c_void_p()
    assert nz.lib().nmslib_borrow_data_sparse(idx.h, 0, C.byref(p), C.byref(sz), C.byref(fn)) == 5
    idx.close()


def test_gpu_shards_rejected_on_a_sparse_index():
    idx = nz.Index("cosinesimil_sparse", "brute_force", data_type="SparseVector")
    with pytest.raises(nz.NmslibError) as e:
        idx.buildIndex(gpu_shards=2)
    assert e.value.code == 8 and "one GPU" in str(e.value)
    idx.close()


def test_empty_sparse_query_is_invalid_sparse_element():
    """Checked before any device work: an empty or unsorted query is refused the same way without a GPU."""
    L = nz.lib()
    idx = nz.Index("l2_sparse", "seq_search", data_type="SparseVector")
    idx.buildIndex(gpu_defer=1)                     # created, nothing to upload
    q = elems([4, 2], [1, 1])
    ids, ds = (C.c_int32 * 4)(), (C.c_float * 4)()
    r = nz.Result(ids, ds, 0, 4)
    assert L.nmslib_knn_query_fill(idx.h, q.ctypes.data, 4, 2, C.byref(r), 2) == 7
    assert L.nmslib_knn_query_fill(idx.h, q.ctypes.data, 4, 2, C.byref(r), 0) == 7
    assert L.nmslib_range_query_fill(idx.h, q.ctypes.data, 4, 1.0, C.byref(r), 2) == 7
    idx.close()


def test_save_sparse_index_is_data_io_failed(tmp_path):
    idx = nz.Index("l1_sparse", "seq_search", data_type="SparseVector")
    idx.addSparseBatch([([1, 2], [1, 1])])
    idx.buildIndex(gpu_defer=1)
    with pytest.raises(nz.NmslibError) as e:
        idx.save(str(tmp_path / "sp"))
    assert e.value.code == 10
    assert not os.path.exists(str(tmp_path / "sp.dat"))
    idx.close()
