"""No GPU: nmslib_gpu_delete_ids / nmslib_gpu_deleted_rows through the C ABI on indexes whose upload is deferred
(gpu_defer=1): the arithmetic of `marked`, what keeps being served by position, what a save answers, and the indexes
that are refused."""
import ctypes as C
import os

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests.gpuutil import make_index

X = np.random.default_rng(11).standard_normal((60, 12)).astype(np.float32)
HNSW = dict(M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1)
NULL_POINTER, SPACE_INCOMPATIBLE, DATA_IO_FAILED = 1, 5, 10


def test_both_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(nz.__file__), "..", "include", "nmslib_gpu.h")).read()
    for name in ("nmslib_gpu_delete_ids", "nmslib_gpu_deleted_rows"):
        assert name in header and name in nz.ABI_SYMBOLS_GPU
        assert getattr(nz.lib(), name) is not None
    assert callable(nz.Index.deleteIds) and callable(nz.Index.deletedRows)


@pytest.mark.parametrize("method,params", [("hnsw", HNSW), ("brute_force", dict(gpu_defer=1)),
                                           ("seq_search", dict(gpu_defer=1))])
def test_marked_arithmetic_before_and_after_build(method, params):
    ids = np.arange(60, dtype=np.int32)
    ids[[7, 20, 41]] = 1000                                      # one id carried by three rows
    idx = nz.Index("l2", method)
    idx.addDenseBatch(X, ids)
    assert idx.deletedRows() == 0
    assert idx.deleteIds([5]) == 1                               # before nmslib_create_index
    assert idx.deletedRows() == 1
    idx.buildIndex(**params)
    assert idx.deletedRows() == 1                                # create_index keeps the tombstones
    assert idx.deleteIds([123456]) == 0                          # no row carries it
    assert idx.deleteIds([9, 9, 9]) == 1                         # listed three times
    assert idx.deletedRows() == 2
    assert idx.deleteIds([1000]) == 3                            # three rows
    assert idx.deletedRows() == 5
    assert idx.deleteIds([1000, 5, 9]) == 0                      # marked already
    assert idx.deleteIds([5, 6, 777]) == 1
    assert idx.deletedRows() == 6
    assert idx.deleteIds([]) == 0 and idx.deleteIds(np.empty(0, np.int32)) == 0
    assert idx.deletedRows() == 6
    idx.buildIndex(**params)                                     # again: still there
    assert idx.deletedRows() == 6
    idx.close()


def test_a_deleted_position_is_still_served_by_position():
    idx = make_index("l2", "hnsw", X, **HNSW)
    assert idx.deleteIds([3, 17]) == 2
    assert idx.dataQty() == 60
    np.testing.assert_array_equal(idx.getDataPoint(3), X[3])
    np.testing.assert_array_equal(idx.getDataPoint(17), X[17])
    p, sz, fn = C.c_void_p(), C.c_size_t(), C.c_void_p()
    assert nz.lib().nmslib_borrow_data_dense(idx.h, 3, C.byref(p), C.byref(sz), C.byref(fn)) == 0
    np.testing.assert_array_equal(np.frombuffer(C.string_at(p, 48), np.float32), X[3])
    try:                                                         # (nmslib_get_distance runs on the device: served there,
        want = np.float32(np.sqrt(np.sum((X[3].astype(np.float64) - X[17]) ** 2)))   # and never refused for the tombstone)
        assert abs(idx.getDistance(3, 17) - want) <= 1e-5 * want
    except nz.NmslibError as e:
        assert "no HIP device" in str(e), e
    idx.close()


def test_a_row_added_under_a_deleted_id_is_live_and_reset_clears():
    idx = make_index("l2", "hnsw", X, **HNSW)
    assert idx.deleteIds([10, 11]) == 2
    idx.addDenseBatch(X[:3] + 1, np.array([10, 11, 12], np.int32))
    assert idx.deletedRows() == 2 and idx.dataQty() == 63
    assert idx.deleteIds([10]) == 1                              # the new row: position 60, the old one is marked already
    assert idx.deletedRows() == 3
    assert idx.deleteIds([12]) == 2                              # an old row and a new one
    idx.reset()
    assert idx.deletedRows() == 0 and idx.dataQty() == 0
    idx.addDenseBatch(X)
    idx.buildIndex(**HNSW)
    assert idx.deletedRows() == 0
    assert idx.deleteIds([10]) == 1
    idx.close()


@pytest.mark.parametrize("method", ["hnsw", "brute_force"])
def test_save_with_tombstones_writes_nothing(method, tmp_path):
    idx = make_index("l2", method, X, **(HNSW if method == "hnsw" else dict(gpu_defer=1)))
    assert idx.deleteIds([4]) == 1
    path = str(tmp_path / "deleted.idx")
    with pytest.raises(nz.NmslibError) as ei:
        idx.save(path, save_data=True)
    assert ei.value.code == DATA_IO_FAILED, ei.value
    assert "deleted rows" in str(ei.value) and "file format" in str(ei.value), ei.value
    assert not os.path.exists(path) and not os.path.exists(path + ".dat")
    idx.close()
    if method == "hnsw":                                         # without a tombstone the same index is saved
        ok = make_index("l2", method, X, **HNSW)
        assert ok.deleteIds([99999]) == 0
        ok.save(path, save_data=True)
        assert os.path.exists(path) and os.path.exists(path + ".dat")
        ok.close()


def test_null_arguments_and_an_empty_list():
    L = nz.lib()
    idx = make_index("l2", "hnsw", X, **HNSW)
    m = C.c_size_t(77)
    assert L.nmslib_gpu_delete_ids(idx.h, None, 3, C.byref(m)) == NULL_POINTER and m.value == 0
    assert L.nmslib_gpu_delete_ids(None, None, 0, C.byref(m)) == NULL_POINTER
    one = np.array([1], np.int32)
    assert L.nmslib_gpu_delete_ids(None, one.ctypes.data, 1, None) == NULL_POINTER
    assert L.nmslib_gpu_deleted_rows(None, C.byref(m)) == NULL_POINTER
    assert L.nmslib_gpu_deleted_rows(idx.h, None) == NULL_POINTER
    assert L.nmslib_gpu_delete_ids(idx.h, None, 0, C.byref(m)) == 0 and m.value == 0       # count == 0: SUCCESS
    assert L.nmslib_gpu_delete_ids(idx.h, one.ctypes.data, 0, None) == 0
    assert L.nmslib_gpu_delete_ids(idx.h, one.ctypes.data, 1, None) == 0                   # `marked` is optional
    assert idx.deletedRows() == 1
    idx.close()


def refused(idx):
    with pytest.raises(nz.NmslibError) as ei:
        idx.deleteIds([0])
    assert ei.value.code == SPACE_INCOMPATIBLE, ei.value
    for needle in ("hnsw, brute_force and seq_search", "dense spaces", "l2sqr_sift", "one device"):
        assert needle in str(ei.value), ei.value
    assert idx.deletedRows() == 0
    idx.close()


def test_sparse_string_divergence_and_sharded_indexes_are_refused():
    s = nz.Index("l2_sparse", "seq_search", data_type="SparseVector")
    s.addSparseBatch([([1, 2], [1.0, 1.0]), ([2, 5], [1.0, 2.0])])
    refused(s)
    for method in ("hnsw", "brute_force"):
        w = nz.Index("leven", method, data_type="ObjectAsString", dist_type="Int")
        w.addStringBatch(["kitten", "sitting", "mitten"])
        refused(w)
    d = nz.Index("kldivgenfast", "seq_search")
    d.addDenseBatch(np.abs(X) + 0.1)
    refused(d)
    refused(make_index("l2", "brute_force", X, gpu_defer=1, gpu_shards=2))
    refused(make_index("l2", "hnsw", X, gpu_shards=2, **HNSW))
    # the other order: tombstones first, shards asked for afterwards
    idx = nz.Index("l2", "brute_force")
    idx.addDenseBatch(X)
    assert idx.deleteIds([1]) == 1
    with pytest.raises(nz.NmslibError) as ei:
        idx.buildIndex(gpu_defer=1, gpu_shards=2)
    assert ei.value.code == SPACE_INCOMPATIBLE and "one device" in str(ei.value), ei.value
    idx.close()
