"""No GPU: the nmslib_gpu_filter_* entries through the C ABI on indexes whose upload is deferred (gpu_defer=1): what is
declared and bound, NULL handling, the argument checks, the indexes that are refused, and that a create which gets as far
as needing a device fails with the usual error and leaks nothing."""
import ctypes as C
import os

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests.gpuutil import make_index

X = np.random.default_rng(12).standard_normal((70, 12)).astype(np.float32)
HNSW = dict(M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1)
NULL_POINTER, INVALID_ARGUMENT, SPACE_INCOMPATIBLE, RUNTIME = 1, 2, 5, 13
NAMES = ("nmslib_gpu_filter_create", "nmslib_gpu_filter_destroy", "nmslib_gpu_filter_info",
         "nmslib_gpu_knn_query_batch_filtered", "nmslib_gpu_knn_query_batch_filtered_device")
ALL = np.full(3, 0xFFFFFFFF, np.uint32)          # 96 bits for 70 rows


def create(idx, bits, words, scan_rows=0):
    f = C.c_void_p(123)
    rc = nz.lib().nmslib_gpu_filter_create(idx.h, None if bits is None else bits.ctypes.data, words, scan_rows, C.byref(f))
    return rc, f, nz.last_error_detail(idx.alloc)


def test_the_five_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(nz.__file__), "..", "include", "nmslib_gpu.h")).read()
    for name in NAMES:
        assert name in header and name in nz.ABI_SYMBOLS_GPU
        fn = getattr(nz.lib(), name)
        assert fn.argtypes is not None
    assert "nmslib_gpu_filter_t" in header
    assert callable(nz.Index.makeFilter) and callable(nz.Index.knnQueryBatchFiltered)
    for attr in ("allowed", "hbm_bytes", "close"):
        assert hasattr(nz.Filter, attr)


@pytest.mark.parametrize("method,params", [("hnsw", HNSW), ("brute_force", dict(gpu_defer=1))])
def test_null_handling_and_argument_checks(method, params):
    L = nz.lib()
    idx = make_index("l2", method, X, **params)
    f = C.c_void_p()
    assert L.nmslib_gpu_filter_create(None, ALL.ctypes.data, 3, 0, C.byref(f)) == NULL_POINTER
    assert L.nmslib_gpu_filter_create(idx.h, ALL.ctypes.data, 3, 0, None) == NULL_POINTER
    rc, f, msg = create(idx, None, 3)
    assert rc == NULL_POINTER and not f.value and "allow_bits" in msg
    rc, f, msg = create(idx, ALL, 2)                             # 70 rows take 3 words
    assert rc == INVALID_ARGUMENT and not f.value and "3 words" in msg and "70 rows" in msg, msg
    rc, f, msg = create(idx, ALL, 3, scan_rows=4097)
    assert rc == INVALID_ARGUMENT and not f.value and "scan_rows" in msg and "4096" in msg, msg
    L.nmslib_gpu_filter_destroy(None)                            # harmless
    a, b = C.c_size_t(), C.c_size_t()
    assert L.nmslib_gpu_filter_info(None, C.byref(a), C.byref(b)) == NULL_POINTER
    q = np.zeros((1, 12), np.float32)
    ids, ds, cnt = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros(1, np.int32)
    assert L.nmslib_gpu_knn_query_batch_filtered(idx.h, None, q.ctypes.data, 1, 12, 1, ids.ctypes.data, ds.ctypes.data,
                                                 cnt.ctypes.data) == NULL_POINTER
    assert L.nmslib_gpu_knn_query_batch_filtered(None, None, q.ctypes.data, 1, 12, 1, ids.ctypes.data, ds.ctypes.data,
                                                 cnt.ctypes.data) == NULL_POINTER
    assert L.nmslib_gpu_knn_query_batch_filtered_device(idx.h, None, q.ctypes.data, 1, 12, 1, ids.ctypes.data,
                                                        ds.ctypes.data, None, None) == NULL_POINTER
    idx.close()


def test_python_mask_forms_are_checked_before_the_library_is_called():
    idx = make_index("l2", "hnsw", X, **HNSW)
    with pytest.raises(ValueError):
        idx.makeFilter(np.ones(69, bool))                        # not dataQty() long
    with pytest.raises(ValueError):
        idx.makeFilter(np.ones(70, np.int64))                    # neither bool nor uint32 words
    with pytest.raises(nz.NmslibError) as ei:
        idx.makeFilter(np.ones(2, np.uint32))                    # words: too few of them
    assert ei.value.code == INVALID_ARGUMENT
    idx.close()


def refused(idx):
    rc, f, msg = create(idx, ALL, 3)
    assert rc == SPACE_INCOMPATIBLE and not f.value, (rc, msg)
    for needle in ("takes no filter", "hnsw, brute_force and seq_search", "l2, l1, linf, cosinesimil, angulardist, negdotprod, "
                   "l2sqr_sift", "one device"):
        assert needle in msg, msg
    idx.close()


def test_sparse_string_divergence_and_sharded_indexes_are_refused_without_a_device():
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


@pytest.mark.parametrize("method,params", [("hnsw", HNSW), ("seq_search", dict(gpu_defer=1))])
def test_create_on_a_served_index_needs_a_device_and_leaks_nothing(method, params):
    """Without a device: the usual "no HIP device" error.  (With one the same calls make a filter, which is freed again.)"""
    idx = make_index("l2", method, X, **params)
    live = len(idx.alloc.live)
    rc, f, msg = create(idx, ALL, 3)
    if nz.lib().nmslib_gpu_device_count() == 0:
        assert rc == RUNTIME and not f.value and "no HIP device" in msg, (rc, msg)
        with pytest.raises(nz.NmslibError) as ei:
            idx.makeFilter(np.ones(70, bool))
        assert ei.value.code == RUNTIME and "no HIP device" in str(ei.value)
    else:
        assert rc == 0 and f.value, (rc, msg)
        a, b = C.c_size_t(), C.c_size_t()
        assert nz.lib().nmslib_gpu_filter_info(f, C.byref(a), C.byref(b)) == 0 and a.value == 70 and b.value > 0
        nz.lib().nmslib_gpu_filter_destroy(f)
    assert len(idx.alloc.live) == live                           # (the messages were handed back and freed)
    idx.close()
