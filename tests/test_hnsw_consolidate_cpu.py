"""No GPU: nmslib_gpu_consolidate through the C ABI on indexes whose upload is deferred (gpu_defer=1), i.e. without a
resident graph: host rows, ids and marks are compacted and the index is then the index of the live rows alone."""
import ctypes as C
import os

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests.gpuutil import make_index

X = np.random.default_rng(21).standard_normal((60, 12)).astype(np.float32)
HNSW = dict(M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1)
NULL_POINTER, SPACE_INCOMPATIBLE, DATA_IO_FAILED = 1, 5, 10


def ids_with_a_triple():
    ids = np.arange(100, 160, dtype=np.int32)
    ids[[7, 20, 41]] = 1000                                      # one id carried by three rows
    return ids


DEAD_IDS = [1000, 100, 131, 132, 159]                            # positions 7, 20, 41, 0, 31, 32, 59
DEAD_POS = [0, 7, 20, 31, 32, 41, 59]


def test_the_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(nz.__file__), "..", "include", "nmslib_gpu.h")).read()
    assert "nmslib_gpu_consolidate" in header and "nmslib_gpu_consolidate" in nz.ABI_SYMBOLS_GPU
    assert getattr(nz.lib(), "nmslib_gpu_consolidate") is not None
    assert callable(nz.Index.consolidate)


@pytest.mark.parametrize("method,params", [("hnsw", HNSW), ("brute_force", dict(gpu_defer=1))])
def test_positions_move_to_the_rank_among_the_live_rows(method, params):
    ids = ids_with_a_triple()
    idx = make_index("l2", method, X, ids, **params)
    assert idx.deleteIds(DEAD_IDS) == len(DEAD_POS)
    assert idx.consolidate() == (len(DEAD_POS), 0)               # no resident graph: nothing is repaired
    live = np.setdiff1d(np.arange(60), DEAD_POS)
    assert idx.dataQty() == len(live) == 53 and idx.deletedRows() == 0
    for p, old in enumerate(live):
        np.testing.assert_array_equal(idx.getDataPoint(p), X[old])
    p, sz, fn = C.c_void_p(), C.c_size_t(), C.c_void_p()
    assert nz.lib().nmslib_borrow_data_dense(idx.h, 52, C.byref(p), C.byref(sz), C.byref(fn)) == 0
    np.testing.assert_array_equal(np.frombuffer(C.string_at(p, 48), np.float32), X[58])
    # a later delete works on the new positions: id 101 was position 1 and is position 0 now
    assert idx.deleteIds([101, 1000]) == 1 and idx.deletedRows() == 1
    assert idx.consolidate() == (1, 0)
    assert idx.dataQty() == 52
    np.testing.assert_array_equal(idx.getDataPoint(0), X[2])
    idx.close()


def test_the_consolidated_index_is_saved_as_the_index_of_the_live_rows(tmp_path):
    ids = ids_with_a_triple()
    idx = make_index("l2", "hnsw", X, ids, **HNSW)
    assert idx.deleteIds(DEAD_IDS) == len(DEAD_POS)
    a = str(tmp_path / "a.idx")
    with pytest.raises(nz.NmslibError) as ei:
        idx.save(a, save_data=True)
    assert ei.value.code == DATA_IO_FAILED and not os.path.exists(a), ei.value
    assert idx.consolidate()[0] == len(DEAD_POS)
    idx.save(a, save_data=True)
    idx.close()
    live = np.setdiff1d(np.arange(60), DEAD_POS)
    fresh = make_index("l2", "hnsw", X[live], ids[live], **HNSW)
    b = str(tmp_path / "b.idx")
    fresh.save(b, save_data=True)
    fresh.close()
    assert open(a, "rb").read() == open(b, "rb").read()
    assert open(a + ".dat", "rb").read() == open(b + ".dat", "rb").read()


def test_no_marks_is_a_no_op_and_so_is_the_second_call(tmp_path):
    idx = make_index("l2", "hnsw", X, **HNSW)
    before = str(tmp_path / "before.idx")
    idx.save(before, save_data=False)
    assert idx.consolidate() == (0, 0)
    assert idx.dataQty() == 60
    after = str(tmp_path / "after.idx")
    idx.save(after, save_data=False)
    assert open(before, "rb").read() == open(after, "rb").read()
    assert idx.deleteIds([3, 4]) == 2
    assert idx.consolidate() == (2, 0)
    assert idx.consolidate() == (0, 0)                           # twice in a row
    assert idx.dataQty() == 58 and idx.deletedRows() == 0
    idx.close()
    raw = nz.Index("l2", "hnsw")                                 # before nmslib_create_index: rows and marks only
    raw.addDenseBatch(X)
    assert raw.deleteIds([0, 59]) == 2
    assert raw.consolidate() == (2, 0)
    assert raw.dataQty() == 58
    np.testing.assert_array_equal(raw.getDataPoint(0), X[1])
    raw.close()


@pytest.mark.parametrize("method,params", [("hnsw", HNSW), ("seq_search", dict(gpu_defer=1))])
def test_every_row_marked_leaves_an_empty_index_that_takes_rows_again(method, params, tmp_path):
    idx = make_index("l2", method, X, **params)
    assert idx.deleteIds(np.arange(60)) == 60
    assert idx.consolidate() == (60, 0)
    assert idx.dataQty() == 0 and idx.deletedRows() == 0
    assert idx.consolidate() == (0, 0)
    idx.addDenseBatch(X[:20], np.arange(20, dtype=np.int32))
    idx.buildIndex(**params)
    assert idx.dataQty() == 20 and idx.deletedRows() == 0
    np.testing.assert_array_equal(idx.getDataPoint(19), X[19])
    if method == "hnsw":
        a, b = str(tmp_path / "a.idx"), str(tmp_path / "b.idx")
        idx.save(a, save_data=False)
        fresh = make_index("l2", "hnsw", X[:20], **params)
        fresh.save(b, save_data=False)
        fresh.close()
        assert open(a, "rb").read() == open(b, "rb").read()
    idx.close()


def test_null_handling():
    L = nz.lib()
    r, f = C.c_size_t(77), C.c_size_t(78)
    assert L.nmslib_gpu_consolidate(None, C.byref(r), C.byref(f)) == NULL_POINTER and (r.value, f.value) == (0, 0)
    assert L.nmslib_gpu_consolidate(None, None, None) == NULL_POINTER
    idx = make_index("l2", "hnsw", X, **HNSW)
    assert idx.deleteIds([1]) == 1
    assert L.nmslib_gpu_consolidate(idx.h, None, None) == 0      # both counts are optional
    assert idx.dataQty() == 59 and idx.deletedRows() == 0
    assert idx.deleteIds([2]) == 1
    assert L.nmslib_gpu_consolidate(idx.h, C.byref(r), None) == 0 and r.value == 1
    assert idx.deleteIds([3]) == 1
    r.value = 9
    assert L.nmslib_gpu_consolidate(idx.h, None, C.byref(r)) == 0 and r.value == 0
    idx.close()


def refused(idx, *needles):
    with pytest.raises(nz.NmslibError) as ei:
        idx.consolidate()
    assert ei.value.code == SPACE_INCOMPATIBLE, ei.value
    for needle in needles + ("hnsw, brute_force and seq_search", "dense spaces", "l2sqr_sift", "one device",
                             "built in this process", "delaunay_type 0-2", "maxM0 <= 254"):
        assert needle in str(ei.value), ei.value
    idx.close()


def test_indexes_that_are_not_served_are_refused(tmp_path):
    s = nz.Index("l2_sparse", "seq_search", data_type="SparseVector")
    s.addSparseBatch([([1, 2], [1.0, 1.0]), ([2, 5], [1.0, 2.0])])
    refused(s, "a sparse index")
    for method in ("hnsw", "brute_force"):
        w = nz.Index("leven", method, data_type="ObjectAsString", dist_type="Int")
        w.addStringBatch(["kitten", "sitting", "mitten"])
        refused(w, "a string index")
    d = nz.Index("kldivgenfast", "seq_search")
    d.addDenseBatch(np.abs(X) + 0.1)
    refused(d, "a divergence index")
    refused(make_index("l2", "brute_force", X, gpu_defer=1, gpu_shards=2), "gpu_shards=2")
    refused(make_index("l2", "hnsw", X, gpu_shards=2, **HNSW), "gpu_shards=2")
    # a graph loaded from a file
    path = str(tmp_path / "saved.idx")
    idx = make_index("l2", "hnsw", X, **HNSW)
    idx.save(path, save_data=True)
    idx.close()
    loaded = nz.Index.load(path)
    assert loaded.deleteIds([1]) == 1
    refused(loaded, "loaded from a file")
    # selection heuristic 3 and lists beyond the GPU builder's
    h3 = make_index("l2", "hnsw", X, delaunay_type=3, **HNSW)
    assert h3.deleteIds([1]) == 1
    refused(h3, "delaunay_type=3")
    wide = make_index("l2", "hnsw", X, **dict(HNSW, maxM0=300))
    assert wide.deleteIds([1]) == 1
    refused(wide, "wider than the GPU builder's")
