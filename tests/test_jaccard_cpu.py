"""bit_jaccard (data type 3, float distance) without a GPU: which configurations are created and which are refused, the
space's name, and rows added through bit_hamming's parser."""
import ctypes as C

import pytest

import nmslib_zig_amd as nz


def create(method, dist_type):
    a = nz.TrackingAllocator()
    h = C.c_void_p()
    rc = nz.lib().nmslib_index_create(b"bit_jaccard", None, method.encode(), 3, dist_type, a.ref(), C.byref(h))
    return rc, h, a


def add_strings(h, strings):
    arr = (C.c_char_p * len(strings))(*strings)
    return nz.lib().nmslib_add_data_point_batch_string(h, C.cast(arr, C.c_void_p), len(strings), None)


@pytest.mark.parametrize("method", ["brute_force", "seq_search"])
def test_bit_jaccard_is_created_with_the_float_distance(method):
    rc, h, a = create(method, 0)
    assert rc == 0
    L = nz.lib()
    name, n = C.c_void_p(), C.c_size_t()
    assert L.nmslib_get_space_type(h, C.byref(name), C.byref(n), a.ref()) == 0
    assert C.string_at(name, n.value) == b"bit_jaccard"
    L.nmslib_free_string(name, a.ref())
    assert add_strings(h, [b"0 1 1 0 1", b"1,0,0,0,0", b"0 0 0 0 0"]) == 0
    assert add_strings(h, [b"1 1 1 1"]) == 2          # bit count differs from the index's
    assert add_strings(h, [b"1 2 0 0 0"]) == 13       # only 0 and 1
    assert L.nmslib_data_qty(h) == 3
    L.nmslib_index_destroy(h)
    assert len(a.live) == 0


@pytest.mark.parametrize("method,dist_type", [("seq_search", 1), ("brute_force", 1), ("hnsw", 0), ("hnsw", 1)])
def test_bit_jaccard_int_distance_and_hnsw_are_refused(method, dist_type):
    rc, h, a = create(method, dist_type)
    assert rc == 5
    assert len(a.live) == 0
