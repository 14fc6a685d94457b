"""nmslib_zig_amd -- MI355X-native k-NN engine behind the NMSLIB-ZIG C ABI.

This package is a thin host-side mirror of the reference's Zig binding (lib.zig:495-1270:
Index.init / addDenseBatch / addUInt8Batch / buildIndex / knnQuery / knnQueryBatch / ...)
written against the *same* C ABI (include/nmslib_c.h) that lib.zig binds with @cImport.  All
k-NN work happens inside libnmslib_c.so (HIP kernels for gfx950); nothing here computes
distances, and importing the package fails loudly if the library is missing.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnmslib_c.so")

# nmslib_error_t (nmslib_c.h:21-37) -> exception names follow lib.zig:56-73
ERRORS = {
    1: "NullPointer", 2: "InvalidArgument", 3: "OutOfMemory", 4: "BufferTooSmall",
    5: "SpaceIncompatible", 6: "QueryTooLarge", 7: "InvalidSparseElement", 8: "IndexBuildFailed",
    9: "QueryExecutionFailed", 10: "DataIOFailed", 11: "PluginRegistrationFailed", 12: "Internal",
    13: "Runtime", 14: "IndexNotBuilt",
}
DATATYPE = {"DenseVector": 0, "SparseVector": 1, "DenseUInt8Vector": 2, "ObjectAsString": 3}
DISTTYPE = {"Float": 0, "Int": 1}
# nmslib_sparse_elem_float_t (nmslib_c.h): {uint32 id, float value}
SPARSE_ELEM = np.dtype([("id", "<u4"), ("value", "<f4")])


def sparse_rows(rows):
    """Pack sparse rows back to back, the reference's batch layout (nmslib_c.cpp:770-800).
    rows: a list of (ids, values) pairs, a CSR triple (indptr, indices, data) of arrays, or an object with
    .indptr / .indices / .data (scipy's csr_matrix).  -> (elements [total] SPARSE_ELEM, counts [n] uint64)"""
    if hasattr(rows, "indptr"):
        rows = (rows.indptr, rows.indices, rows.data)
    if isinstance(rows, tuple) and len(rows) == 3 and all(isinstance(a, np.ndarray) for a in rows):
        indptr = np.asarray(rows[0], np.int64)
        el = np.empty(int(indptr[-1] - indptr[0]), SPARSE_ELEM)
        el["id"] = np.asarray(rows[1])[indptr[0]:indptr[-1]]
        el["value"] = np.asarray(rows[2])[indptr[0]:indptr[-1]]
        return el, np.diff(indptr).astype(np.uint64)
    counts = np.array([len(r[0]) for r in rows], np.uint64)
    el = np.empty(int(counts.sum()), SPARSE_ELEM)
    at = 0
    for ids, vals in rows:
        m = len(ids)
        el["id"][at:at + m] = ids
        el["value"][at:at + m] = vals
        at += m
    return el, counts


def _as_bytes(s):
    return s.encode() if isinstance(s, str) else bytes(s)


def sparse_vector(ids, values):
    """One sparse vector as nmslib_sparse_elem_float_t elements."""
    el = np.empty(len(ids), SPARSE_ELEM)
    el["id"] = ids
    el["value"] = values
    return el


class NmslibError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        self.name = ERRORS.get(code, "Runtime")
        super().__init__(f"{self.name} ({code}): {detail}")


class Allocator(C.Structure):
    _fields_ = [("alloc", C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)),
                ("free", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)),
                ("ctx", C.c_void_p)]


class Result(C.Structure):
    _fields_ = [("ids", C.POINTER(C.c_int32)), ("distances", C.POINTER(C.c_float)),
                ("size", C.c_size_t), ("capacity", C.c_size_t)]


class ErrorDetail(C.Structure):
    _fields_ = [("code", C.c_int), ("message", C.c_void_p), ("file", C.c_void_p), ("line", C.c_int)]


class GpuStats(C.Structure):
    _fields_ = [("upload_seconds", C.c_double), ("build_seconds", C.c_double),
                ("hbm_bytes", C.c_size_t), ("rows", C.c_size_t), ("dim", C.c_size_t), ("shards", C.c_size_t),
                ("last_path", C.c_size_t), ("fast_tiles", C.c_size_t), ("fast_tiles_precise", C.c_size_t),
                ("fast_tiles_fallback", C.c_size_t), ("hnsw_redone", C.c_size_t),
                ("rows_appended", C.c_size_t), ("rows_uploaded", C.c_size_t)]


def build_library(force=False):
    """Compile nmslib_zig_amd/libnmslib_c.so with hipcc for gfx950 (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", csrc, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", csrc, "-j8"], stdout=subprocess.DEVNULL)
    return LIB_PATH


_lib = None
_alloc_live = {}


def lib():
    """Load the C ABI.  There is no fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "or `make -C nmslib_zig_amd/csrc` (the engine has no CPU fallback)")
    # One HIP runtime per process: PyTorch's wheels request "libamdhip64.so" (their bundled copy)
    # while this library is linked against the SONAME "libamdhip64.so.7".  Opening the runtime
    # by its unversioned NAME first makes both requests resolve to the same loaded object,
    # whichever of torch / this library is imported first (two runtimes in one process cannot
    # both see the GPU).
    try:
        C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
    except OSError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, sz, i32p, f32p = C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    AP = C.POINTER(Allocator)
    sigs = {
        "nmslib_init": (None, []),
        "nmslib_index_create": (C.c_int, [C.c_char_p, vp, C.c_char_p, C.c_int, C.c_int, AP, C.POINTER(vp)]),
        "nmslib_index_destroy": (None, [vp]),
        "nmslib_create_index": (C.c_int, [vp, vp, C.c_int]),
        "nmslib_reset_index": (C.c_int, [vp]),
        "nmslib_create_params": (vp, [AP]),
        "nmslib_add_param": (C.c_int, [vp, C.c_char_p, C.c_int, vp]),
        "nmslib_free_params": (None, [vp]),
        "nmslib_get_space_type": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), AP]),
        "nmslib_get_method": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), AP]),
        "nmslib_free_string": (None, [vp, AP]),
        "nmslib_get_last_error_detail": (C.c_int, [C.POINTER(ErrorDetail), AP]),
        "nmslib_add_data_point": (C.c_int, [vp, vp, sz, C.c_int32]),
        "nmslib_add_data_point_batch": (C.c_int, [vp, vp, sz, sz, vp, vp]),
        "nmslib_add_data_point_batch_uint8": (C.c_int, [vp, vp, sz, sz, vp]),
        "nmslib_add_data_point_batch_string": (C.c_int, [vp, vp, sz, vp]),
        "nmslib_gpu_string_hnsw_links": (C.c_int, [vp, sz, C.c_int, vp, sz, C.POINTER(sz), C.POINTER(C.c_int),
                                                  C.POINTER(C.c_int)]),
        "nmslib_add_data_point_batch_pointers": (C.c_int, [vp, C.c_int, vp, sz, sz, vp, vp]),
        "nmslib_knn_query_get_size": (C.c_int, [vp, vp, sz, sz, C.POINTER(sz), sz]),
        "nmslib_knn_query_fill": (C.c_int, [vp, vp, sz, sz, C.POINTER(Result), sz]),
        "nmslib_knn_query_batch": (C.c_int, [vp, vp, sz, sz, sz, C.POINTER(Result), vp, sz]),
        "nmslib_range_query_get_size": (C.c_int, [vp, vp, sz, C.c_double, C.POINTER(sz), sz]),
        "nmslib_range_query_fill": (C.c_int, [vp, vp, sz, C.c_double, C.POINTER(Result), sz]),
        "nmslib_get_distance": (C.c_int, [vp, sz, sz, C.POINTER(C.c_float)]),
        "nmslib_get_data_point_size": (C.c_int, [vp, sz, C.POINTER(sz)]),
        "nmslib_get_data_point_fill": (C.c_int, [vp, sz, vp, sz]),
        "nmslib_get_data_point_string": (C.c_int, [vp, sz, C.POINTER(vp), C.POINTER(sz), AP]),
        "nmslib_borrow_data_dense": (C.c_int, [vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp)]),
        "nmslib_borrow_data_sparse": (C.c_int, [vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp)]),
        "nmslib_save_index": (C.c_int, [vp, C.c_char_p, C.c_int]),
        "nmslib_load_index": (C.c_int, [C.c_char_p, C.c_int, C.c_int, AP, C.c_int, C.POINTER(vp)]),
        "nmslib_set_query_time_params": (C.c_int, [vp, vp]),
        "nmslib_set_thread_pool_size": (C.c_int, [vp, sz]),
        "nmslib_get_thread_pool_size": (sz, [vp]),
        "nmslib_data_qty": (sz, [vp]),
        "nmslib_index_memory_usage": (sz, [vp]),
        "nmslib_initialize_pool": (None, [vp]),
        "nmslib_free_result": (None, [C.POINTER(Result), AP]),
        # device-resident extensions (include/nmslib_gpu.h)
        "nmslib_gpu_device_count": (C.c_int, []),
        "nmslib_gpu_finalize": (C.c_int, [vp]),
        "nmslib_gpu_knn_query_batch_device": (C.c_int, [vp, vp, sz, sz, sz, vp, vp, vp, vp]),
        "nmslib_gpu_last_batch_counters": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]),
        "nmslib_gpu_merge_topk": (C.c_int, [vp, vp, sz, sz, sz, vp, vp, vp]),
        "nmslib_gpu_merge_topk_strided": (C.c_int, [vp, vp, sz, sz, sz, sz, vp, vp, vp]),
        "nmslib_gpu_get_stats": (C.c_int, [vp, C.POINTER(GpuStats)]),
        "nmslib_gpu_kernel_timing": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
        "nmslib_gpu_graph_builder": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "nmslib_gpu_delete_ids": (C.c_int, [vp, vp, sz, C.POINTER(sz)]),
        "nmslib_gpu_deleted_rows": (C.c_int, [vp, C.POINTER(sz)]),
        "nmslib_gpu_consolidate": (C.c_int, [vp, C.POINTER(sz), C.POINTER(sz)]),
        "nmslib_gpu_filter_create": (C.c_int, [vp, vp, sz, sz, C.POINTER(vp)]),
        "nmslib_gpu_filter_destroy": (None, [vp]),
        "nmslib_gpu_filter_info": (C.c_int, [vp, C.POINTER(sz), C.POINTER(sz)]),
        "nmslib_gpu_knn_query_batch_filtered": (C.c_int, [vp, vp, vp, sz, sz, sz, vp, vp, vp]),
        "nmslib_gpu_knn_query_batch_filtered_device": (C.c_int, [vp, vp, vp, sz, sz, sz, vp, vp, vp, vp]),
        "nmslib_gpu_knn_query_batch_filtered_each": (C.c_int, [vp, vp, sz, vp, vp, sz, sz, sz, vp, vp, vp, vp]),
        "nmslib_gpu_knn_query_batch_filtered_each_device": (C.c_int, [vp, vp, sz, vp, vp, sz, sz, sz, vp, vp, vp, vp, vp]),
        "nmslib_gpu_range_query_batch": (C.c_int, [vp, vp, sz, sz, vp, sz, vp, vp, vp, vp]),
        "nmslib_gpu_range_query_batch_device": (C.c_int, [vp, vp, sz, sz, vp, sz, vp, vp, vp, vp, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)   # AttributeError here = a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


ABI_SYMBOLS_C = [  # the 37 symbols of the reference boundary
    "nmslib_init", "nmslib_index_create", "nmslib_index_destroy", "nmslib_create_index",
    "nmslib_reset_index", "nmslib_create_params", "nmslib_add_param", "nmslib_free_params",
    "nmslib_get_space_type", "nmslib_get_method", "nmslib_free_string",
    "nmslib_get_last_error_detail", "nmslib_add_data_point", "nmslib_add_data_point_batch",
    "nmslib_add_data_point_batch_uint8", "nmslib_add_data_point_batch_string",
    "nmslib_knn_query_get_size", "nmslib_knn_query_fill", "nmslib_knn_query_batch",
    "nmslib_range_query_get_size", "nmslib_range_query_fill", "nmslib_get_distance",
    "nmslib_get_data_point_size", "nmslib_get_data_point_fill", "nmslib_get_data_point_string",
    "nmslib_borrow_data_dense", "nmslib_borrow_data_sparse", "nmslib_save_index",
    "nmslib_load_index", "nmslib_set_query_time_params", "nmslib_set_thread_pool_size",
    "nmslib_get_thread_pool_size", "nmslib_data_qty", "nmslib_index_memory_usage",
    "nmslib_add_data_point_batch_pointers", "nmslib_initialize_pool", "nmslib_free_result",
]
ABI_SYMBOLS_GPU = ["nmslib_gpu_device_count", "nmslib_gpu_finalize",
                   "nmslib_gpu_knn_query_batch_device", "nmslib_gpu_last_batch_counters",
                   "nmslib_gpu_merge_topk", "nmslib_gpu_merge_topk_strided", "nmslib_gpu_get_stats", "nmslib_gpu_kernel_timing",
                   "nmslib_gpu_string_hnsw_links", "nmslib_gpu_graph_builder", "nmslib_gpu_delete_ids",
                   "nmslib_gpu_deleted_rows", "nmslib_gpu_consolidate", "nmslib_gpu_filter_create",
                   "nmslib_gpu_filter_destroy", "nmslib_gpu_filter_info", "nmslib_gpu_knn_query_batch_filtered",
                   "nmslib_gpu_knn_query_batch_filtered_device", "nmslib_gpu_knn_query_batch_filtered_each",
                   "nmslib_gpu_knn_query_batch_filtered_each_device", "nmslib_gpu_range_query_batch",
                   "nmslib_gpu_range_query_batch_device"]


class TrackingAllocator:
    """The caller-side allocator the ABI requires (lib.zig:192-257): counts live blocks so tests
    can assert that the library returns everything it took."""

    def __init__(self):
        libc = C.CDLL(None)
        libc.malloc.restype = C.c_void_p
        libc.malloc.argtypes = [C.c_size_t]
        libc.free.argtypes = [C.c_void_p]
        self.live = {}
        self._libc = libc

        def _alloc(n, ctx):
            p = libc.malloc(max(n, 1))
            if p:
                self.live[p] = n
            return p

        def _free(p, ctx):
            if p:
                self.live.pop(p, None)
                libc.free(p)

        self._a = Allocator._fields_[0][1](_alloc)
        self._f = Allocator._fields_[1][1](_free)
        self.c = Allocator(self._a, self._f, None)

    def ref(self):
        return C.byref(self.c)


def last_error_detail(alloc):
    """nmslib_get_last_error_detail -> message; the returned strings are allocator-owned and are
    released with nmslib_free_string, as lib.zig does (lib.zig:564-571)."""
    d = ErrorDetail()
    L = lib()
    if L.nmslib_get_last_error_detail(C.byref(d), alloc.ref()) != 0:
        return ""
    msg = C.string_at(d.message).decode() if d.message else ""
    if d.message:
        L.nmslib_free_string(d.message, alloc.ref())
    if d.file:
        L.nmslib_free_string(d.file, alloc.ref())
    return msg


def _check(rc, alloc=None):
    if rc != 0:
        raise NmslibError(rc, last_error_detail(alloc) if alloc is not None else "")


class Params:
    """lib.zig:260-348 Params: typed name/value pairs behind nmslib_create_params / nmslib_add_param."""

    def __init__(self, alloc, **kw):
        self.alloc = alloc
        self.h = C.c_void_p(lib().nmslib_create_params(alloc.ref()))
        if not self.h:
            raise NmslibError(3, "nmslib_create_params")
        for k, v in kw.items():
            self.add(k, v)

    def add(self, key, value):
        L = lib()
        if isinstance(value, bool):
            value = int(value)
        if isinstance(value, int):
            v = C.c_int(value)
            _check(L.nmslib_add_param(self.h, key.encode(), 0, C.byref(v)), self.alloc)
        elif isinstance(value, float):
            v = C.c_double(value)
            _check(L.nmslib_add_param(self.h, key.encode(), 1, C.byref(v)), self.alloc)
        else:
            s = C.create_string_buffer(str(value).encode())
            _check(L.nmslib_add_param(self.h, key.encode(), 2, s), self.alloc)

    def free(self):
        if self.h:
            lib().nmslib_free_params(self.h)
            self.h = None


class Index:
    """Mirror of lib.zig's Index (lib.zig:495-1270) over the same C ABI.

    Call order is the reference's own *data-first* order (add -> nmslib_create_index -> queries),
    the order BASELINE.md prescribes; lib.zig's create-then-add order is also accepted by the
    library (nmslib_initialize_pool finalises a dirty index once)."""

    def __init__(self, space, method="hnsw", data_type="DenseVector", dist_type="Float", space_params=None):
        L = lib()
        L.nmslib_init()
        self.alloc = TrackingAllocator()
        if space == "cosine":        # lib.zig:530-533 canonicalisation
            space = "cosinesimil"
        self.data_type = data_type
        self.h = C.c_void_p()
        sp = Params(self.alloc, **space_params) if space_params else None
        rc = L.nmslib_index_create(space.encode(), sp.h if sp else None, method.encode(), DATATYPE[data_type],
                                   DISTTYPE[dist_type], self.alloc.ref(), C.byref(self.h))
        if sp:
            sp.free()
        _check(rc, self.alloc)
        self.built = False

    # -- data ------------------------------------------------------------------------------
    def addDenseBatch(self, data, ids=None):
        data = np.ascontiguousarray(data, np.float32)
        idp = None if ids is None else np.ascontiguousarray(ids, np.int32)
        _check(lib().nmslib_add_data_point_batch(self.h, data.ctypes.data, data.shape[0], data.shape[1],
                                                 None if idp is None else idp.ctypes.data, None), self.alloc)

    def addUInt8Batch(self, data, ids=None):
        data = np.ascontiguousarray(data, np.uint8)
        idp = None if ids is None else np.ascontiguousarray(ids, np.int32)
        _check(lib().nmslib_add_data_point_batch_uint8(self.h, data.ctypes.data, data.shape[0], data.shape[1],
                                                       None if idp is None else idp.ctypes.data), self.alloc)

    def addSparseBatch(self, rows, ids=None):
        """lib.zig:724-756: rows back to back, row i with num_elements[i] elements.  rows: see sparse_rows()."""
        el, counts = sparse_rows(rows)
        if len(counts) == 0:
            return
        el = np.ascontiguousarray(el)
        idp = None if ids is None else np.ascontiguousarray(ids, np.int32)
        _check(lib().nmslib_add_data_point_batch(self.h, el.ctypes.data, len(counts), max(int(counts.max()), 1),
                                                 None if idp is None else idp.ctypes.data, counts.ctypes.data),
               self.alloc)

    def addStringBatch(self, strings, ids=None):
        """lib.zig addStringBatch: one NUL-terminated string per row (nmslib_add_data_point_batch_string).  leven rows
        are the strings' bytes; bit_hamming rows are texts of 0/1 values ("0 1 1 0")."""
        bs = [_as_bytes(x) for x in strings]
        if not bs:
            return
        arr = (C.c_char_p * len(bs))(*bs)
        idp = None if ids is None else np.ascontiguousarray(ids, np.int32)
        _check(lib().nmslib_add_data_point_batch_string(self.h, C.cast(arr, C.c_void_p), len(bs),
                                                        None if idp is None else idp.ctypes.data), self.alloc)

    def buildIndex(self, **index_params):
        p = Params(self.alloc, **index_params) if index_params else None
        try:
            _check(lib().nmslib_create_index(self.h, p.h if p else None, 0), self.alloc)
        finally:
            if p:
                p.free()
        self.built = True

    def setQueryTimeParams(self, **params):
        """hnsw: efSearch / ef, algoType; engine extensions gpu_rows="f32"|"f16" (the walk reads an fp16 copy of the rows,
        the result is re-ranked in f32; also an index parameter of buildIndex) and gpu_rerank=R (how many entries of the
        final array are re-ranked); gpu_inwalk=0|1 (1: an index with deleted rows and a filtered batch test eligibility inside
        the walk, so that deleted and disallowed rows do not count against efSearch and selective filters return k results;
        served for max(efSearch, k) <= 1024 and maxM0 <= 254, on the f32 rows; stats()["last_path"] == 8).  The extensions
        stay as set until set again."""
        p = Params(self.alloc, **params)
        try:
            _check(lib().nmslib_set_query_time_params(self.h, p.h), self.alloc)
        finally:
            p.free()

    # -- queries (host buffers: the reference's own entry points) -----------------------------
    def _query(self, query):
        """-> (buffer, query_size_or_elem_count, num_elements); a sparse query is (ids, values) or SPARSE_ELEM elements
        (QueryPoint.SparseVector, lib.zig:414-424): its slot is 2 floats per element, num_elements its length."""
        if self.data_type == "SparseVector":
            q = query if isinstance(query, np.ndarray) and query.dtype == SPARSE_ELEM else sparse_vector(*query)
            q = np.ascontiguousarray(q)
            return q, max(2 * len(q), 1), len(q)
        if self.data_type == "ObjectAsString":   # create_object: elem_count - 1 bytes (nmslib_c.cpp:275-285)
            b = _as_bytes(query)
            return np.frombuffer(b + b"\0", np.uint8).copy(), len(b) + 1, 0
        q = np.ascontiguousarray(query, np.uint8 if self.data_type == "DenseUInt8Vector" else np.float32)
        return q, q.shape[0], 0

    def knnQuery(self, query, k):
        L = lib()
        q, qsz, ne = self._query(query)
        L.nmslib_initialize_pool(self.h)      # lib.zig:802
        cap = C.c_size_t()
        _check(L.nmslib_knn_query_get_size(self.h, q.ctypes.data, qsz, k, C.byref(cap), ne), self.alloc)
        ids = np.empty(cap.value, np.int32)
        ds = np.empty(cap.value, np.float32)
        r = Result(ids.ctypes.data_as(C.POINTER(C.c_int32)), ds.ctypes.data_as(C.POINTER(C.c_float)), 0, cap.value)
        _check(L.nmslib_knn_query_fill(self.h, q.ctypes.data, qsz, k, C.byref(r), ne), self.alloc)
        return ids[:r.size].copy(), ds[:r.size].copy()

    def rangeQuery(self, query, radius):
        """lib.zig:933-965: get_size (an estimate, 128) sizes the buffers, fill writes the first `capacity`
        objects within the radius, in insertion order.  HNSW -> NmslibError(SPACE_INCOMPATIBLE)."""
        L = lib()
        q, qsz, ne = self._query(query)
        L.nmslib_initialize_pool(self.h)
        cap = C.c_size_t()
        _check(L.nmslib_range_query_get_size(self.h, q.ctypes.data, qsz, float(radius), C.byref(cap), ne), self.alloc)
        return self.rangeQueryFill(q, radius, cap.value)

    def rangeQueryFill(self, query, radius, capacity):
        L = lib()
        q, qsz, ne = self._query(query)
        ids = np.empty(capacity, np.int32)
        ds = np.empty(capacity, np.float32)
        r = Result(ids.ctypes.data_as(C.POINTER(C.c_int32)), ds.ctypes.data_as(C.POINTER(C.c_float)), 0, capacity)
        _check(L.nmslib_range_query_fill(self.h, q.ctypes.data, qsz, float(radius), C.byref(r), ne), self.alloc)
        return ids[:r.size].copy(), ds[:r.size].copy()

    def rangeQueryBatch(self, queries, radii, capacity):
        """nmslib_gpu_range_query_batch: one range query per row of `queries`, each with its own radius (a scalar `radii`
        broadcasts), in one pass over the rows -> ids [Q, capacity], dists [Q, capacity], counts [Q], totals [Q].  Row q
        holds what rangeQueryFill(queries[q], radii[q], capacity) returns, bit for bit, then -1 / +inf; counts[q] =
        min(totals[q], capacity) entries are valid and totals[q] counts every row within the radius.  capacity = 0 counts
        only.  brute_force / seq_search over the dense float spaces and l2sqr_sift; stats()["last_path"] is 10 (the batched
        kernels) or 11 (one single-query chain per query: rows of more than 256 dimensions)."""
        q = np.ascontiguousarray(queries, np.uint8 if self.data_type == "DenseUInt8Vector" else np.float32)
        nq = q.shape[0]
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float64), (nq,)))
        ids = np.empty((nq, capacity), np.int32)      # (the call writes every element: the entries, then -1 / +inf)
        ds = np.empty((nq, capacity), np.float32)
        cnt = np.zeros(nq, np.int32)
        tot = np.zeros(nq, np.int32)
        _check(lib().nmslib_gpu_range_query_batch(self.h, q.ctypes.data, nq, q.shape[1], r.ctypes.data, capacity,
                                                  ids.ctypes.data if capacity else None,
                                                  ds.ctypes.data if capacity else None, cnt.ctypes.data, tot.ctypes.data),
               self.alloc)
        return ids, ds, cnt, tot

    def range_device(self, d_queries_ptr, nq, dim, radii, capacity, d_ids_ptr, d_dists_ptr, d_cnt_ptr=None,
                     d_totals_ptr=None, stream=None):
        """nmslib_gpu_range_query_batch_device: queries and results in device memory; radii (a scalar broadcasts) on the
        host, read before the call returns.  The call only enqueues."""
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(radii, np.float64), (nq,)))
        _check(lib().nmslib_gpu_range_query_batch_device(self.h, d_queries_ptr, nq, dim, r.ctypes.data, capacity, d_ids_ptr,
                                                         d_dists_ptr, d_cnt_ptr, d_totals_ptr, stream), self.alloc)

    def knnQueryBatch(self, queries, k):
        """One call of nmslib_knn_query_batch: a single GPU batch.  -> ids [Q,k], dists [Q,k], counts [Q]
        Sparse queries (see sparse_rows) are packed in the reference's slot layout (nmslib_c.cpp:1003-1031): query i
        at byte i * query_size_or_elem_count * 4, one slot of the longest query's size each, num_elements[i] elements."""
        L = lib()
        num = None
        if self.data_type == "ObjectAsString":
            return self._knn_string_batch(queries, k)
        if self.data_type == "SparseVector":
            el, counts = sparse_rows(queries)
            nq, width = len(counts), max(int(counts.max()) if len(counts) else 1, 1)
            q = np.zeros((nq, width), SPARSE_ELEM)
            starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
            for i in range(nq):
                q[i, :counts[i]] = el[starts[i]:starts[i + 1]]
            qsz = 2 * width
            num = np.ascontiguousarray(counts, np.uint64)
        else:
            q = np.ascontiguousarray(queries, np.uint8 if self.data_type == "DenseUInt8Vector" else np.float32)
            nq, qsz = q.shape[0], q.shape[1]
        ids = np.full((nq, k), -1, np.int32)
        ds = np.full((nq, k), np.inf, np.float32)
        res = (Result * nq)()
        for i in range(nq):
            res[i] = Result(ids[i].ctypes.data_as(C.POINTER(C.c_int32)),
                            ds[i].ctypes.data_as(C.POINTER(C.c_float)), 0, k)
        _check(L.nmslib_knn_query_batch(self.h, q.ctypes.data, nq, qsz, k, res,
                                        None if num is None else num.ctypes.data, 0), self.alloc)
        cnt = np.array([res[i].size for i in range(nq)], np.int32)
        return ids, ds, cnt

    def _knn_string_batch(self, queries, k):
        """String queries in the reference's batch layout (nmslib_c.cpp:1003-1031): query i at byte
        i * query_size_or_elem_count * 4, each query_size_or_elem_count - 1 bytes long.  One call per distinct length."""
        L = lib()
        bs = [_as_bytes(x) for x in queries]
        nq = len(bs)
        ids = np.full((nq, k), -1, np.int32)
        ds = np.full((nq, k), np.inf, np.float32)
        cnt = np.zeros(nq, np.int32)
        for ln in sorted(set(len(b) for b in bs)):
            sel = [i for i, b in enumerate(bs) if len(b) == ln]
            qsz = ln + 1
            buf = np.zeros((len(sel), 4 * qsz), np.uint8)
            for j, i in enumerate(sel):
                buf[j, :ln] = np.frombuffer(bs[i], np.uint8)
            gi = np.full((len(sel), k), -1, np.int32)
            gd = np.full((len(sel), k), np.inf, np.float32)
            res = (Result * len(sel))()
            for j in range(len(sel)):
                res[j] = Result(gi[j].ctypes.data_as(C.POINTER(C.c_int32)), gd[j].ctypes.data_as(C.POINTER(C.c_float)),
                                0, k)
            _check(L.nmslib_knn_query_batch(self.h, buf.ctypes.data, len(sel), qsz, k, res, None, 0), self.alloc)
            ids[sel], ds[sel] = gi, gd
            cnt[sel] = [res[j].size for j in range(len(sel))]
        return ids, ds, cnt

    def getDataPointString(self, pos):
        """nmslib_get_data_point_string: data_len bytes (the object's bytes as the reference's strncpy copy leaves
        them, plus the terminating NUL)."""
        p, n = C.c_void_p(), C.c_size_t()
        _check(lib().nmslib_get_data_point_string(self.h, pos, C.byref(p), C.byref(n), self.alloc.ref()), self.alloc)
        s = C.string_at(p, n.value)
        lib().nmslib_free_string(p, self.alloc.ref())
        return s

    # -- device-resident entry (include/nmslib_gpu.h) -------------------------------------------
    def finalize(self):
        _check(lib().nmslib_gpu_finalize(self.h), self.alloc)

    def knn_device(self, d_queries_ptr, nq, dim, k, d_ids_ptr, d_dists_ptr, d_cnt_ptr=None, stream=None):
        _check(lib().nmslib_gpu_knn_query_batch_device(self.h, d_queries_ptr, nq, dim, k, d_ids_ptr, d_dists_ptr,
                                                       d_cnt_ptr, stream), self.alloc)

    def last_counters(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().nmslib_gpu_last_batch_counters(self.h, C.byref(a), C.byref(b), C.byref(c)), self.alloc)
        return a.value, b.value, c.value

    def read_counters(self, nq):
        """Copy the per-query work counters of the last HNSW batch to the host:
        -> (ndc, hops, hops_up) int32 arrays, or None after a brute-force batch."""
        pn, ph, pu = self.last_counters()
        if not pn:
            return None
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipDeviceSynchronize()
        out = []
        for p in (pn, ph, pu):
            a = np.empty(nq, np.int32)
            rc = hip.hipMemcpy(a.ctypes.data, p, 4 * nq, 2)   # hipMemcpyDeviceToHost
            if rc != 0:
                raise RuntimeError(f"hipMemcpy failed: {rc}")
            out.append(a)
        return tuple(out)

    def kernel_timing(self, enable=True, collect=False):
        """HIP-event timing of the dominant kernel: -> (total_ms, launches) when collect."""
        ms, n = C.c_double(), C.c_uint64()
        _check(lib().nmslib_gpu_kernel_timing(self.h, int(enable), C.byref(ms) if collect else None,
                                              C.byref(n) if collect else None), self.alloc)
        return (ms.value, n.value) if collect else None

    def stats(self):
        s = GpuStats()
        _check(lib().nmslib_gpu_get_stats(self.h, C.byref(s)), self.alloc)
        return {f[0]: getattr(s, f[0]) for f in GpuStats._fields_}

    def graphBuilder(self):
        """Who built the HNSW graph: 0 = no graph or one loaded from a file, 1 = host builder, 2 = GPU builder."""
        b = C.c_int()
        _check(lib().nmslib_gpu_graph_builder(self.h, C.byref(b)), self.alloc)
        return b.value

    def deleteIds(self, ids):
        """nmslib_gpu_delete_ids: marks every stored row that carries one of `ids` as deleted -> rows newly marked.  Later
        k-NN and range results never contain them; positions do not move, and a row added later under a deleted id is live
        (update = deleteIds([id]), then add the new row under it).  hnsw: results are the first k live entries of the search
        for max(efSearch, k), so counts can fall below k under heavy deletion -- unless setQueryTimeParams(gpu_inwalk=1),
        under which a deleted row does not count against efSearch; brute_force / seq_search: the index is prepared again at
        its next use."""
        a = np.ascontiguousarray(ids, np.int32).reshape(-1)
        m = C.c_size_t()
        _check(lib().nmslib_gpu_delete_ids(self.h, a.ctypes.data if a.size else None, a.size, C.byref(m)), self.alloc)
        return m.value

    def deletedRows(self):
        """Rows of this index that are marked deleted."""
        n = C.c_size_t()
        _check(lib().nmslib_gpu_deleted_rows(self.h, C.byref(n)), self.alloc)
        return n.value

    def consolidate(self):
        """nmslib_gpu_consolidate: the rows marked by deleteIds leave the index -> (rows removed, adjacency lists rewritten).
        Positions move: a live row's new position is its rank among the live rows; ids do not change.  A resident hnsw
        graph is repaired around the deleted nodes and compacted on the GPU (no filter and counts of k afterwards, save()
        works again); without a resident graph, and for brute_force / seq_search, the host side is compacted and the index
        is built / prepared again at its next use.  Blocks until the device is done."""
        removed, repaired = C.c_size_t(), C.c_size_t()
        _check(lib().nmslib_gpu_consolidate(self.h, C.byref(removed), C.byref(repaired)), self.alloc)
        return removed.value, repaired.value

    # -- filtered search (nmslib_gpu_filter_*) ------------------------------------------------------
    def makeFilter(self, mask, scan_rows=0):
        """nmslib_gpu_filter_create: a subset of the index's positions, prepared on the GPU -> Filter.  mask: a bool array of
        length dataQty() (True = allowed), or the bitset itself as uint32 words (bit p & 31 of word p >> 5).  scan_rows
        (hnsw): a subset of at most max(efSearch, k, scan_rows) rows is scanned exactly instead of walked; 0 = default."""
        mask = np.asarray(mask)
        if mask.dtype == np.uint32:
            words = np.ascontiguousarray(mask).reshape(-1)
        else:
            if mask.dtype != np.bool_ or mask.ndim != 1 or mask.size != self.dataQty():
                raise ValueError("mask: a bool array of length dataQty(), or uint32 words")
            words = np.packbits(np.ascontiguousarray(mask), bitorder="little")
            words = np.concatenate([words, np.zeros(-len(words) % 4, np.uint8)]).view("<u4").astype(np.uint32)
        f = C.c_void_p()
        _check(lib().nmslib_gpu_filter_create(self.h, words.ctypes.data if words.size else None, words.size, scan_rows,
                                              C.byref(f)), self.alloc)
        return Filter(self, f)

    def knnQueryBatchFiltered(self, flt, queries, k):
        """nmslib_gpu_knn_query_batch_filtered: knnQueryBatch over the rows the filter allows -> ids [Q,k], dists [Q,k],
        counts [Q].  hnsw: counts can fall below k when few of the rows the search finds are allowed; a filter of at most
        max(efSearch, k, scan_rows) rows is answered exactly; setQueryTimeParams(gpu_inwalk=1) filters inside the walk
        instead, which keeps counts at k under selective filters."""
        q = np.ascontiguousarray(queries, np.uint8 if self.data_type == "DenseUInt8Vector" else np.float32)
        nq = q.shape[0]
        ids = np.full((nq, k), -1, np.int32)
        ds = np.full((nq, k), np.inf, np.float32)
        cnt = np.zeros(nq, np.int32)
        _check(lib().nmslib_gpu_knn_query_batch_filtered(self.h, flt.h, q.ctypes.data, nq, q.shape[1], k, ids.ctypes.data,
                                                         ds.ctypes.data, cnt.ctypes.data), self.alloc)
        return ids, ds, cnt

    def knn_device_filtered(self, flt, d_queries_ptr, nq, dim, k, d_ids_ptr, d_dists_ptr, d_cnt_ptr=None, stream=None):
        _check(lib().nmslib_gpu_knn_query_batch_filtered_device(self.h, flt.h, d_queries_ptr, nq, dim, k, d_ids_ptr,
                                                                d_dists_ptr, d_cnt_ptr, stream), self.alloc)

    @staticmethod
    def _filter_table(filters, filter_of_query, nq):
        """The host arrays of a batch with one filter per query: the handles, the int32 entries."""
        hs = (C.c_void_p * max(len(filters), 1))(*[f.h.value if isinstance(f.h, C.c_void_p) else f.h for f in filters])
        fq = np.ascontiguousarray(filter_of_query, np.int32).reshape(-1)
        if fq.size != nq:
            raise ValueError("filter_of_query: one entry per query")
        return hs, fq

    def knnQueryBatchEachFiltered(self, filters, filter_of_query, queries, k, return_routes=False):
        """nmslib_gpu_knn_query_batch_filtered_each: one batch whose query q runs under filters[filter_of_query[q]] (-1:
        unfiltered) -> ids [Q,k], dists [Q,k], counts [Q] and, with return_routes, routes [Q]: per query the last_path
        knnQueryBatchFiltered reports for its filter's queries.  Every row is what that call returns for the query.  hnsw: one
        launch chain per route, whatever the number of filters; brute_force / seq_search: one scan per filter with queries."""
        q = np.ascontiguousarray(queries, np.uint8 if self.data_type == "DenseUInt8Vector" else np.float32)
        nq = q.shape[0]
        hs, fq = self._filter_table(filters, filter_of_query, nq)
        ids = np.full((nq, k), -1, np.int32)
        ds = np.full((nq, k), np.inf, np.float32)
        cnt = np.zeros(nq, np.int32)
        routes = np.full(nq, -1, np.int32)
        _check(lib().nmslib_gpu_knn_query_batch_filtered_each(self.h, hs if len(filters) else None, len(filters),
                                                              fq.ctypes.data, q.ctypes.data, nq, q.shape[1], k, ids.ctypes.data,
                                                              ds.ctypes.data, cnt.ctypes.data, routes.ctypes.data), self.alloc)
        return (ids, ds, cnt, routes) if return_routes else (ids, ds, cnt)

    def knn_device_each_filtered(self, filters, filter_of_query, d_queries_ptr, nq, dim, k, d_ids_ptr, d_dists_ptr,
                                 d_cnt_ptr=None, stream=None, routes=None):
        """nmslib_gpu_knn_query_batch_filtered_each_device: queries and results in device memory, filter_of_query (and
        routes: an int32 array of nq entries, optional) on the host; both host arrays are read before the call returns."""
        hs, fq = self._filter_table(filters, filter_of_query, nq)
        _check(lib().nmslib_gpu_knn_query_batch_filtered_each_device(
            self.h, hs if len(filters) else None, len(filters), fq.ctypes.data, d_queries_ptr, nq, dim, k, d_ids_ptr,
            d_dists_ptr, d_cnt_ptr, routes.ctypes.data if routes is not None else None, stream), self.alloc)

    # -- metadata / stored data -------------------------------------------------------------------
    def getDistance(self, a, b):
        v = C.c_float()
        _check(lib().nmslib_get_distance(self.h, a, b, C.byref(v)), self.alloc)
        return v.value

    def dataQty(self):
        return lib().nmslib_data_qty(self.h)

    def _string(self, fn):
        p, n = C.c_void_p(), C.c_size_t()
        _check(fn(self.h, C.byref(p), C.byref(n), self.alloc.ref()), self.alloc)
        s = C.string_at(p, n.value).decode()
        lib().nmslib_free_string(p, self.alloc.ref())
        return s

    def getSpaceType(self):
        s = self._string(lib().nmslib_get_space_type)
        return "cosine" if s == "cosinesimil" else s   # lib.zig:1224-1240 round-trips the alias

    def getMethod(self):
        return self._string(lib().nmslib_get_method)

    def getDataPoint(self, pos):
        n = C.c_size_t()
        _check(lib().nmslib_get_data_point_size(self.h, pos, C.byref(n)), self.alloc)
        buf = np.empty(n.value, np.uint8)
        _check(lib().nmslib_get_data_point_fill(self.h, pos, buf.ctypes.data, n.value), self.alloc)
        if self.data_type == "DenseUInt8Vector":
            return buf[:128].copy()
        if self.data_type == "SparseVector":   # -> (ids, values)
            el = buf.view(SPARSE_ELEM)
            return el["id"].copy(), el["value"].copy()
        if self.data_type == "ObjectAsString":  # -> the object's bytes (bit_hamming: packed words + bit count)
            return buf.tobytes()
        return buf.view(np.float32).copy()

    def save(self, path, save_data=True):
        _check(lib().nmslib_save_index(self.h, path.encode(), int(save_data)), self.alloc)

    @classmethod
    def load(cls, path, data_type="DenseVector", dist_type="Float", load_data=True):
        self = cls.__new__(cls)
        self.alloc = TrackingAllocator()
        self.data_type = data_type
        self.h = C.c_void_p()
        _check(lib().nmslib_load_index(path.encode(), DATATYPE[data_type], DISTTYPE[dist_type], self.alloc.ref(),
                                       int(load_data), C.byref(self.h)), self.alloc)
        self.built = True
        return self

    def setThreadPoolSize(self, n):
        _check(lib().nmslib_set_thread_pool_size(self.h, n), self.alloc)

    def getThreadPoolSize(self):
        return lib().nmslib_get_thread_pool_size(self.h)

    def reset(self):
        _check(lib().nmslib_reset_index(self.h), self.alloc)
        self.built = False

    def close(self):
        if getattr(self, "h", None):
            lib().nmslib_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Filter:
    """A nmslib_gpu_filter_t of Index.makeFilter.  It belongs to its index and goes with it: close() after the index was
    closed does nothing."""

    def __init__(self, index, handle):
        self.index = index
        self.h = handle

    def _info(self):
        if not self.h or not self.index.h:
            raise NmslibError(2, "the filter or its index is closed")
        a, b = C.c_size_t(), C.c_size_t()
        _check(lib().nmslib_gpu_filter_info(self.h, C.byref(a), C.byref(b)), self.index.alloc)
        return a.value, b.value

    @property
    def allowed(self):
        """Rows the filter allows that are not deleted now."""
        return self._info()[0]

    @property
    def hbm_bytes(self):
        """Device memory the filter holds (not part of the index's hbm_bytes)."""
        return self._info()[1]

    def close(self):
        if self.h and self.index.h:
            lib().nmslib_gpu_filter_destroy(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
