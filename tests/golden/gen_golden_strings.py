#!/usr/bin/env python3
"""String fixture from the REAL reference (oracle/_ref/libnmslib_ref.so through its C ABI, data type 3, seq_search).

    make -C oracle ref && python3 tests/golden/gen_golden_strings.py

Sets (inputs regenerated from their seeds by the functions below, pinned by SHA-256):
  leven       : "ascii" (random printable strings of length 1-80), "long" (length 513-700: the reference's heap-buffer
                branch), "bytes8" (bytes 1-255), "small" (alphabet "ab", length 1-8: heavy ties), "onebyte" (one-byte
                rows), "tiny" (7 rows, k = 10 > n);
  bit_hamming : 32, 33, 256 and 1000 bits, written with the separators and labels the reference's parser accepts.
HNSW: the reference's recall@10 on a 5 000-row leven set (lowercase, length 5-20; M = 16, efConstruction = 200,
indexThreadQty = 1; the shim searches with efSearch = 200, nmslib_c.cpp:330), with the exact distances of the same
queries from seq_search; recall counts a returned row whose distance is at most the 10th exact distance.  And the Zig
test "Index string data workflow" (lib.zig:1381-1398) run through the reference: "hello", "world", k = 2.
Cases per set: k = 10 and k = 100, range at two radii (the 3rd and 10th k-NN distance) with capacities 4 and 1000,
get_distance over fixed pairs, and nmslib_get_data_point_string's bytes for a few positions.
Only the reference's outputs are stored.

Tie order: the reference's queue orders equal distances by object address, so the k-NN cases ask for every row
(k = n) and store the results in (distance, position) order, cut to k (as gen_golden_sparse.py does).
"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import orc  # noqa: E402

RANGE_CAPS = (4, 1000)
POINT_POS = (0, 1, 5)


def sha(strings):
    h = hashlib.sha256()
    for s in strings:
        h.update(len(s).to_bytes(8, "little"))
        h.update(s)
    return np.frombuffer(h.digest(), np.uint8).copy()


def _rand_str(rng, lo, hi, alphabet):
    m = int(rng.integers(lo, hi + 1))
    return bytes(alphabet[rng.integers(0, len(alphabet), size=m)].tolist())


def _bits_text(rng, bits, i):
    """0/1 values with mixed separators; every 7th row carries a label, every 5th a trailing blank"""
    v = rng.integers(0, 2, size=bits)
    seps = [b" ", b",", b":", b"  ", b"\t", b", "]
    out = bytearray()
    for j, b in enumerate(v.tolist()):
        if j:
            out += seps[int(rng.integers(0, len(seps)))] if i % 3 == 0 else b" "
        out += b"1" if b else b"0"
    if i % 7 == 0:
        out = bytearray(b"label:%d " % (i % 5)) + out
    if i % 5 == 0:
        out += b" "
    return bytes(out)


PRINTABLE = np.arange(32, 127, dtype=np.uint8)
BYTES8 = np.arange(1, 256, dtype=np.uint16)


def leven_sets():
    """-> {tag: (rows, queries)}"""
    rng = np.random.default_rng(20261016)
    out = {}
    out["ascii"] = ([_rand_str(rng, 1, 80, PRINTABLE) for _ in range(400)],
                    [_rand_str(rng, 1, 80, PRINTABLE) for _ in range(16)])
    out["long"] = ([_rand_str(rng, 513, 700, PRINTABLE[:8]) for _ in range(40)] +
                   [_rand_str(rng, 1, 64, PRINTABLE[:8]) for _ in range(20)],
                   [_rand_str(rng, 513, 600, PRINTABLE[:8]) for _ in range(4)] + [_rand_str(rng, 60, 70, PRINTABLE[:8])])
    out["bytes8"] = ([_rand_str(rng, 1, 40, BYTES8) for _ in range(300)],
                     [_rand_str(rng, 1, 40, BYTES8) for _ in range(10)])
    ab = np.array([97, 98], np.uint8)
    out["small"] = ([_rand_str(rng, 1, 8, ab) for _ in range(300)], [_rand_str(rng, 1, 8, ab) for _ in range(10)])
    out["onebyte"] = ([_rand_str(rng, 1, 1, PRINTABLE[:20]) for _ in range(200)],
                      [_rand_str(rng, 1, 3, PRINTABLE[:20]) for _ in range(6)])
    out["tiny"] = ([_rand_str(rng, 1, 12, PRINTABLE[:6]) for _ in range(7)],
                   [_rand_str(rng, 1, 12, PRINTABLE[:6]) for _ in range(3)])
    return out


def bit_sets():
    out = {}
    for bits, n in ((32, 300), (33, 300), (256, 300), (1000, 200)):
        rng = np.random.default_rng(1000 + bits)
        out[f"b{bits}"] = ([_bits_text(rng, bits, i) for i in range(n)],
                           [_bits_text(rng, bits, i + 1) for i in range(10)])
    return out


LOWER = np.arange(97, 123, dtype=np.uint8)
HNSW_M, HNSW_EFC, HNSW_K = 16, 200, 10


def hnsw_set():
    rng = np.random.default_rng(4242)
    return [_rand_str(rng, 5, 20, LOWER) for _ in range(5000)], [_rand_str(rng, 5, 20, LOWER) for _ in range(100)]


def recall_at_k(dists, exact, k=HNSW_K):
    """returned rows whose distance is at most the k-th exact distance, over k, averaged over queries"""
    return float(np.mean([min(k, int(np.sum(d[:k] <= e[k - 1]))) / k for d, e in zip(dists, exact)]))


def pairs_for(n):
    rng = np.random.default_rng(n)
    return np.array([[0, 1], [1, 0], [2, 2], [0, n - 1]] + rng.integers(0, n, size=(8, 2)).tolist(), np.int64)


# ---- the reference's C ABI (include/nmslib_c.h) over ctypes ---------------------------------------------------------
class _Alloc(C.Structure):
    _fields_ = [("alloc", C.CFUNCTYPE(C.c_void_p, C.c_size_t, C.c_void_p)),
                ("free", C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)), ("ctx", C.c_void_p)]


class _Result(C.Structure):
    _fields_ = [("ids", C.POINTER(C.c_int32)), ("distances", C.POINTER(C.c_float)),
                ("size", C.c_size_t), ("capacity", C.c_size_t)]


_libc = C.CDLL(None)
_libc.malloc.restype = C.c_void_p
_libc.malloc.argtypes = [C.c_size_t]
_libc.free.argtypes = [C.c_void_p]
_ALLOC = _Alloc(_Alloc._fields_[0][1](lambda n, ctx: _libc.malloc(max(n, 1))),
                _Alloc._fields_[1][1](lambda p, ctx: _libc.free(p)), None)


def ref_lib():
    L = C.CDLL(orc.REF_LIB)
    vp, sz = C.c_void_p, C.c_size_t
    L.nmslib_index_create.argtypes = [C.c_char_p, vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(_Alloc), C.POINTER(vp)]
    L.nmslib_add_data_point_batch_string.argtypes = [vp, vp, sz, vp]
    L.nmslib_create_index.argtypes = [vp, vp, C.c_int]
    L.nmslib_knn_query_fill.argtypes = [vp, vp, sz, sz, C.POINTER(_Result), sz]
    L.nmslib_range_query_fill.argtypes = [vp, vp, sz, C.c_double, C.POINTER(_Result), sz]
    L.nmslib_get_distance.argtypes = [vp, sz, sz, C.POINTER(C.c_float)]
    L.nmslib_get_data_point_string.argtypes = [vp, sz, C.POINTER(vp), C.POINTER(sz), C.POINTER(_Alloc)]
    L.nmslib_index_memory_usage.restype = sz
    L.nmslib_index_memory_usage.argtypes = [vp]
    L.nmslib_index_destroy.argtypes = [vp]
    L.nmslib_create_params.restype = vp
    L.nmslib_create_params.argtypes = [C.POINTER(_Alloc)]
    L.nmslib_add_param.argtypes = [vp, C.c_char_p, C.c_int, vp]
    L.nmslib_free_params.argtypes = [vp]
    return L


class RefIndex:
    def __init__(self, L, space, rows, method="seq_search", params=None):
        self.L = L
        L.nmslib_init()
        self.h = C.c_void_p()
        assert L.nmslib_index_create(space.encode(), None, method.encode(), 3, 1, C.byref(_ALLOC), C.byref(self.h)) == 0
        arr = (C.c_char_p * len(rows))(*rows)
        assert L.nmslib_add_data_point_batch_string(self.h, C.cast(arr, C.c_void_p), len(rows), None) == 0
        p = None
        if params:
            p = C.c_void_p(L.nmslib_create_params(C.byref(_ALLOC)))
            for key, v in params.items():
                iv = C.c_int(v)
                assert L.nmslib_add_param(p, key.encode(), 0, C.byref(iv)) == 0
        assert L.nmslib_create_index(self.h, p, 0) == 0
        if p:
            L.nmslib_free_params(p)
        self.n = len(rows)

    def knn(self, q, k):
        buf = np.frombuffer(q + b"\0", np.uint8).copy()
        ids = np.full(k, -1, np.int32)
        ds = np.full(k, np.inf, np.float32)
        r = _Result(ids.ctypes.data_as(C.POINTER(C.c_int32)), ds.ctypes.data_as(C.POINTER(C.c_float)), 0, k)
        assert self.L.nmslib_knn_query_fill(self.h, buf.ctypes.data, len(q) + 1, k, C.byref(r), 0) == 0
        o = np.lexsort((ids[:r.size], ds[:r.size]))
        return ids[:r.size][o], ds[:r.size][o]

    def knn_all(self, q):
        buf = np.frombuffer(q + b"\0", np.uint8).copy()
        ids = np.full(self.n, -1, np.int32)
        ds = np.full(self.n, np.inf, np.float32)
        r = _Result(ids.ctypes.data_as(C.POINTER(C.c_int32)), ds.ctypes.data_as(C.POINTER(C.c_float)), 0, self.n)
        assert self.L.nmslib_knn_query_fill(self.h, buf.ctypes.data, len(q) + 1, self.n, C.byref(r), 0) == 0
        assert r.size == self.n
        o = np.lexsort((ids, ds))
        return ids[o], ds[o]

    def range(self, q, radius, capacity):
        buf = np.frombuffer(q + b"\0", np.uint8).copy()
        ids = np.full(capacity, -1, np.int32)
        ds = np.full(capacity, np.inf, np.float32)
        r = _Result(ids.ctypes.data_as(C.POINTER(C.c_int32)), ds.ctypes.data_as(C.POINTER(C.c_float)), 0, capacity)
        assert self.L.nmslib_range_query_fill(self.h, buf.ctypes.data, len(q) + 1, float(radius), C.byref(r), 0) == 0
        return ids[:r.size], ds[:r.size]

    def distance(self, a, b):
        v = C.c_float()
        assert self.L.nmslib_get_distance(self.h, int(a), int(b), C.byref(v)) == 0
        return v.value

    def point_string(self, pos):
        p, n = C.c_void_p(), C.c_size_t()
        assert self.L.nmslib_get_data_point_string(self.h, pos, C.byref(p), C.byref(n), C.byref(_ALLOC)) == 0
        s = C.string_at(p, n.value)
        _libc.free(p)
        return s

    def close(self):
        self.L.nmslib_index_destroy(self.h)


def run_set(L, space, tag, rows, queries, out):
    ix = RefIndex(L, space, rows)
    n = len(rows)
    out[f"{tag}_rows_sha"], out[f"{tag}_queries_sha"] = sha(rows), sha(queries)
    full = [ix.knn_all(q) for q in queries]
    for k in (10, 100):
        ids = np.full((len(queries), k), -1, np.int32)
        ds = np.full((len(queries), k), np.inf, np.float32)
        for i, (a, b) in enumerate(full):
            ids[i, :min(k, n)], ds[i, :min(k, n)] = a[:k], b[:k]
        out[f"{tag}_k{k}_ids"], out[f"{tag}_k{k}_dists"] = ids, ds
    radii = np.array([[f[1][min(2, n - 1)], f[1][min(9, n - 1)]] for f in full], np.float64)
    out[f"{tag}_radii"] = radii
    for cap in RANGE_CAPS:
        rid, rd, rn = [], [], []
        for qi, q in enumerate(queries):
            for r in radii[qi]:
                a, b = ix.range(q, r, cap)
                rid.append(a)
                rd.append(b)
                rn.append(len(a))
        out[f"{tag}_range{cap}_n"] = np.array(rn, np.int32)
        out[f"{tag}_range{cap}_ids"] = np.concatenate(rid).astype(np.int32)
        out[f"{tag}_range{cap}_dists"] = np.concatenate(rd).astype(np.float32)
    pairs = pairs_for(n)
    out[f"{tag}_pairs"] = pairs
    out[f"{tag}_pair_dists"] = np.array([ix.distance(a, b) for a, b in pairs], np.float32)
    for p in POINT_POS:
        if p < n:
            out[f"{tag}_point{p}"] = np.frombuffer(ix.point_string(p), np.uint8).copy()
    out[f"{tag}_memory"] = np.array([L.nmslib_index_memory_usage(ix.h)], np.int64)
    ix.close()


def run_reference():
    L = ref_lib()
    out = {}
    for tag, (rows, qs) in leven_sets().items():
        run_set(L, "leven", "leven_" + tag, rows, qs, out)
    for tag, (rows, qs) in bit_sets().items():
        run_set(L, "bit_hamming", "bit_" + tag, rows, qs, out)
    rows, qs = hnsw_set()
    out["hnsw_rows_sha"], out["hnsw_queries_sha"] = sha(rows), sha(qs)
    ex = RefIndex(L, "leven", rows)
    exact = np.array([ex.knn(q, HNSW_K)[1] for q in qs], np.float32)
    ex.close()
    hx = RefIndex(L, "leven", rows, "hnsw", {"M": HNSW_M, "efConstruction": HNSW_EFC, "indexThreadQty": 1})
    got = [hx.knn(q, HNSW_K)[1] for q in qs]
    hx.close()
    out["hnsw_exact_dists"] = exact
    out["hnsw_ref_recall"] = np.array([recall_at_k(got, exact)], np.float64)
    zx = RefIndex(L, "leven", [b"hello", b"world"], "hnsw")
    zi, zd = zx.knn(b"hello", 2)
    out["zig_ids"], out["zig_dists"] = zi.astype(np.int32), zd.astype(np.float32)
    out["zig_point0"] = np.frombuffer(zx.point_string(0), np.uint8).copy()
    zx.close()
    return out


def main():
    assert os.path.exists(orc.REF_LIB), "build oracle/_ref first: make -C oracle ref"
    out = run_reference()
    path = os.path.join(HERE, "golden_strings.npz")
    # fixed member dates: a rerun gives the same bytes
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.save(buf, out[key], allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(2020, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(len(out), "arrays ->", path)


if __name__ == "__main__":
    main()
