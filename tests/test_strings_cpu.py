"""String data (data type 3) without a GPU: the fixture against the compiled reference, the Python restatement
against the fixture, and the host logic of the C ABI over leven and bit_hamming indexes (creation, input errors,
stored objects, get_data_point_string, memory figures)."""
import ctypes as C
import os

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import orc, string_ref
from tests.golden import gen_golden_strings as gs

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_strings.npz")


def all_sets():
    out = {"leven_" + t: ("leven", r, q) for t, (r, q) in gs.leven_sets().items()}
    out.update({"bit_" + t: ("bit_hamming", r, q) for t, (r, q) in gs.bit_sets().items()})
    return out


SETS = all_sets()


@pytest.fixture(scope="module")
def gst():
    with np.load(GOLDEN) as z:
        d = {k: z[k] for k in z.files}
    for tag, (_, rows, qs) in SETS.items():
        assert np.array_equal(gs.sha(rows), d[f"{tag}_rows_sha"]), tag
        assert np.array_equal(gs.sha(qs), d[f"{tag}_queries_sha"]), tag
    return d


def ref_distance(space, a, b):
    if space == "leven":
        return string_ref.levenshtein(a, b)
    return string_ref.bit_hamming(string_ref.bit_object(a), string_ref.bit_object(b))


@pytest.mark.skipif(not os.path.exists(orc.REF_LIB), reason="oracle/_ref not built (make -C oracle ref)")
def test_fixture_equals_live_reference(gst):
    live = gs.run_reference()
    assert sorted(live) == sorted(gst)
    for key in live:
        np.testing.assert_array_equal(live[key], gst[key], err_msg=key)


@pytest.mark.parametrize("tag", sorted(SETS))
def test_restatement_equals_fixture(gst, tag):
    """k = 100 in (distance, position) order, range results, get_distance and the stored objects, all recomputed."""
    space, rows, qs = SETS[tag]
    n = len(rows)
    for qi, q in enumerate(qs):
        order, d = string_ref.knn(lambda i: ref_distance(space, rows[i], q), n, 100)
        got_i, got_d = gst[f"{tag}_k100_ids"][qi], gst[f"{tag}_k100_dists"][qi]
        m = min(100, n)
        np.testing.assert_array_equal(order, got_i[:m], err_msg=f"{tag} query {qi}")
        np.testing.assert_array_equal(d.astype(np.float32), got_d[:m])
        assert (got_i[m:] == -1).all()
    pd = [ref_distance(space, rows[a], rows[b]) for a, b in gst[f"{tag}_pairs"]]
    np.testing.assert_array_equal(np.array(pd, np.float32), gst[f"{tag}_pair_dists"])
    at = 0
    rn = gst[f"{tag}_range1000_n"]
    for qi, q in enumerate(qs):
        d = np.array([ref_distance(space, r, q) for r in rows])
        for j, rad in enumerate(gst[f"{tag}_radii"][qi]):
            want = np.nonzero(d <= int(rad))[0]
            c = rn[2 * qi + j]
            np.testing.assert_array_equal(gst[f"{tag}_range1000_ids"][at:at + c], want)
            np.testing.assert_array_equal(gst[f"{tag}_range1000_dists"][at:at + c], d[want].astype(np.float32))
            at += c


# ---- C-ABI host logic -----------------------------------------------------------------------------------------------
def build_deferred(h, a):
    """nmslib_create_index with the upload to HBM deferred to the first query (nothing here needs a device)"""
    p = nz.Params(a, gpu_defer=1)
    rc = nz.lib().nmslib_create_index(h, p.h, 0)
    p.free()
    return rc


def create(space, method="seq_search", data_type=3, dist_type=1):
    L = nz.lib()
    a = nz.TrackingAllocator()
    h = C.c_void_p()
    rc = L.nmslib_index_create(space.encode(), None, method.encode(), data_type, dist_type, a.ref(), C.byref(h))
    return rc, h, a


def add_strings(h, strings, ids=None):
    arr = (C.c_char_p * len(strings))(*strings)
    idp = None if ids is None else np.ascontiguousarray(ids, np.int32)
    return nz.lib().nmslib_add_data_point_batch_string(h, C.cast(arr, C.c_void_p), len(strings),
                                                       None if idp is None else idp.ctypes.data)


@pytest.mark.parametrize("space", ["leven", "bit_hamming"])
@pytest.mark.parametrize("method", ["brute_force", "seq_search", "hnsw"])
def test_string_spaces_are_created(space, method):
    rc, h, a = create(space, method)
    assert rc == 0
    idx_space = C.c_void_p()
    n = C.c_size_t()
    assert nz.lib().nmslib_get_space_type(h, C.byref(idx_space), C.byref(n), a.ref()) == 0
    assert C.string_at(idx_space, n.value) == space.encode()
    nz.lib().nmslib_free_string(idx_space, a.ref())
    nz.lib().nmslib_index_destroy(h)
    assert len(a.live) == 0


@pytest.mark.parametrize("space,method,dist_type", [
    ("leven", "hnsw", 0), ("bit_hamming", "seq_search", 0), ("normleven", "seq_search", 1),
    ("bit_jaccard", "seq_search", 1), ("l2", "seq_search", 1), ("cosinesimil", "brute_force", 1),
    ("leven", "vptree", 1)])
def test_unserved_string_configurations_are_space_incompatible(space, method, dist_type):
    rc, h, a = create(space, method, dist_type=dist_type)
    assert rc == 5
    assert len(a.live) == 0


def graph_of(h, n):
    """-> (links(node, level), maxlevel, enterpoint, node levels) through nmslib_gpu_string_hnsw_links"""
    L = nz.lib()
    out = (C.c_int32 * 8192)()
    cnt, ep, ml = C.c_size_t(), C.c_int(), C.c_int()
    lists, levels = {}, []
    for v in range(n):
        lvl = 0
        while L.nmslib_gpu_string_hnsw_links(h, v, lvl, out, 8192, C.byref(cnt), C.byref(ep), C.byref(ml)) == 0:
            lists[(v, lvl)] = list(out[:cnt.value])
            lvl += 1
        levels.append(lvl - 1)
    return (lambda v, lvl: lists[(v, lvl)]), ml.value, ep.value, levels


@pytest.mark.parametrize("space", ["leven", "bit_hamming"])
def test_host_hnsw_builder_with_string_distance(space):
    """The host builder over string rows: a well-formed graph (no self links, no repeats, lists within maxM0 / maxM,
    the entry point on the top level), the same graph on a rebuild, and a neighbour of each node's list beside it."""
    rng = np.random.default_rng(5)
    if space == "leven":
        rows = [gs._rand_str(rng, 3, 12, gs.LOWER[:6]) for _ in range(600)]
    else:
        rows = [" ".join(map(str, rng.integers(0, 2, 64).tolist())).encode() for _ in range(600)]
    graphs = []
    for _ in range(2):
        rc, h, a = create(space, "hnsw")
        assert rc == 0 and add_strings(h, rows) == 0
        p = nz.Params(a, M=8, efConstruction=50, indexThreadQty=1, gpu_defer=1)
        assert nz.lib().nmslib_create_index(h, p.h, 0) == 0
        p.free()
        graphs.append(graph_of(h, len(rows)))
        nz.lib().nmslib_index_destroy(h)
    links, ml, ep, levels = graphs[0]
    assert levels[ep] == ml == max(levels)
    for v in range(len(rows)):
        for lvl in range(levels[v] + 1):
            lst = links(v, lvl)
            assert v not in lst and len(set(lst)) == len(lst)
            assert len(lst) <= (16 if lvl == 0 else 8)
            assert all(levels[u] >= lvl for u in lst)
            assert lst == graphs[1][0](v, lvl)
        assert len(links(v, 0)) > 0
    # the level-0 list holds the node's nearest neighbour (it is inserted through the heuristic's first pick)
    d = lambda i, j: ref_distance(space, rows[i], rows[j])      # noqa: E731
    near = sum(min(d(v, u) for u in links(v, 0)) == min(d(v, u) for u in range(len(rows)) if u != v)
               for v in range(0, len(rows), 20))
    assert near >= 0.9 * len(range(0, len(rows), 20))


def test_graph_inspection_refuses_other_indexes():
    rc, h, a = create("leven", "seq_search")
    assert add_strings(h, [b"abc"]) == 0
    cnt, ep, ml = C.c_size_t(), C.c_int(), C.c_int()
    assert nz.lib().nmslib_gpu_string_hnsw_links(h, 0, 0, None, 0, C.byref(cnt), C.byref(ep), C.byref(ml)) == 5
    nz.lib().nmslib_index_destroy(h)


def test_string_batch_into_other_data_types_stays_refused():
    L = nz.lib()
    a = nz.TrackingAllocator()
    h = C.c_void_p()
    assert L.nmslib_index_create(b"l2", None, b"seq_search", 0, 0, a.ref(), C.byref(h)) == 0
    assert add_strings(h, [b"abc"]) == 5
    L.nmslib_index_destroy(h)


def test_leven_rows_objects_and_metadata():
    L = nz.lib()
    rc, h, a = create("leven")
    assert rc == 0
    rows = [b"hello", b"world", bytes(range(1, 200)), b"x"]
    assert add_strings(h, rows, [10, 11, 12, 13]) == 0
    s = b"ab\0cd"                                        # add_data_point: element_count - 1 bytes, NULs included
    assert L.nmslib_add_data_point(h, s, len(s) + 1, 14) == 0
    assert L.nmslib_data_qty(h) == 5
    rows.append(s)
    for i, r in enumerate(rows):
        sz = C.c_size_t()
        assert L.nmslib_get_data_point_size(h, i, C.byref(sz)) == 0 and sz.value == len(r)
        buf = (C.c_char * len(r))()
        assert L.nmslib_get_data_point_fill(h, i, buf, len(r)) == 0 and bytes(buf) == r
        p, n = C.c_void_p(), C.c_size_t()
        assert L.nmslib_get_data_point_string(h, i, C.byref(p), C.byref(n), a.ref()) == 0
        assert n.value == len(r) + 1
        # strncpy: the copy stops at the first NUL, the rest is zero
        cut = r.split(b"\0", 1)[0]
        assert C.string_at(p, n.value) == cut + b"\0" * (n.value - len(cut))
        L.nmslib_free_string(p, a.ref())
    assert L.nmslib_get_data_point_fill(h, 2, (C.c_char * 10)(), 10) == 4
    assert build_deferred(h, a) == 0
    assert L.nmslib_index_memory_usage(h) == sum(16 + len(r) for r in rows)
    L.nmslib_index_destroy(h)
    assert len(a.live) == 0


@pytest.mark.parametrize("tag", ["leven_ascii", "leven_bytes8", "bit_b33", "bit_b1000"])
def test_stored_objects_and_memory_equal_fixture(gst, tag):
    space, rows, _ = SETS[tag]
    L = nz.lib()
    rc, h, a = create(space)
    assert rc == 0 and add_strings(h, rows) == 0
    assert build_deferred(h, a) == 0
    for p in gs.POINT_POS:
        q, n = C.c_void_p(), C.c_size_t()
        assert L.nmslib_get_data_point_string(h, p, C.byref(q), C.byref(n), a.ref()) == 0
        assert np.array_equal(np.frombuffer(C.string_at(q, n.value), np.uint8), gst[f"{tag}_point{p}"]), p
        L.nmslib_free_string(q, a.ref())
    if space == "bit_hamming":
        for i in (0, 1, len(rows) - 1):
            sz = C.c_size_t()
            assert L.nmslib_get_data_point_size(h, i, C.byref(sz)) == 0
            buf = np.zeros(sz.value, np.uint8)
            assert L.nmslib_get_data_point_fill(h, i, buf.ctypes.data, sz.value) == 0
            np.testing.assert_array_equal(buf.view(np.uint32), string_ref.bit_object(rows[i]))
    assert L.nmslib_index_memory_usage(h) == int(gst[f"{tag}_memory"][0])   # before any upload: no HBM copy yet
    L.nmslib_index_destroy(h)
    assert len(a.live) == 0


def test_input_errors_leave_the_index_unchanged():
    L = nz.lib()
    rc, h, a = create("leven")
    assert add_strings(h, [b"abc", b"de"]) == 0
    assert add_strings(h, [b"fgh", b""]) == 2                        # empty leven string: refused, batch not stored
    assert L.nmslib_data_qty(h) == 2
    assert L.nmslib_add_data_point(h, b"\0", 1, 5) == 2              # element_count 1 -> 0 bytes
    arr = (C.c_char_p * 2)(b"ok", None)
    assert L.nmslib_add_data_point_batch_string(h, C.cast(arr, C.c_void_p), 2, None) == 1
    assert L.nmslib_data_qty(h) == 2
    L.nmslib_index_destroy(h)

    rc, h, a = create("bit_hamming")
    assert add_strings(h, [b"0 1 1", b"1,0,0"]) == 0
    assert add_strings(h, [b"1 1 1", b"1 2 0"]) == 13                # only 0 and 1: the reference's parse error code
    assert add_strings(h, [b"1 1 1", b"1 1 1 1"]) == 2               # bit count differs from the index's
    assert add_strings(h, [b"", b"1 1 1"]) == 2                       # no bits
    assert add_strings(h, [b"label:x 1 0 1"]) == 13                   # malformed label
    assert L.nmslib_data_qty(h) == 2
    assert add_strings(h, [b"label:7 1:0,1 trailing words ignored", b"  0 0 1\t"]) == 0
    assert L.nmslib_data_qty(h) == 4
    sz = C.c_size_t()
    assert L.nmslib_get_data_point_size(h, 2, C.byref(sz)) == 0 and sz.value == 8
    buf = np.zeros(2, np.uint32)
    assert L.nmslib_get_data_point_fill(h, 2, buf.ctypes.data, 8) == 0
    assert buf.tolist() == [0b101, 3]
    L.nmslib_index_destroy(h)


def test_parser_rules():
    assert string_ref.parse_bits("label:3 0,1:1 1 x 0") == [0, 1, 1, 1]
    assert string_ref.parse_bits(b"1 0\0 1") == [1, 0]
    with pytest.raises(string_ref.ParseError):
        string_ref.parse_bits("0 1 3")
    w = string_ref.bit_object("1 " * 33)
    assert w.tolist() == [0xFFFFFFFF, 1, 33]


def test_string_index_is_one_gpu_and_not_saved(tmp_path):
    L = nz.lib()
    rc, h, a = create("leven")
    assert add_strings(h, [b"abc"]) == 0
    p = nz.Params(a, gpu_shards=2)
    assert L.nmslib_create_index(h, p.h, 0) == 8
    p.free()
    L.nmslib_index_destroy(h)
    rc, h, a = create("leven")
    assert add_strings(h, [b"abc"]) == 0
    assert build_deferred(h, a) == 0
    assert L.nmslib_save_index(h, str(tmp_path / "s.idx").encode(), 1) == 10
    L.nmslib_index_destroy(h)


def test_python_binding_string_forms():
    idx = nz.Index("leven", "seq_search", data_type="ObjectAsString", dist_type="Int")
    idx.addStringBatch(["hello", b"world"], ids=[3, 4])
    idx.buildIndex(gpu_defer=1)
    assert idx.dataQty() == 2
    assert idx.getDataPoint(1) == b"world"
    assert idx.getDataPointString(0) == b"hello\0"
    idx.close()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_string_kernels_use_no_scratch(tmp_path):
    """Every kernel of string_kernels.hip and sparse_kernels.hip keeps its state in registers and LDS: no private
    segment, no scratch_ ops.  (sparse_kernels.hip as the library builds it: -ffp-contract=off; its 7 spaces come as
    two k-NN scans, one distance and one pair kernel each.)"""
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for name, flags, least in (("string_kernels.hip", [], 9), ("sparse_kernels.hip", ["-ffp-contract=off"], 28)):
        src = os.path.join(root, "nmslib_zig_amd", "csrc", "kernels", name)
        asm = str(tmp_path / (name + ".s"))
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed",
                               *flags, "-S", "--cuda-device-only", src, "-o", asm], stderr=subprocess.DEVNULL)
        text = open(asm).read()
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", text)
        assert len(sizes) >= least and all(s == "0" for s in sizes), (name, sizes)
        assert "scratch_" not in text, name
