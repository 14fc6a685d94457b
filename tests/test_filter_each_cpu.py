"""No GPU: the entries of the batch with one filter per query (nmslib_gpu_knn_query_batch_filtered_each and its _device
twin) through the C ABI on indexes whose upload is deferred (gpu_defer=1): what is declared and bound, NULL handling, the
range check of filter_of_query, the indexes that are refused, and that a batch of unfiltered queries which gets as far as
needing a device fails with the usual error and leaks nothing.  The batch plan (csrc/filter_batch_plan.hpp) is compiled
alone and compared with numpy's stable argsort on the (segment, filter) key."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests.gpuutil import make_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = np.random.default_rng(13).standard_normal((70, 12)).astype(np.float32)
HNSW = dict(M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1)
NULL_POINTER, INVALID_ARGUMENT, SPACE_INCOMPATIBLE, QUERY_EXECUTION_FAILED = 1, 2, 5, 9
NAMES = ("nmslib_gpu_knn_query_batch_filtered_each", "nmslib_gpu_knn_query_batch_filtered_each_device")
BOTH = [("hnsw", HNSW), ("brute_force", dict(gpu_defer=1))]


class Call:
    """the arguments of one call, every one replaceable; the outputs hold sentinels"""

    def __init__(self, idx, nq=3, fq=None):
        self.idx = idx
        self.q = np.zeros((max(nq, 1), 12), np.float32)
        self.fq = np.full(max(nq, 1), -1, np.int32) if fq is None else np.asarray(fq, np.int32)
        self.nq = nq
        self.ids = np.full((max(nq, 1), 2), 77, np.int32)
        self.ds = np.full((max(nq, 1), 2), 77, np.float32)
        self.cnt = np.full(max(nq, 1), 77, np.int32)
        self.routes = np.full(max(nq, 1), 77, np.int32)
        self.filters = (C.c_void_p * 2)(None, None)

    def args(self, device, **over):
        a = dict(index=self.idx.h, filters=None, n_filters=0, fq=self.fq.ctypes.data, queries=self.q.ctypes.data, nq=self.nq,
                 dim=12, k=2, ids=self.ids.ctypes.data, ds=self.ds.ctypes.data, cnt=self.cnt.ctypes.data,
                 routes=self.routes.ctypes.data)
        a.update(over)
        out = [a[n] for n in ("index", "filters", "n_filters", "fq", "queries", "nq", "dim", "k", "ids", "ds", "cnt", "routes")]
        return out + [None] if device else out

    def run(self, device=False, **over):
        fn = getattr(nz.lib(), NAMES[1 if device else 0])
        rc = fn(*self.args(device, **over))
        return rc, nz.last_error_detail(self.idx.alloc)

    def untouched(self):
        return all((a == 77).all() for a in (self.ids, self.ds, self.cnt, self.routes))


def test_both_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(nz.__file__), "..", "include", "nmslib_gpu.h")).read()
    for name in NAMES:
        assert name + "(" in header and name in nz.ABI_SYMBOLS_GPU
        assert getattr(nz.lib(), name).argtypes is not None
    assert "9 = a batch with one" in header                       # last_path of such a batch
    assert callable(nz.Index.knnQueryBatchEachFiltered) and callable(nz.Index.knn_device_each_filtered)


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("method,params", BOTH)
def test_null_handling(method, params, device):
    idx = make_index("l2", method, X, **params)
    c = Call(idx)
    for name in ("index", "fq", "queries", "ids", "ds"):
        rc, msg = c.run(device, **{name: None})
        assert rc == NULL_POINTER, (name, rc, msg)
    rc, msg = c.run(device, filters=None, n_filters=1)
    assert rc == NULL_POINTER and "filters" in msg, (rc, msg)
    for name in ("k", "dim"):
        assert c.run(device, **{name: 0})[0] == INVALID_ARGUMENT
    assert c.untouched()
    idx.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("method,params", BOTH)
def test_filter_of_query_is_checked_before_a_device_is_needed(method, params, device):
    idx = make_index("l2", method, X, **params)
    live = len(idx.alloc.live)
    rc, msg = Call(idx, fq=[-1, 0, -1]).run(device)               # n_filters = 0: entry 0 names no filter
    assert rc == INVALID_ARGUMENT and "filter_of_query[1] = 0" in msg and "[-1, 0)" in msg, (rc, msg)
    c = Call(idx, fq=[-1, 1, 2])
    rc, msg = c.run(device, filters=c.filters, n_filters=2)
    assert rc == INVALID_ARGUMENT and "filter_of_query[2] = 2" in msg and "[-1, 2)" in msg, (rc, msg)
    rc, msg = Call(idx, fq=[-1, -1, -2]).run(device)
    assert rc == INVALID_ARGUMENT and "filter_of_query[2] = -2" in msg, (rc, msg)
    # a NULL handle in filters is no filter of this index; the message says which entry
    c = Call(idx, fq=[-1, 0, 0])
    rc, msg = c.run(device, filters=c.filters, n_filters=2)
    assert rc == INVALID_ARGUMENT and "filters[0]" in msg and c.untouched(), (rc, msg)
    with pytest.raises(nz.NmslibError) as ei:
        idx.knnQueryBatchEachFiltered([], [0], X[:1], 2)
    assert ei.value.code == INVALID_ARGUMENT and "filter_of_query[0] = 0" in str(ei.value)
    with pytest.raises(ValueError):
        idx.knnQueryBatchEachFiltered([], [-1, -1], X[:1], 2)     # one entry per query
    assert len(idx.alloc.live) == live
    idx.close()


@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("method,params", BOTH)
def test_an_empty_batch_succeeds_and_writes_nothing(method, params, device):
    idx = make_index("l2", method, X, **params)
    c = Call(idx, nq=0)
    rc, msg = c.run(device)
    assert rc == 0 and c.untouched(), (rc, msg)
    idx.close()


def refused(idx, qdim=12):
    """the refusal of nmslib_gpu_filter_create, in its words"""
    f = C.c_void_p()
    bits = np.full(3, 0xFFFFFFFF, np.uint32)
    assert nz.lib().nmslib_gpu_filter_create(idx.h, bits.ctypes.data, 3, 0, C.byref(f)) == SPACE_INCOMPATIBLE
    want = nz.last_error_detail(idx.alloc)
    for device in (False, True):
        c = Call(idx)
        rc, msg = c.run(device)
        assert rc == SPACE_INCOMPATIBLE and c.untouched(), (rc, msg)
        assert msg.split(": ", 1)[1] == want.split(": ", 1)[1], (msg, want)   # (behind each entry's own prefix)
        assert "takes no filter" in msg
    idx.close()


def test_sparse_string_divergence_and_sharded_indexes_are_refused_without_a_device():
    s = nz.Index("l2_sparse", "seq_search", data_type="SparseVector")
    s.addSparseBatch([([1, 2], [1.0, 1.0]), ([2, 5], [1.0, 2.0])])
    refused(s)
    w = nz.Index("leven", "brute_force", data_type="ObjectAsString", dist_type="Int")
    w.addStringBatch(["kitten", "sitting", "mitten"])
    refused(w)
    d = nz.Index("kldivgenfast", "seq_search")
    d.addDenseBatch(np.abs(X) + 0.1)
    refused(d)
    refused(make_index("l2", "brute_force", X, gpu_defer=1, gpu_shards=2))
    refused(make_index("l2", "hnsw", X, gpu_shards=2, **HNSW))


@pytest.mark.parametrize("method,params", BOTH)
def test_an_unfiltered_batch_needs_a_device_and_leaks_nothing(method, params):
    """Without a device: the usual "no HIP device" error.  (With one the batch is answered as knnQueryBatch answers it.)"""
    idx = make_index("l2", method, X, **params)
    live = len(idx.alloc.live)
    c = Call(idx)
    c.q[:] = X[:3]
    rc, msg = c.run()
    if nz.lib().nmslib_gpu_device_count() == 0:
        assert rc == QUERY_EXECUTION_FAILED and "no HIP device" in msg and c.untouched(), (rc, msg)
        with pytest.raises(nz.NmslibError) as ei:
            idx.knnQueryBatchEachFiltered([], [-1, -1, -1], X[:3], 2)
        assert "no HIP device" in str(ei.value)
    else:
        assert rc == 0, (rc, msg)
        want = idx.knnQueryBatch(X[:3], 2)
        np.testing.assert_array_equal(c.ids, want[0])
        np.testing.assert_array_equal(c.cnt, want[2])
    assert len(idx.alloc.live) == live
    idx.close()


# ---- the batch plan ----------------------------------------------------------------------------------------------------
def plan_cases():
    """(name, filter_of_query, segment of every filter: 1 walk, 2 subset)"""
    rng = np.random.default_rng(5)
    mixed, walk = [1, 2, 1, 2, 2, 1], [1] * 6
    cases = []
    for tag, seg in (("mixed", mixed), ("same", walk)):
        cases += [
            (f"empty-{tag}", [], seg),
            (f"one-{tag}", [3], seg),
            (f"one-unfiltered-{tag}", [-1], seg),
            (f"all-one-filter-{tag}", [4] * 9, seg),
            (f"interleaved-{tag}", list(np.arange(40) % 7 - 1), seg),
            (f"reversed-{tag}", [5, 5, 4, 3, 3, 2, 1, 0, -1, -1], seg),
            (f"unused-filter-{tag}", [0, 2, 0, 2, -1, 5], seg),   # 1, 3 and 4 have no query
            (f"random-{tag}", list(rng.integers(-1, 6, 300)), seg),
        ]
    # in plan order already: the identity must be flagged
    cases.append(("sorted-mixed", [-1, -1, 0, 0, 2, 5, 1, 3, 3, 4], mixed))
    cases.append(("sorted-same", [-1, 0, 0, 1, 2, 3, 3, 4, 5], walk))
    cases.append(("no-filters", [-1] * 5, []))
    return cases


def test_batch_plan_header_standalone_equals_a_stable_argsort(tmp_path):
    """tests/filter_batch_plan_check.cpp includes csrc/filter_batch_plan.hpp alone (no HIP, nothing of the engine) and prints,
    per case read from a file, the permutation, its inverse, the segment bounds, the groups and the identity flag; the
    checker is built with the host sanitizers and run on its own"""
    exe = str(tmp_path / "filter_batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "filter_batch_plan_check.cpp"), "-o", exe])
    cases = plan_cases()
    src = tmp_path / "cases.txt"
    with open(src, "w") as f:
        f.write(f"{len(cases)}\n")
        for _, fq, seg in cases:
            f.write(f"{len(fq)} {len(seg)}\n{' '.join(map(str, fq))}\n{' '.join(map(str, seg))}\n")
    run = subprocess.run([exe, str(src)], capture_output=True, text=True)
    assert run.returncode == 0 and "filter batch plan ok" in run.stdout, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    row = lambda s: [int(v) for v in s.split()[1:]]               # noqa: E731
    assert len(lines) == 5 * len(cases) + 1
    for i, (name, fq, seg) in enumerate(cases):
        perm, inv, segs, groups, ident = (row(s) for s in lines[5 * i:5 * i + 5])
        fq, seg = np.array(fq, np.int64), np.array(seg, np.int64)
        segq = np.where(fq < 0, 0, np.r_[seg, 0][np.maximum(fq, 0)]) if len(fq) else np.zeros(0, np.int64)
        want = np.argsort(segq * 100 + fq, kind="stable")
        assert perm == list(want), name
        assert [inv[q] for q in perm] == list(range(len(fq))), name
        assert segs == [0] + [int((segq <= s).sum()) for s in (0, 1, 2)], name
        assert ident == [int((want == np.arange(len(fq))).all())], name
        # the groups: (filter, begin, end) of every filter with queries, in plan order
        sf = fq[want]
        g_want = []
        for p in range(len(sf)):
            if sf[p] >= 0 and (p == 0 or sf[p - 1] != sf[p]):
                g_want += [int(sf[p]), p, p + int((sf == sf[p]).sum())]
        assert groups == g_want, name
    ident = {name: row(lines[5 * i + 4])[0] for i, (name, _, _) in enumerate(cases)}
    assert ident["sorted-mixed"] == 1 and ident["sorted-same"] == 1 and ident["reversed-mixed"] == 0
    assert ident["empty-mixed"] == 1 and ident["one-mixed"] == 1 and ident["all-one-filter-same"] == 1
