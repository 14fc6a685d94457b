"""No GPU: the batched range query (nmslib_gpu_range_query_batch and its _device twin) through the C ABI on
indexes whose upload is deferred (gpu_defer=1): what is declared and bound, every refusal that needs no device with its
code, its message and untouched outputs; and the plan (csrc/range_batch_plan.hpp) compiled alone under the host sanitizers
against its restatement tests/range_batch_plan_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import range_batch_plan_ref as rbp
from tests.gpuutil import make_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = np.random.default_rng(17).standard_normal((70, 12)).astype(np.float32)
NULL_POINTER, INVALID_ARGUMENT, SPACE_INCOMPATIBLE, INDEX_BUILD_FAILED = 1, 2, 5, 8
NAMES = ("nmslib_gpu_range_query_batch", "nmslib_gpu_range_query_batch_device")
HNSW = dict(M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1)


class Call:
    """the arguments of one call, every one replaceable; the outputs hold sentinels"""

    def __init__(self, idx, nq=3, dim=12, dtype=np.float32):
        self.idx, self.nq, self.dim = idx, nq, dim
        self.q = np.zeros((max(nq, 1), dim), dtype)
        self.radii = np.ones(max(nq, 1), np.float64)
        self.ids = np.full((max(nq, 1), 4), 77, np.int32)
        self.ds = np.full((max(nq, 1), 4), 77, np.float32)
        self.cnt = np.full(max(nq, 1), 77, np.int32)
        self.tot = np.full(max(nq, 1), 77, np.int32)

    def run(self, device=False, **over):
        a = dict(index=self.idx.h if self.idx is not None else None, queries=self.q.ctypes.data, nq=self.nq, dim=self.dim,
                 radii=self.radii.ctypes.data, capacity=4, ids=self.ids.ctypes.data, ds=self.ds.ctypes.data,
                 cnt=self.cnt.ctypes.data, tot=self.tot.ctypes.data)
        a.update(over)
        args = [a[n] for n in ("index", "queries", "nq", "dim", "radii", "capacity", "ids", "ds", "cnt", "tot")]
        rc = getattr(nz.lib(), NAMES[1 if device else 0])(*(args + [None] if device else args))
        return rc, nz.last_error_detail(self.idx.alloc) if self.idx is not None else ""

    def untouched(self):
        return all((a == 77).all() for a in (self.ids, self.ds, self.cnt, self.tot))


def test_both_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(os.path.dirname(nz.__file__), "..", "include", "nmslib_gpu.h")).read()
    flat = " ".join(header.split())
    assert ("nmslib_error_t nmslib_gpu_range_query_batch(nmslib_index_handle_t index, const void* queries, size_t query_count, "
            "size_t elem_count, const double* radii, size_t capacity, int32_t* ids, float* dists, int32_t* counts, "
            "int32_t* totals);") in flat
    assert ("nmslib_error_t nmslib_gpu_range_query_batch_device(nmslib_index_handle_t index, const void* d_queries, "
            "size_t query_count, size_t elem_count, const double* radii, size_t capacity, int32_t* d_ids, float* d_dists, "
            "int32_t* d_counts, int32_t* d_totals, void* stream);") in flat
    for name, nargs in zip(NAMES, (10, 11)):
        assert name in nz.ABI_SYMBOLS_GPU
        assert len(getattr(nz.lib(), name).argtypes) == nargs
    assert "9 = a batch with one" in header and "10 = a batched" in flat and "11 = a batched" in flat
    assert callable(nz.Index.rangeQueryBatch) and callable(nz.Index.range_device)


@pytest.mark.parametrize("device", [False, True])
def test_null_pointers_and_arguments(device):
    idx = make_index("l2", "brute_force", X, gpu_defer=1)
    c = Call(idx)
    for name in ("index", "queries", "radii", "ids", "ds"):
        rc, msg = c.run(device, **{name: None})
        assert rc == NULL_POINTER, (name, rc, msg)
    # counts and totals may be NULL with a capacity; count only needs totals; then ids and dists may be NULL
    rc, msg = c.run(device, capacity=0, tot=None)
    assert rc == INVALID_ARGUMENT and "totals" in msg, (rc, msg)
    rc, msg = c.run(device, capacity=0, tot=None, ids=None, ds=None)
    assert rc == INVALID_ARGUMENT, (rc, msg)
    # a query length other than the index's
    for dim in (11, 13, 0):
        rc, msg = c.run(device, dim=dim)
        assert rc == INVALID_ARGUMENT and "query length" in msg and "12" in msg, (dim, rc, msg)
    assert c.untouched()
    with pytest.raises(nz.NmslibError) as ei:
        idx.rangeQueryBatch(X[:2, :11], 1.0, 4)
    assert ei.value.code == INVALID_ARGUMENT
    idx.close()


@pytest.mark.parametrize("device", [False, True])
def test_an_empty_batch_succeeds_and_writes_nothing(device):
    idx = make_index("l2", "brute_force", X, gpu_defer=1)
    c = Call(idx, nq=0)
    rc, msg = c.run(device)
    assert rc == 0 and c.untouched(), (rc, msg)
    idx.close()


@pytest.mark.parametrize("device", [False, True])
def test_an_index_that_was_never_built(device):
    idx = nz.Index("l2", "brute_force")
    idx.addDenseBatch(X)
    c = Call(idx)
    rc, msg = c.run(device)
    assert rc == INDEX_BUILD_FAILED and "Index not built" in msg and c.untouched(), (rc, msg)
    idx.close()


@pytest.mark.parametrize("device", [False, True])
def test_hnsw_is_refused_in_the_single_entrys_words(device):
    idx = make_index("l2", "hnsw", X, **HNSW)
    with pytest.raises(nz.NmslibError) as ei:
        idx.rangeQueryFill(X[0], 1.0, 4)
    single = str(ei.value)
    assert ei.value.code == SPACE_INCOMPATIBLE and "Range search is not supported!" in single
    c = Call(idx)
    rc, msg = c.run(device)
    assert rc == SPACE_INCOMPATIBLE and "Range query not supported by method: Range search is not supported!" in msg, (rc, msg)
    assert c.untouched()
    idx.close()


@pytest.mark.parametrize("device", [False, True])
def test_sparse_string_and_divergence_indexes_are_refused_without_a_device(device):
    s = nz.Index("l2_sparse", "seq_search", data_type="SparseVector")
    s.addSparseBatch([([1, 2], [1.0, 1.0]), ([2, 5], [1.0, 2.0])])
    s.buildIndex(gpu_defer=1)
    w = nz.Index("leven", "brute_force", data_type="ObjectAsString", dist_type="Int")
    w.addStringBatch(["kitten", "sitting", "mitten"])
    w.buildIndex(gpu_defer=1)
    d = nz.Index("kldivgenfast", "seq_search")
    d.addDenseBatch(np.abs(X) + 0.1)
    d.buildIndex(gpu_defer=1)
    for idx in (s, w, d):
        c = Call(idx)
        rc, msg = c.run(device)
        assert rc == SPACE_INCOMPATIBLE and c.untouched(), (rc, msg)
        for word in ("l2, l1, linf, cosinesimil, angulardist, negdotprod", "l2sqr_sift", "nmslib_range_query_fill"):
            assert word in msg, msg
        idx.close()


def test_the_device_entry_refuses_an_index_that_asked_for_shards():
    idx = make_index("l2", "brute_force", X, gpu_defer=1, gpu_shards=2)
    c = Call(idx)
    rc, msg = c.run(True)
    assert rc == SPACE_INCOMPATIBLE and "one device" in msg and c.untouched(), (rc, msg)
    idx.close()


def test_a_batch_needs_a_device_and_leaks_nothing():
    """Without a device the usual "no HIP device" error and untouched outputs; with one, the single entry's rows."""
    idx = make_index("l2", "brute_force", X, gpu_defer=1)
    live = len(idx.alloc.live)
    c = Call(idx)
    c.q[:] = X[:3]
    c.radii[:] = 3.0
    rc, msg = c.run()
    if nz.lib().nmslib_gpu_device_count() == 0:
        assert rc != 0 and "no HIP device" in msg and c.untouched(), (rc, msg)
    else:
        assert rc == 0, (rc, msg)
        for q in range(3):
            ids, ds = idx.rangeQueryFill(X[q], 3.0, 4)
            assert c.cnt[q] == len(ids) and (c.ids[q, :len(ids)] == ids).all()
    assert len(idx.alloc.live) == live
    idx.close()


# ---- the plan --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def printed_plans(tmp_path_factory):
    """tests/range_batch_plan_check.cpp includes the header alone, is built with the host sanitizers and run as its own
    program; it asserts the invariants (workspace <= budget, the slices cover every query once, the grid every row once)"""
    exe = str(tmp_path_factory.mktemp("range_batch_plan") / "range_batch_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "range_batch_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "range batch plan ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    return run.stdout.splitlines()


def test_restatement_equals_the_header_on_the_grid(printed_plans):
    want = [rbp.line(pt) for pt in rbp.grid()]
    assert printed_plans[-2] == f"{len(want)} cases"
    assert printed_plans[:-2] == want


def test_the_grid_holds_both_sides_of_every_switch():
    pts = list(rbp.grid())
    plans = {pt: rbp.plan(*pt) for pt in pts}
    by = lambda **kw: [p for pt, p in plans.items()                                             # noqa: E731
                       if all(dict(zip(("n", "dim", "elem", "nq", "cap", "budget"), pt))[k] == v for k, v in kw.items())]
    # the largest batched dimension and one more; bytes that are no sift rows
    assert {p.route for p in by(dim=rbp.MAX_DIM, elem=4, nq=33, budget=rbp.WS_BYTES)} == {10}
    assert {p.route for p in by(dim=rbp.MAX_DIM + 1, elem=4, nq=33)} == {11}
    assert {p.route for p in by(dim=64, elem=1)} == {11}
    assert {p.chunks for p in by(elem=4, nq=33, budget=rbp.WS_BYTES) if p.route == 10} == {1, 2, 3, 4}
    # one slice, two slices, a ragged last one; a budget below one query's masks goes to route 11
    for n in (63, 64, 65, 1023, 1024, 1025):
        assert n in rbp.GRID_N
        b = rbp.query_bytes(n)
        assert rbp.plan(n, 5, 4, 33, 128, b // 2).route == 11
        assert rbp.slice_sizes(rbp.plan(n, 5, 4, 33, 128, b), 33) == [1] * 33
        assert rbp.slice_sizes(rbp.plan(n, 5, 4, 33, 128, 2 * b), 33) == [2] * 16 + [1]
        assert rbp.slice_sizes(rbp.plan(n, 5, 4, 33, 128, 5 * b // 2), 33) == [2] * 16 + [1]
        assert rbp.slice_sizes(rbp.plan(n, 5, 4, 64, 128, 2 * b), 64) == [2] * 32
        assert rbp.slice_sizes(rbp.plan(n, 5, 4, 33, 128), 33) == [33]
        assert all(pt in plans for pt in ((n, 5, 4, 33, 128, b), (n, 5, 4, 33, 128, 5 * b // 2), (n, 5, 4, 33, 128, b // 2)))
    assert [rbp.plan(n, 5, 4, 1, 1).mask_words for n in (63, 64, 65)] == [1, 1, 2]
    assert [rbp.plan(n, 5, 4, 1, 1).blocks for n in (1023, 1024, 1025)] == [1, 1, 2]
    assert [rbp.plan(n, 5, 4, 1, 1).grid_x for n in (255, 256, 257)] == [1, 1, 2]
    # Q at tile - 1, tile, tile + 1: the query splits of a small index follow the tiles
    T = rbp.QUERY_TILE
    assert all(q in rbp.GRID_Q for q in (T - 1, T, T + 1))
    assert [rbp.plan(1025, 5, 4, q, 1).grid_y for q in (T - 1, T, T + 1, 2 * T + 1)] == [1, 1, 2, 3]
    assert rbp.plan(1000000, 128, 4, 1024, 128).grid_y == 1 and rbp.plan(1000000, 128, 4, 1024, 128).slices == 1
    # the cap of a slice
    assert rbp.slice_sizes(rbp.plan(1, 5, 4, 32769, 1), 32769) == [32768, 1]
    assert rbp.plan(1000000, 128, 4, 1024, 0).count_only == 1
