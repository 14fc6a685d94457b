"""No GPU: the query-time parameter gpu_inwalk through the C ABI on indexes whose upload is deferred; the routing and LDS
arithmetic of the in-walk kernel (nmslib_zig_amd/csrc/hnsw_inwalk_plan.hpp) in a stand-alone program built with the host
sanitizers; and the sequential restatement of the rule (tests/inwalk_ref.py) on the host-built graphs the GPU tests use
(indexThreadQty=1 is deterministic): it returns only eligible rows, in (distance, position) order, and shows each case's
witness.

Rows per case: the smallest of tests/batched_ref.ROWS at which the witness shows.  Counters reached (70 queries, efSearch
32, k 10, M 8 unless the case says otherwise):

  filter-1in8       2500  310 eligible rows; every count is k; 15 182 expansions after W was full
  far-cluster       2500  40 eligible rows around row 7 (20 queries): C reaches 1024 entries and drops some
  tombstones        2500  2156 rows deleted, no filter: every count is k         tombstones-filter: 313 eligible rows
  cosinesimil       1000  unit rows: 27 730 admitted keys tie, 5674 pops at the bound   l2sqr_sift: 13 867 and 215
  l1 / linf / negdotprod 1000  ties 4488 / 20 481 / 38
  wide-m64 / m100    600  level-0 lists of 128 / 200 entries (delaunay_type 0 fills them)
  k-above-ef        2500  k = 40: cap is k                                       ef-k-1: cap 1
  ef-1024-dry       1500  754 eligible rows below cap 1024 (8 queries): W never fills, the walk ends on an empty C
"""
import os
import subprocess

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import inwalk_ref as ir
from tests.gpuutil import make_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X = np.random.default_rng(5).standard_normal((60, 12)).astype(np.float32)
HNSW = dict(M=6, efConstruction=20, indexThreadQty=1, gpu_defer=1)
INVALID_ARGUMENT = 2


def refused(fn, *needles):
    with pytest.raises(nz.NmslibError) as ei:
        fn()
    assert ei.value.code == INVALID_ARGUMENT, ei.value
    for s in needles:
        assert s in str(ei.value), ei.value


@pytest.mark.parametrize("space", ["l2", "cosinesimil", "l2sqr_sift"])
def test_zero_and_one_are_accepted_and_the_value_stays(space):
    rows = np.random.default_rng(6).integers(0, 255, (40, 128)).astype(np.uint8) if space == "l2sqr_sift" else X
    idx = make_index(space, "hnsw", rows, **HNSW)
    idx.setQueryTimeParams(gpu_inwalk=1)
    idx.setQueryTimeParams(efSearch=40)                          # the extension stays as set
    idx.setQueryTimeParams(efSearch=40, gpu_inwalk=0)
    idx.setQueryTimeParams(gpu_inwalk="1", algoType="old")
    idx.close()


def test_other_values_are_refused_with_a_reason():
    idx = make_index("l2", "hnsw", X, **HNSW)
    for bad in (2, -1, "on"):
        refused(lambda: idx.setQueryTimeParams(gpu_inwalk=bad), "gpu_inwalk", "0 or 1", str(bad))
    refused(lambda: idx.setQueryTimeParams(efSearch=40, gpu_inwalk=1.5), "gpu_inwalk")
    idx.setQueryTimeParams(gpu_inwalk=1)                         # the index still takes good values
    idx.close()


@pytest.mark.parametrize("method", ["brute_force", "seq_search"])
def test_the_exact_scan_refuses_it_as_an_unknown_parameter(method):
    idx = make_index("l2", method, X, gpu_defer=1)
    with pytest.raises(nz.NmslibError) as ei:
        idx.setQueryTimeParams(gpu_inwalk=1)
    assert ei.value.code != INVALID_ARGUMENT and "Unknown parameters" in str(ei.value), ei.value
    idx.close()


def test_a_string_graph_refuses_it_as_an_unknown_parameter():
    s = nz.Index("leven", "hnsw", data_type="ObjectAsString", dist_type="Int")
    s.addStringBatch(["kitten", "sitting", "mitten", "fitting", "bitten", "knitting", "written", "smitten"])
    s.buildIndex(M=4, efConstruction=10, indexThreadQty=1, gpu_defer=1)
    with pytest.raises(nz.NmslibError) as ei:
        s.setQueryTimeParams(gpu_inwalk=1)
    assert "Unknown parameters" in str(ei.value), ei.value
    s.close()


def test_the_documents_name_the_parameter_and_the_path():
    header = open(os.path.join(ROOT, "include", "nmslib_gpu.h")).read()
    assert "gpu_inwalk" in header and "8 = " in header
    assert "gpu_inwalk" in nz.Index.setQueryTimeParams.__doc__


def test_plan_header_standalone_under_host_sanitizers(tmp_path):
    """tests/hnsw_inwalk_plan_check.cpp includes csrc/hnsw_inwalk_plan.hpp alone (no HIP, nothing of the engine)."""
    exe = str(tmp_path / "hnsw_inwalk_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "hnsw_inwalk_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "inwalk plan ok" in run.stdout, run.stdout + run.stderr
    assert f"{6 + 9 + 5 + 5 + 4} cases" in run.stdout, run.stdout


@pytest.mark.parametrize("name", list(ir.CASES))
def test_restatement_returns_eligible_rows_in_order_and_shows_the_witness(name):
    space, Xc, Q, ids, build, ef, k, allow, dead, witness = ir.case(name)
    g = ir.host_graph(name)
    want = ir.restated(name)
    (oi, od, cnt), (ndc, hops, hops_up), wit = want
    eligible = ir.eligible_of(len(Xc), allow, dead)
    print(f"{name}: n={len(Xc)} eligible={int(eligible.sum())} counts {cnt.min()}..{cnt.max()} mean ndc {ndc.mean():.0f} "
          f"hops {hops.mean():.0f} witness {wit}")
    ir.check_witness(name, g, want, wit, eligible, k, ef)
    pos_of = {int(e): p for p, e in enumerate(ids)}
    for q in range(len(Q)):
        c = int(cnt[q])
        assert (oi[q, c:] == -1).all() and np.isposinf(od[q, c:]).all()
        pos = np.array([pos_of[int(e)] for e in oi[q, :c]], np.int64)
        assert eligible[pos].all(), (name, q)
        assert len(set(pos.tolist())) == c
        # the distances are the rows' own, and the order is (distance, position)
        np.testing.assert_array_equal(od[q, :c], ir.distance_fn(space, Xc, Q[q])(pos))
        keys = list(zip(od[q, :c].tolist(), pos.tolist()))
        assert keys == sorted(keys), (name, q)
        assert 0 < hops[q] <= ndc[q] and hops_up[q] >= g["maxlevel"]
    # a walk that fills W found no fewer eligible rows than it returns; with every row eligible and a wide cap the answer is the
    # exact one (a check of the restatement against a plain scan)
    if name == "filter-1in8":
        every = np.ones(len(Xc), bool)
        (ei, ed, ec), _, _ = ir.search(space, Xc, Q[:5], g, k, 1024, every, ids)
        for q in range(5):
            d = ir.distance_fn(space, Xc, Q[q])(np.arange(len(Xc)))
            order = np.lexsort((np.arange(len(Xc)), d))[:k]
            np.testing.assert_array_equal(ei[q], ids[order])
            np.testing.assert_array_equal(ed[q], d[order])
