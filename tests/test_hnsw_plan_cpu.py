"""The launch layer of the dense HNSW search without a GPU: the Python restatement (tests/hnsw_plan_ref.py) against the C++
planners on a grid, the plans' invariants, the switches one by one, what no input reaches, the route of every case of
tests/hnsw_edge_cases.py, the conditions on those cases' inputs from the oracle alone, and the checkers against corrupted
answers."""
import os
import subprocess

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import hnsw_edge_cases as hec, hnsw_plan_ref as hpr, refio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRID_CAP = (1, 56, 57, 64, 65, 113, 114, 128, 129, 227, 228, 256, 257, 1024, 1025, 2048, 2049, 8192, 8193)
GRID_M0 = (4, 12, 16, 17, 32, 62, 63, 64, 126, 127, 128, 191, 192, 254, 255, 256, 300)
GRID_MORE_M = ((70, 20), (62, 20), (63, 20), (255, 100), (256, 100), (0, 0))
# 5760 / 5768: the LDS planner's table 4096 -> 2048; 13968 / 13976 and 14056 / 14064: its 64 KiB clause at cap 56 and 10;
# 16120 / 16128: the HBM-array kernel passes 64 KiB; 40584 / 40592 and 40696 / 40704: the LDS kernels (ef 56) and the
# HBM-array kernel pass a workgroup's LDS -- the largest rows the search accepts
GRID_LDV = (8, 128, 768, 1664, 4096, 5760, 5768, 6000, 9000, 13968, 13976, 14000, 14056, 14064, 16120, 16128, 16384, 40584,
            40592, 40696, 40704)
GRID_N = (1, 2, 2046, 2047, 2048, 100000)


@pytest.fixture(scope="module")
def printed_plans(tmp_path_factory):
    """tests/hnsw_plan_check.cpp includes kernels.hpp and compiles hnsw_plan.cpp as they are and prints both planners over
    the grid; built as a stand-alone program under the host sanitizers"""
    exe = str(tmp_path_factory.mktemp("hnsw_plan") / "hnsw_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "hnsw_plan_check.cpp"),
                           os.path.join(ROOT, "nmslib_zig_amd", "csrc", "hnsw_plan.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "hnsw plan ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    lds, old = {}, {}
    for line in run.stdout.splitlines():
        f = line.split()
        if f and f[0] == "L":
            lds[tuple(int(x) for x in f[1:9])] = tuple(int(x) for x in f[10:])
        elif f and f[0] == "O":
            old[tuple(int(x) for x in f[1:10])] = tuple(int(x) for x in f[11:])
    return lds, old


def _grid_points():
    for u8 in (0, 1):
        for n in GRID_N:
            for ldv in GRID_LDV:
                if n != 100000 and ldv != 128:
                    continue
                for cap in GRID_CAP:
                    for ef, k in ((cap, min(cap, 10)), (min(cap, 5), cap)):
                        for maxM, maxM0 in [(m0 // 2, m0) for m0 in GRID_M0] + list(GRID_MORE_M):
                            yield u8, n, ldv, maxM, maxM0, k, ef


def test_restatement_equals_the_planners_on_the_grid(printed_plans):
    lds, old = printed_plans
    points = sorted(set(_grid_points()))        # (cap 1: both ways to it are the same point)
    assert len(lds) == 2 * len(points) and len(old) == 4 * len(points)
    for u8, n, ldv, maxM, maxM0, k, ef in points:
        for force in (0, 1):
            at = (u8, n, ldv, maxM, maxM0, k, ef, force)
            p = hpr.make_plan(u8, n, ldv, maxM, maxM0, k, ef, bool(force))
            assert tuple(p) + (hpr.nbcap(maxM, maxM0), hpr.big_lds(u8, ldv, maxM, maxM0), int(hpr.wide(maxM, maxM0)),
                               hpr.emax_of(p.cap)) == lds[at], at
            for heap_cap in (0, n + 1):
                o = hpr.make_plan_old(u8, n, ldv, maxM, maxM0, k, ef, bool(force), heap_cap)
                assert tuple(o) == old[at + (heap_cap,)], at + (heap_cap,)


def test_plan_invariants_on_the_grid(printed_plans):
    lds, old = printed_plans
    for (u8, n, ldv, maxM, maxM0, k, ef, force), (cap, table, shift, words, lds_bytes, nbcap, big, wide, emax) in lds.items():
        at = (u8, n, ldv, maxM, maxM0, k, ef, force)
        # a narrow list is one word a lane: the count, up to 62 ids, one lane spare; the sorted array holds cap items
        assert wide == (max(maxM, maxM0) + 1 > 63) and (wide or nbcap == 64), at
        # ... in the narrowest of the three arrays that does (beyond 1024 the HBM-array kernel has none)
        assert (cap > 1024 or 64 * emax >= cap) and cap > 64 * {2: 0, 4: 2, 16: 4}[emax], at
        assert cap == max(ef, k) and nbcap % 64 == 0 and nbcap > max(maxM, maxM0) - 1 and nbcap >= 64, at
        # (a frontier array holds the longest list: 255 entries go to the 256-entry arrays, 256 to the HBM-array kernel)
        assert nbcap >= max(maxM, maxM0) and (nbcap <= hpr.NBCAP_LDS) == (max(maxM, maxM0) <= 255), at
        if table:
            assert not force and table >= 2048 and table & (table - 1) == 0 and shift == 32 - hpr.ilog2(table), at
            assert 18 * cap <= table // 2 and words == 0, at
            # (the smallest table is kept beyond the residency budget, up to 64 KiB)
            assert lds_bytes <= (hpr.LDS_BUDGET if table > 2048 else 64 * 1024), at
            # the one-wave kernel carves exactly the plan; the multi-wave kernel gets 16 bytes more and carves less
            assert hpr.carved_lds(u8, ldv, maxM, maxM0, cap, table) == lds_bytes, at
            if not hpr.wide(maxM, maxM0) and not u8:
                assert hpr.carved_mw(ldv, cap, table) <= lds_bytes + 16, at
        else:
            assert shift == 0 and words == (n + 31) // 32, at
            assert hpr.carved_lds(u8, ldv, maxM, maxM0, cap, 0) + 16 == lds_bytes, at
        assert hpr.carved_big(u8, ldv, maxM, maxM0) + 16 == big, at
    for (u8, n, ldv, maxM, maxM0, k, ef, force, asked), v in old.items():
        at = (u8, n, ldv, maxM, maxM0, k, ef, force, asked)
        o = hpr.OldPlan(*v)
        assert 0 <= o.heap_lds <= o.heap_cap <= n + 1 and o.heap_lds <= 2048, at
        assert o.heap_cap == (n + 1 if asked else min(32 * o.cap + 4096, n + 1)), at
        assert o.a_in_lds == (ef <= 8192) and o.r_in_lds == (k <= 2048), at
        assert o.ws_a >= 0 and o.ws_r >= 0 and o.ws_heap >= 0, at
        assert (o.ws_a == 0) == bool(o.a_in_lds) and (o.ws_r == 0) == bool(o.r_in_lds), at
        assert o.ws_heap == (o.heap_cap - o.heap_lds) * 8, at
        if o.table_size:
            assert o.table_size & (o.table_size - 1) == 0 and o.table_size >= 2048, at
            assert o.table_shift == 32 - hpr.ilog2(o.table_size) and 18 * o.cap <= o.table_size // 2, at
            assert o.lds_bytes <= hpr.OLD_BUDGET and o.table_size <= 8192, at
            assert hpr.carved_old(u8, ldv, maxM, maxM0, o, k, ef) == o.lds_bytes, at
        else:
            assert hpr.carved_old(u8, ldv, maxM, maxM0, o, k, ef) + 16 == o.lds_bytes, at


def test_every_launch_stays_within_what_it_asks_the_runtime_for():
    """Every launch function names its dynamic LDS to the runtime (hipFuncSetAttribute; the HBM-array kernel's did not and
    passes 64 KiB from 16 128 floats a row on) and refuses a plan beyond a workgroup's 160 KiB; the engine refuses rows that
    fit no kernel (hnsw_big_lds > HNSW_LDS_LIMIT, error 6).  So over the grid: a route is either launched within the limit or
    refused, and the rows the engine accepts are exactly those the HBM-array kernel can stage.  A batch on accepted rows whose
    own route passes the limit (the LDS kernels and SearchOld keep arrays next to the row) is refused by the engine with the
    same error 6 before any launch: Engine::hnsw_search_lds and knn_hnsw_old compare the plan's lds_bytes with the limit, as
    the restatement's route does here."""
    for ldv in GRID_LDV:
        for maxM0 in (16, 62, 64, 255, 256):
            accepted = hpr.big_lds(False, ldv, maxM0 // 2, maxM0) <= hpr.LDS_LIMIT
            for cap in GRID_CAP:
                for algo in ("v1merge", "old"):
                    r = hpr.route("l2", 2000, ldv, maxM0 // 2, maxM0, 64, 10, cap, algo)
                    launched = r.lds_bytes <= hpr.LDS_LIMIT
                    if not accepted:
                        assert not launched, (ldv, maxM0, cap, algo)      # nothing smaller than the HBM-array kernel
                    if r.family == "big":
                        assert launched == accepted
    # the edges, narrow lists
    assert hpr.big_lds(False, 16120, 8, 16) <= 64 * 1024 < hpr.big_lds(False, 16128, 8, 16)
    assert hpr.big_lds(False, 40696, 8, 16) <= hpr.LDS_LIMIT < hpr.big_lds(False, 40704, 8, 16)
    assert hpr.route("l2", 300, 40584, 8, 16, 64, 10, 56).lds_bytes <= hpr.LDS_LIMIT
    assert hpr.route("l2", 300, 40592, 8, 16, 64, 10, 56).lds_bytes > hpr.LDS_LIMIT
    assert hpr.route(hpr.SIFT, 300, 128, 8, 16, 64, 10, 8193, "old").lds_bytes <= 64 * 1024     # bytes: nothing grows
    # (a table plan, the only one the multi-wave kernel's 16 bytes more are asked for, stays within 64 KiB)
    assert all(hpr.route("l2", 2000, ldv, 8, 16, 64, 10, cap, mw="2").lds_bytes <= 64 * 1024 + 16
               for ldv in GRID_LDV for cap in GRID_CAP if hpr.route("l2", 2000, ldv, 8, 16, 64, 10, cap, mw="2").table)
    # SearchOld keeps its heap and queues next to the row: 300 rows, ef 56 pass the limit from 40 088 floats a row on
    assert [hpr.route("l2", 300, D, 8, 16, 64, 10, 56, "old").lds_bytes <= hpr.LDS_LIMIT for D in (40080, 40088)] == [True, False]
    # the refused cases stand past these edges, the case before them on it
    at_limit = [c for c in hec.LONG_CASES if c.name == "long_lds_at_limit"][0]
    assert hec.LONG_LDS_REFUSED.graph.D == at_limit.graph.D + 8
    assert hec.route_of(at_limit).lds_bytes <= hpr.LDS_LIMIT < hec.route_of(hec.LONG_LDS_REFUSED).lds_bytes
    assert hec.route_of(hec.LONG_OLD_REFUSED).lds_bytes > hpr.LDS_LIMIT
    assert hpr.big_lds(False, hec.LONG_LDS_REFUSED.graph.D, 8, 16) <= hpr.LDS_LIMIT


def _plan(cap, M=8, D=128, n=2000, space="l2", **kw):
    return hpr.route(space, n, D, M, 2 * M, 64, 10, cap, "v1merge", **kw)


def test_the_switches_fall_where_the_cases_stand():
    """the switches of the launch layer, one by one, from the restatement (which the grid test holds to the C++)"""
    tables = lambda M, caps: [_plan(c, M).table for c in caps]     # noqa: E731
    # the table / bitset choice is not monotone in cap: M = 8, D = 128 ...
    assert tables(8, (1, 56, 57, 64, 65, 113, 114, 128, 129, 227, 228)) == [2048, 2048, 0, 0, 4096, 4096, 0, 0, 8192, 8192, 0]
    # ... and M = 16
    assert tables(16, (1, 32, 33, 64, 65, 227, 228)) == [2048, 2048, 4096, 4096, 8192, 8192, 0]
    assert [hec.PLAN_M8[c][0] for c in hec.PLAN_M8] == tables(8, hec.PLAN_M8)
    assert [hec.PLAN_M16[c][0] for c in hec.PLAN_M16 if c <= 1024] == tables(16, [c for c in hec.PLAN_M16 if c <= 1024])
    # bytes: the same flips
    assert [_plan(c, space=hpr.SIFT).table for c in (56, 57, 227, 228)] == [2048, 0, 8192, 0]
    # long rows shrink the table: 8192 entries wanted (M = 31, cap 56)
    assert [_plan(56, 31, D).table for D in (1664, 1672, 5760, 5768, 13968, 13976)] == [8192, 4096, 4096, 2048, 2048, 0]
    assert [_plan(113, 31, D).table for D in (1544, 1552, 1664, 5640, 5648)] == [8192, 4096, 4096, 4096, 0]
    assert [_plan(56, 8, D).table for D in (13968, 13976)] == [2048, 0]                              # the 64 KiB clause alone
    assert [_plan(10, 8, D).table for D in (14056, 14064)] == [2048, 0]
    old_table = lambda D: hpr.make_plan_old(False, 6000, D, 31, 62, 10, 56).table_size             # noqa: E731
    assert [old_table(D) for D in (3824, 3832, 7920, 7928, 9968, 9976)] == [8192, 4096, 4096, 2048, 2048, 0]
    # EMAX and the kernels
    assert [_plan(c, 16).emax for c in (128, 129, 256, 257, 1024)] == [2, 4, 4, 16, 16]
    assert [_plan(c, 16).family for c in (1024, 1025)] == ["lds", "big"]
    assert (_plan(256, 16).kernel, _plan(257, 16).kernel) == ("one", "one")                          # (both bitset plans)
    assert [_plan(c, 16, mw="2").kernel for c in (56, 227)] == ["mw", "mw"]
    assert [_plan(56, mw=m).kernel for m in (None, "0", "1", "2")] == ["mw", "one", "mw", "mw"]
    assert [hpr.route("l2", 2000, 128, 8, 16, nq, 10, 56, mw=m, mw_maxq="64").kernel
            for nq, m in ((64, None), (65, None), (65, "2"))] == ["mw", "one", "mw"]
    assert _plan(56, space=hpr.SIFT).kernel == "one"
    # list lengths: narrow -> wide (which ends the multi-wave kernel) at a longest list of 62 / 63, on level 0 and above it,
    # in every family; and the frontier arrays
    assert [(r.wide, r.kernel) for r in (_plan(40, 31), _plan(40, 32))] == [(False, "mw"), (True, "one")]
    lists = lambda maxM, maxM0, **kw: hpr.route("l2", 2000, 128, maxM, maxM0, 64, 10, 40, **kw)       # noqa: E731
    assert [(lists(31, L).wide, lists(31, L).kernel) for L in (62, 63)] == [(False, "mw"), (True, "one")]
    assert [(lists(L, 20).wide, lists(L, 20).kernel) for L in (62, 63)] == [(False, "mw"), (True, "one")]
    assert [lists(31, L, algo="old").wide for L in (62, 63)] == [False, True]
    assert [lists(L, 20, algo="old").wide for L in (62, 63)] == [False, True]
    assert [hpr.route("l2", 2000, 128, 31, L, 64, 10, 1025).wide for L in (62, 63)] == [False, True]      # the HBM-array kernel
    assert [hpr.wide(31, L) for L in (0, 62, 63, 64)] == [False, False, True, True]
    assert [hec.route_of(c, "2").wide for c in hec.LIST_CASES[:4]] == [False, True, False, True]
    assert [hpr.nbcap(40, L) for L in (62, 63, 127, 128, 191, 192, 254, 255, 256)] == [64, 64, 128, 192, 192, 256, 256, 256, 320]
    assert [hpr.route("l2", 600, 6, 40, L, 64, 10, 40, "v1merge").family for L in (254, 255, 256)] == ["lds", "lds", "big"]
    assert hpr.route("l2", 600, 6, 256, 100, 64, 10, 40, "v1merge").family == "big"                  # (maxM counts too)
    # SearchOld: queue placement, the heap, hybrid
    old = lambda n, k, ef: hpr.make_plan_old(False, n, 16, 8, 16, k, ef)       # noqa: E731
    assert (old(9000, 10, 8192).a_in_lds, old(9000, 10, 8193).a_in_lds) == (1, 0)
    assert (old(9000, 10, 8192).ws_a, old(9000, 10, 8193).ws_a) == (0, 8193 * 4)
    assert (old(9000, 2048, 100).r_in_lds, old(9000, 2049, 100).r_in_lds) == (1, 0)
    assert (old(2046, 10, 100).heap_lds, old(2046, 10, 100).ws_heap) == (2047, 0)
    assert (old(2047, 10, 100).heap_lds, old(2047, 10, 100).ws_heap) == (2048, 0)
    assert (old(2048, 10, 100).heap_lds, old(2048, 10, 100).ws_heap) == (2048, 8)
    assert [hpr.route("l2", 2000, 128, 16, 32, 64, 10, ef, "hybrid").family for ef in (999, 1000)] == ["lds", "old"]
    # fp16 walk: the LDS families only
    assert [hpr.route("l2", 2000, 128, 8, 16, 64, 10, ef, "hybrid", "f16").family for ef in (56, 1000, 1025)] == ["f16", "old", "old"]
    assert hpr.route("l2", 2000, 128, 8, 16, 64, 1025, 10, "hybrid", "f16").family == "big"
    # the overflow launch
    assert [hpr.route("l2", 2000, 128, 8, 16, nq, 10, 56).fix_slots for nq in (1, 128, 129)] == [1, 128, 128]
    assert hpr.route("l2", 2000, 128, 8, 16, 300, 10, 57).fix_slots == 0
    assert (hpr.overflow_threshold(2048), hpr.overflow_threshold(4096)) == (1792, 3584)


def test_what_no_input_reaches(printed_plans):
    """No table plan exists beyond cap 227 (18 * cap <= table / 2 needs 16384 entries from cap 228 on; they do not fit the
    40 KiB budget), so the hnsw_search_kernel<.., BITSET = false, EMAX = 16, ..> instantiations are never launched: over the
    grid, and for every cap with the shortest rows and lists.  The `> 64 KiB` clause IS reached, in both planners."""
    lds, old = printed_plans
    for (u8, n, ldv, maxM, maxM0, k, ef, force), v in lds.items():
        assert not (v[1] and v[0] > 256), (u8, n, ldv, maxM, maxM0, k, ef)
    for cap in range(228, 1025):
        for maxM0 in (1, 4, 62, 255):
            assert hpr.make_plan(True, 10 ** 6, 128, 1, maxM0, 1, cap).table_size == 0
            assert hpr.make_plan(False, 10 ** 6, 8, 1, maxM0, 1, cap).table_size == 0
    for (u8, n, ldv, maxM, maxM0, k, ef, force, asked), v in old.items():      # SearchOld: 64 KiB hold no 16384 entries either
        assert v[1] <= 8192
    # the clause: cap 10 passes the other two at 14 064 floats a row; SearchOld, with a 16 KiB heap in LDS, at 9976
    p = hpr.make_plan(False, 300, 14064, 8, 16, 10, 10)
    assert p.table_size == 0 and 18 * 10 <= 1024 and 2048 * 4 + hpr.lds_fixed(False, 14064, 8, 16, 10) > 64 * 1024
    assert hpr.make_plan(False, 300, 14056, 8, 16, 10, 10).table_size == 2048
    assert [hpr.make_plan_old(False, 6000, D, 31, 62, 10, 56).table_size for D in (9968, 9976)] == [2048, 0] and 18 * 56 <= 1024


# ---- the cases ---------------------------------------------------------------------------------------------------------
def test_every_case_names_the_route_it_takes():
    names = [c.name for c in hec.ALL_CASES]
    assert len(set(names)) == len(names)
    for c in hec.ALL_CASES:
        assert 8 <= c.nq <= 300
        for mw in c.mw:
            r = hec.route_of(c, mw)
            for field, want in c.expect.items():
                if field == "kernel" and mw == "0" and want == "mw":
                    want = "one"
                assert getattr(r, field) == want, (c.name, mw, field, getattr(r, field), want)
            assert r.path == (5 if c.rows == "f16" and r.family == "f16" else 4), c.name
        if len(c.mw) > 1:       # both kernels serve the first launch of a table plan
            assert {hec.route_of(c, m).kernel for m in c.mw} == {"one", "mw"} or c.graph.space == hpr.SIFT or \
                hec.route_of(c, "2").wide, c.name
            assert hec.route_of(c, "2").table > 0, c.name
    # every table plan of the cap sweeps runs under both settings, every flip has a case on either side
    for c in hec.CAP_CASES:
        assert (len(c.mw) == 2) == (hec.route_of(c).table > 0), c.name
    caps = lambda tag: sorted({max(c.k, c.ef) for c in hec.CAP_CASES if c.name.startswith(tag)})     # noqa: E731
    assert caps("m8_") == [56, 57, 64, 65, 113, 114, 128, 129, 227, 228]
    assert caps("m16_") == [32, 33, 64, 65, 227, 228, 256, 257, 1024, 1025]
    assert caps("sift_") == caps("f16_") == [56, 57, 227, 228]
    # the routes of the refused case and of the overflow batches
    assert hec.route_of(hec.LONG_REFUSED).lds_bytes > hpr.LDS_LIMIT
    g = hec.G_OVER
    r = hpr.route(g.space, g.n, g.D, g.maxM, g.maxM0, 300, 10, hec.OVER_EF, mw="2")
    assert (r.table, r.kernel, r.fix_slots, r.wide) == (hec.OVER_TABLE, "mw", 128, False)
    assert hpr.make_plan(False, g.n, g.D, g.maxM, g.maxM0, 10, hec.OVER_EF).table_size * 4 == 2048 * 4
    assert 1 << hpr.ilog2(g.maxM0 * hec.OVER_EF * 2) == 8192                   # wanted; the rows leave a quarter
    assert hpr.make_plan_old(False, g.n, g.D, g.maxM, g.maxM0, 10, hec.OVER_EF).table_size == hec.OVER_TABLE


@pytest.mark.parametrize("L", hec.LIST_LENGTHS)
def test_list_cases_hold_a_list_of_exactly_that_length(L):
    g = hec.G_LIST[L]
    l0 = hec.oracle_graph(g).links0()
    assert l0[:, 0].max() == L == g.maxM0, f"longest list {l0[:, 0].max()}"
    # the walks meet no equal keys (hec.G_LIST), and the sums stay exact
    Q = hec.short_queries(g, 64)
    assert len(Q) == 64 and hec.distinct_distances(g, Q).all()
    assert g.d0 * (2 * g.span) ** 2 < 2 ** 24


def test_wide_tie_cases_meet_equal_keys():
    """the conditions of hec.WIDE_TIES_CASES from the oracle alone: a list of 128 entries, queries with rows at equal
    distances among their ten nearest; and the checker's own distances are the oracle's bits"""
    g = hec.G_LIST_TIES
    assert hec.oracle_graph(g).links0()[:, 0].max() == 128 == g.maxM0 and hpr.wide(g.maxM, g.maxM0)
    Q = hec.short_queries(g, 64)
    assert not hec.distinct_distances(g, Q).any()
    for case in hec.WIDE_TIES_CASES:
        want = hec.reference(case)
        hec.check_under_ties(g, Q, want, want)
        assert sum(len(np.unique(d)) < len(d) for d in want[1]) > 16, case.name
    want = hec.reference(hec.WIDE_TIES_CASES[0])
    q = int(np.nonzero([len(np.unique(d)) == len(d) for d in want[1]])[0][0])       # a query whose ten distances differ
    for what in ("ids_swapped", "distance_one_ulp", "count_off", "first_launch_output"):
        assert _rejects(hec.check_under_ties, g, Q, hec.corrupt(want, what, q), want), what


@pytest.mark.parametrize("g", [hec.G8, hec.G_LIST[255], hec.G_LONG[13968], hec.G_FEW[2]], ids=lambda g: g.name)
def test_host_builder_gives_the_oracles_graph(g, tmp_path):
    """what the GPU cases rely on (and assert again there): one thread builds the graph the oracle builds, also with
    delaunay_type 0, explicit list bounds and zero-padded long rows"""
    idx = nz.Index(g.space, "hnsw")
    idx.addDenseBatch(hec.rows(g))
    idx.buildIndex(gpu_defer=1, **hec.index_params(g))
    path = str(tmp_path / "g.idx")
    idx.save(path, save_data=False)
    idx.close()
    got, want = refio.parse_optimized_index(path), hec.arrays_of(hec.oracle_graph(g))
    for key in ("maxM", "maxM0", "maxlevel", "enterpoint"):
        assert int(got[key]) == int(want[key]), key
    for key in ("levels", "links0", "up_off", "up_links"):
        np.testing.assert_array_equal(got[key], want[key])


def test_widened_index_file_holds_the_same_graph_over_padded_rows(tmp_path):
    """how the overflow case gets 6000 long rows with a sequential graph: the index of the first columns, its file padded"""
    g = hec.G_LONG[13968]._replace(D=1000)
    idx = nz.Index(g.space, "hnsw")
    idx.addDenseBatch(hec.short_rows(g))
    idx.buildIndex(gpu_defer=1, **hec.index_params(g))
    a, b, c = (str(tmp_path / f) for f in ("short.idx", "long.idx", "again.idx"))
    idx.save(a, save_data=False)
    idx.close()
    hec.widen_optimized_index(a, b, g.D)
    wide = nz.Index.load(b, load_data=False)
    wide.save(c, save_data=False)
    wide.close()
    short, again = refio.parse_optimized_index(a), refio.parse_optimized_index(c)
    assert again["payload"].shape[1] == g.D * 4
    np.testing.assert_array_equal(again["payload"].copy().view(np.float32), hec.rows(g))
    for key in ("ids", "links0", "levels", "up_off", "up_links"):
        np.testing.assert_array_equal(again[key], short[key])
    assert (again["maxlevel"], again["enterpoint"]) == (short["maxlevel"], short["enterpoint"])


def test_few_row_cases_pad():
    for c in hec.FEW_CASES:
        ids, ds, cnt, _, _ = hec.reference(c)
        assert (cnt == c.graph.n).all() and c.k > c.graph.n and (ids[:, c.graph.n:] == -1).all()
    for c in hec.OLD_CASES[:4]:
        ids, ds, cnt, _, _ = hec.reference(c)
        assert (cnt == c.k).all() and c.graph.n > max(c.k, c.ef), c.name       # the counts stay meaningful


def test_integer_cases_are_exact_in_f32():
    for g in (hec.G8, hec.G16, hec.G_OVER, hec.G_LONG[40704]):
        x = hec.short_rows(g)
        assert (x == np.round(x)).all() and np.abs(x).max() <= 8 and g.d0 * 16 * 16 < 2 ** 24
    x = hec.short_rows(hec.G8_SIFT)
    assert x.dtype == np.uint8 and x.max() <= 16


# ---- the overflow case -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def over_sequential():
    """the overflow graph as the oracle builds it (the GPU case loads the host builder's, the same): the graph, its arrays,
    the pool's answers"""
    og = hec.oracle_graph(hec.G_OVER)
    Q = hec.short_queries(hec.G_OVER, hec.OVER_POOL)
    return og, hec.arrays_of(og), Q, og.search(Q, 10, hec.OVER_EF)


def test_upper_evaluations_restate_the_descent(over_sequential):
    """with every level-0 list emptied a search evaluates the entry point and the descent only: ndc = 1 + upper"""
    og, arrays, Q, _ = over_sequential
    assert arrays["maxlevel"] >= 1
    bare = dict(arrays, links0=np.zeros_like(arrays["links0"]))
    og0 = hec.oracle_from_saved(hec.G_OVER, bare)
    ndc = og0.search(Q[:200], 1, 1)[3]
    upper = hec.upper_evaluations(arrays, hec.short_rows(hec.G_OVER), Q[:200])
    np.testing.assert_array_equal(ndc, 1 + upper)
    assert upper.min() > 0 and len(np.unique(upper)) > 3


def test_overflow_batches_overflow(over_sequential):
    """the conditions of the two batches, from the oracle alone: more queries overflow than the second launch has
    workgroups, so slots are reused; and a batch that mixes both kinds.  (Exact relation, hec.marked_rows: no slack.)"""
    og, arrays, Q, (_, _, cnt, ndc, hops) = over_sequential
    upper = hec.upper_evaluations(arrays, hec.short_rows(hec.G_OVER), Q)
    over = hec.overflows(ndc, upper, hec.OVER_TABLE)
    marked = hec.marked_rows(ndc, upper)
    print(f"marked rows min / median / max {marked.min()} / {np.median(marked)} / {marked.max()}, over 1792: {over.sum()} of {len(over)}")
    a, b = hec.pick_batches(over)
    assert len(a) == 300 and len(b) == 100 and len(set(a.tolist())) == 300 and len(set(b.tolist())) == 100
    assert over[a].sum() > hpr.FIX_SLOTS and (~over[a]).sum() > 0
    assert 0 < over[b].sum() < len(b)
    assert (marked <= hec.G_OVER.n).all() and (cnt == 10).all()
    # SearchOld on the same table size: the batch holds queries past the threshold, so the host retries with bitsets
    ondc = og.search(Q[a], 10, hec.OVER_EF, algo="old")[3]
    assert hec.overflows(ondc, upper[a], hec.OVER_TABLE).any()


# ---- the checkers reject corrupted answers -------------------------------------------------------------------------------
def _rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("case", [hec.CAP_CASES[0], hec.FEW_CASES[6], hec.LIST_CASES[3]], ids=lambda c: c.name)
def test_exact_checker_rejects_corrupted_answers(case):
    want = hec.reference(case)
    hec.check_exact(want, want)
    q = case.nq - 1
    for what in ("ids_swapped", "distance_one_ulp", "count_off", "ndc_off", "hops_off", "first_launch_output"):
        assert want[2][q] >= 2
        assert _rejects(hec.check_exact, hec.corrupt(want, what, q), want), what
    assert not _rejects(hec.check_exact, hec.corrupt(want, "ndc_off", q), want, False)      # (counters switched off)


def test_redone_checker_rejects_a_count_off_by_one():
    hec.check_redone(130, 130)
    assert _rejects(hec.check_redone, 129, 130) and _rejects(hec.check_redone, 131, 130) and _rejects(hec.check_redone, 0, 130)


def test_float_checker_rejects_corrupted_answers():
    case = hec.FLOAT_CASES[0]
    want = hec.reference(case)
    hec.check_float(case.graph.space, want, want)
    q = 3
    i = int(np.nonzero(np.diff(want[1][q]) > 0)[0][0])
    swapped = tuple(np.array(a, copy=True) for a in want)
    swapped[0][q, [i, i + 1]] = swapped[0][q, [i + 1, i]]
    assert _rejects(hec.check_float, case.graph.space, swapped, want)
    assert _rejects(hec.check_float, case.graph.space, hec.corrupt(want, "count_off", q), want)
    off = tuple(np.array(a, copy=True) for a in want)
    off[1][q, 5] *= np.float32(1 + 3e-5)
    assert _rejects(hec.check_float, case.graph.space, off, want)
    assert _rejects(hec.check_float, case.graph.space, hec.corrupt(want, "first_launch_output", q), want)
