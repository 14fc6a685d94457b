"""Python restatement of the plan the exact scans over sparse, string and divergence rows share.

scan_make_plan (nmslib_zig_amd/csrc/kernels/kernels.hpp) cuts the rows into splits and sizes the per-split lists, the LDS
key buffer and the query tile; Engine::scan_slices (engine.cpp) cuts a batch into slices of queries; launch_merge_topk_ex
(kernels/bf_kernels.hip) merges the split lists by an LDS sort or, past 64 KiB of keys, by the bisection kernel.

THIS FILE CHANGES TOGETHER WITH scan_make_plan: tests/test_scan_plan_cpu.py holds it to the C++ on a grid, and the cases of
tests/scan_edge_cases.py name the plan values they are there for, so a planner change that moves a switch fails there."""
from collections import namedtuple

SCAN_MAX_KL = 4096          # kScanMaxKl
SLICE_QUERIES = 32768       # scan_slices: queries per slice at most
SLICE_KEYS = 1 << 25        # ... and split keys per slice at most
MERGE_LDS_BYTES = 64 * 1024

Plan = namedtuple("Plan", "nsplit rows_per_split last_rows kl P tq")


def pow2_at_least(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def plan(n, nq, k, tq):
    """scan_make_plan(n, nq, k, tq); last_rows = the rows of the last split."""
    tiles = (nq + tq - 1) // tq
    want = (2048 + tiles - 1) // (tiles if tiles > 0 else 1)
    rps = (n + want - 1) // (want if want > 0 else 1)
    rps = max(rps, 1024)
    if k <= 4096:
        per = 8192 // k
        rps = max(rps, (n + per - 1) // per)
    if k > SCAN_MAX_KL:
        rps = SCAN_MAX_KL
    nsplit = (n + rps - 1) // rps if n > 0 else 1
    kl = min(k, rps)
    P = pow2_at_least(kl + 256)
    return Plan(nsplit, rps, n - (nsplit - 1) * rps, kl, P, tq if P <= 1024 else 1)


def merge_route(nsplit, k):
    """launch_merge_topk_ex: 'lds' (one bitonic sort of every list's keys) or 'bisect'"""
    return "bisect" if pow2_at_least(max(nsplit * k, 2)) * 8 > MERGE_LDS_BYTES else "lds"


def slices(n, nq, k, tq):
    """Engine::scan_slices -> [(first query, queries, Plan)]"""
    out, q0 = [], 0
    while q0 < nq:
        m = min(SLICE_QUERIES, nq - q0)
        p = plan(n, m, k, tq)
        while m > 1 and p.nsplit * m * k > SLICE_KEYS:
            m = max(1, m // 2)
            p = plan(n, m, k, tq)
        out.append((q0, m, p))
        q0 += m
    return out
