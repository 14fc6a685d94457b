"""Python restatement of the launch layer of the dense HNSW search.

hnsw_nbcap and the hnsw_old_ws_* sizes (nmslib_zig_amd/csrc/kernels/kernels.hpp), hnsw_make_plan and hnsw_make_plan_old
(hnsw_plan.cpp), the choice of the kernel family (Engine::hnsw_walk, hnsw_search_lds and knn_hnsw_old, hnsw_search.cpp) and
the template choices of the launch functions at the end of kernels/hnsw_kernels.hip, the LDS size of the HBM-array kernel
among them.

THIS FILE CHANGES TOGETHER WITH THOSE: tests/test_hnsw_plan_cpu.py holds it to the C++ on a grid, and the cases of
tests/hnsw_edge_cases.py name the route values they are there for, so a change that moves a switch fails there.

What is held to the C++ and what is not.  tests/hnsw_plan_check.cpp compiles kernels.hpp and hnsw_plan.cpp, so nbcap, wide
(hnsw_wide), emax_of (hnsw_emax), both planners, the workspace sizes, big_lds and the two limits are compared with the code the
launch functions call.  The rest restates code that the check program cannot compile (the .hip file and the engine), and the
host tests compare it only with itself: search_old (Engine::search_old), the order of the families in route (Engine::hnsw_walk),
the multi-wave choice and its two environment variables (launch_space_w), FIX_SLOTS (Engine::hnsw_search_lds),
overflow_threshold (the kernels) and the carved_* sums (read from the kernels by hand).  On the GPU the cases observe last_path,
hnsw_redone and the answers, not which kernel or EMAX instantiation ran: a wrong choice there shows only where it changes an
answer, a counter or an overflow count."""
from collections import namedtuple

SIFT = "l2sqr_sift"
LDS_BUDGET = 40 * 1024 - 64        # hnsw_make_plan: four workgroups a CU
OLD_BUDGET = 64 * 1024             # hnsw_make_plan_old
NBCAP_LDS = 256                    # HNSW_NBCAP_LDS
LDS_LIMIT = 160 * 1024             # HNSW_LDS_LIMIT: what a workgroup may take on gfx950
FIX_SLOTS = 128                    # hnsw_search_lds: workgroups that walk the overflow list

Plan = namedtuple("Plan", "cap table_size table_shift bitset_words lds_bytes")
OldPlan = namedtuple("OldPlan", "cap table_size table_shift bitset_words lds_bytes heap_lds heap_cap a_in_lds r_in_lds "
                                "ws_a ws_r ws_heap")
Route = namedtuple("Route", "family kernel emax wide table bitset fix_slots lds_bytes path")


def ilog2(v):
    l = 0
    while (1 << l) < v:
        l += 1
    return l


def f32_row_stride(dim):
    return (dim + 7) & ~7


def ldv_of(space, D):
    return 128 if space == SIFT else f32_row_stride(D)


def nbcap(maxM, maxM0):
    longest = max(maxM0, maxM)
    return 64 if longest <= 62 else (longest + 64) // 64 * 64


def wide(maxM, maxM0):
    return maxM0 > 62 or maxM > 62


def row_bytes(u8, ldv):
    return 128 if u8 else ldv * 4


def plan_visited(cap, n, maxM0, fixed, budget, force_bitset):
    """-> table_size, table_shift, bitset_words, lds_bytes"""
    want = 1 << ilog2((maxM0 if maxM0 > 0 else 32) * cap * 2)
    want = max(want, 2048)
    while want * 4 + fixed > budget and want > 2048:
        want >>= 1
    if force_bitset or 18 * cap > want // 2 or want * 4 + fixed > 64 * 1024:
        return 0, 0, (n + 31) // 32, fixed + 16
    return want, 32 - ilog2(want), 0, fixed + want * 4


def lds_fixed(u8, ldv, maxM, maxM0, cap):
    return ((cap + 3) & ~3) * 8 + row_bytes(u8, ldv) + (2 * nbcap(maxM, maxM0) + 2 * 64) * 4


def make_plan(u8, n, ldv, maxM, maxM0, k, ef, force_bitset=False):
    """hnsw_make_plan"""
    cap = max(ef, k)
    return Plan(cap, *plan_visited(cap, n, maxM0, lds_fixed(u8, ldv, maxM, maxM0, cap), LDS_BUDGET, force_bitset))


def make_plan_old(u8, n, ldv, maxM, maxM0, k, ef, force_bitset=False, heap_cap=0):
    """hnsw_make_plan_old and the per-query workspaces hnsw_old_ws_a / _r / _heap"""
    cap = max(ef, k)
    a_in_lds, r_in_lds = int(ef <= 8192), int(k <= 2048)
    hc = heap_cap if heap_cap > 0 else 32 * cap + 4096
    hc = min(hc, n + 1)
    heap_lds = min(hc, 2048)
    fixed = (row_bytes(u8, ldv) + (2 * nbcap(maxM, maxM0) + 64) * 4 + heap_lds * 8 +
             (((ef + 1) & ~1) * 4 if a_in_lds else 0) + (k * 8 if r_in_lds else 0))
    v = plan_visited(cap, n, maxM0, fixed, OLD_BUDGET, force_bitset)
    return OldPlan(cap, *v, heap_lds, hc, a_in_lds, r_in_lds,
                   0 if a_in_lds else ef * 4, 0 if r_in_lds else k * 8, (hc - heap_lds) * 8)


def big_lds(u8, ldv, maxM, maxM0):
    """hnsw_big_lds: the dynamic LDS of hnsw_search_big_kernel"""
    return row_bytes(u8, ldv) + (2 * nbcap(maxM, maxM0) + 2 * 64) * 4 + 16


# ---- what the kernels carve out of their dynamic LDS, read from the kernels ------------------------------------------
def carved_lds(u8, ldv, maxM, maxM0, cap, table_size):
    """hnsw_search_body: keys, idu [capa]; the query; nbr, nd [nbcap]; sk, si [64]; the table"""
    nb = nbcap(maxM, maxM0) if wide(maxM, maxM0) else 64
    return 2 * ((cap + 3) & ~3) * 4 + row_bytes(u8, ldv) + 2 * nb * 4 + 2 * 64 * 4 + table_size * 4


def carved_mw(ldv, cap, table_size):
    """hnsw_search_mw_kernel: keys, idu [capa]; the query; nbr, nd [64]; ctl [4]; the table"""
    return 2 * ((cap + 3) & ~3) * 4 + ldv * 4 + 2 * 64 * 4 + 16 + table_size * 4


def carved_old(u8, ldv, maxM, maxM0, p, k, ef):
    """hnsw_search_old_kernel: the query; nbr, nd [nbcap]; sk [64]; the heap; A; R; the table"""
    nb = nbcap(maxM, maxM0) if wide(maxM, maxM0) else 64
    return (row_bytes(u8, ldv) + 2 * nb * 4 + 64 * 4 + p.heap_lds * 8 + (((ef + 1) & ~1) * 4 if p.a_in_lds else 0) +
            (k * 8 if p.r_in_lds else 0) + p.table_size * 4)


def carved_big(u8, ldv, maxM, maxM0):
    """hnsw_search_big_kernel: the query; nbr, nd [nbcap]; sk, si [64]"""
    nb = nbcap(maxM, maxM0) if wide(maxM, maxM0) else 64
    return row_bytes(u8, ldv) + 2 * nb * 4 + 2 * 64 * 4


# ---- the route of a batch ------------------------------------------------------------------------------------------------
def search_old(algo, ef):
    """Engine::search_old"""
    return algo == "old" or (algo == "hybrid" and ef >= 1000)


def emax_of(cap):
    """launch_space_r: 64-entry registers a lane of the sorted array"""
    return 2 if cap <= 128 else 4 if cap <= 256 else 16


def route(space, n, D, maxM, maxM0, nq, k, ef, algo="hybrid", gpu_rows="f32", mw=None, mw_maxq=None):
    """The kernels a batch without deleted rows or a filter takes.  mw / mw_maxq: NMSLIB_HNSW_MW / NMSLIB_HNSW_MW_MAXQ as the
    process has them (None: unset).  family: old | big | f16 | lds; kernel: old | big | mw | one (the first launch of the two
    LDS families); table: entries of the LDS visited table, 0 with bitset; fix_slots: workgroups of the overflow launch (0
    without one); path: nmslib_gpu_stats_t.last_path."""
    u8 = space == SIFT
    ldv = ldv_of(space, D)
    cap = max(ef, k)
    w = wide(maxM, maxM0)
    if search_old(algo, ef):
        p = make_plan_old(u8, n, ldv, maxM, maxM0, k, ef)
        return Route("old", "old", 0, w, p.table_size, p.table_size == 0, 0, p.lds_bytes, 4)
    if cap > 1024 or nbcap(maxM, maxM0) > NBCAP_LDS:
        return Route("big", "big", 0, w, 0, True, 0, big_lds(u8, ldv, maxM, maxM0), 4)
    f16 = gpu_rows == "f16" and not u8
    # (the fp16 walk is the search asked for cap results: the same cap, so the same plan)
    p = make_plan(u8, n, ldv, maxM, maxM0, cap if f16 else k, ef)
    emax = emax_of(cap)
    kernel = "one"
    if p.table_size and not w and emax <= 4 and not u8:
        mode = 1 if mw is None else int(mw)
        max_nq = 0x7fffffff if mw_maxq is None else int(mw_maxq)
        if mode and (mode == 2 or nq <= max_nq):
            kernel = "mw"
    lds = p.lds_bytes + (16 if kernel == "mw" else 0)
    return Route("f16" if f16 else "lds", kernel, emax, w, p.table_size, p.table_size == 0,
                 min(nq, FIX_SLOTS) if p.table_size else 0, lds, 5 if f16 else 4)


def overflow_threshold(table_size):
    """a query is re-run once it has marked more rows than this (hnsw_search_body, hnsw_search_mw_kernel)"""
    return table_size - (table_size >> 3)
