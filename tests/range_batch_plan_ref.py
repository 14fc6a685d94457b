"""Restatement of nmslib_zig_amd/csrc/range_batch_plan.hpp: the plan of a batched range query on the exact scan.
tests/test_range_batch_cpu.py holds it to the header's output line by line; the GPU tests take the tile, the bound of
the batched dimension and the slice sizes from here."""
from collections import namedtuple

ROWS_PER_WG = 256
QUERY_TILE = 32
MAX_DIM = 256
SELECT_ROWS = 1024
TARGET_WGS = 1024
MAX_SLICE_QUERIES = 32768
WS_BYTES = 256 << 20

Plan = namedtuple("Plan", "route rows_per_wg chunks query_tile grid_x grid_y mask_words blocks slice_queries slices "
                          "workspace_bytes count_only")


def ceil_div(a, b):
    return -(-a // b)


def query_bytes(n):
    """bytes of the workspace one query takes: a bit per row in 64-bit words, a count per 1024 rows and the total"""
    return ceil_div(n, 64) * 8 + (ceil_div(n, SELECT_ROWS) + 1) * 4


def plan(n, dim, elem, nq, capacity, budget=WS_BYTES):
    count_only = int(capacity == 0)
    dim_ok = dim == 128 if elem == 1 else 1 <= dim <= MAX_DIM
    per_query = query_bytes(n)
    if not dim_ok or per_query > budget or nq == 0:
        return Plan(11, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, count_only)
    slice_queries = min(nq, budget // per_query, MAX_SLICE_QUERIES)
    grid_x = ceil_div(n, ROWS_PER_WG)
    tiles = ceil_div(slice_queries, QUERY_TILE)
    want = ceil_div(TARGET_WGS, grid_x) if grid_x else 1
    return Plan(10, ROWS_PER_WG, 1 if elem == 1 else ceil_div(dim, 64), QUERY_TILE, grid_x, max(1, min(tiles, want)),
                ceil_div(n, 64), ceil_div(n, SELECT_ROWS), slice_queries, ceil_div(nq, slice_queries),
                slice_queries * per_query, count_only)


def slice_sizes(p, nq):
    return [min(p.slice_queries, nq - s * p.slice_queries) for s in range(p.slices)]


def budget_for(n, slice_queries):
    """the smallest NMSLIB_GPU_RANGE_WS_BYTES under which a slice holds exactly `slice_queries` queries"""
    return slice_queries * query_bytes(n)


# the grid the header's check program prints (tests/range_batch_plan_check.cpp walks the same lists in the same order)
GRID_N = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 262144, 263173, 1000000)
GRID_DIM = ((4, 1), (4, 5), (4, 64), (4, 65), (4, 128), (4, 129), (4, 256), (4, 257), (4, 768), (1, 128), (1, 64))
GRID_Q = (0, 1, 31, 32, 33, 64, 65, 1024, 32768, 32769)
GRID_CAP = (0, 128)
# budgets: the default; then, as multiples of the bytes one query takes (the check program resolves them per n):
# below one query, exactly one, two, two and a half
GRID_BUDGET_X2 = (1, 2, 4, 5)    # halves of a query's bytes


def grid():
    for n in GRID_N:
        budgets = [WS_BYTES] + [query_bytes(n) * h // 2 for h in GRID_BUDGET_X2]
        for elem, dim in GRID_DIM:
            for nq in GRID_Q:
                for cap in GRID_CAP:
                    for budget in budgets:
                        yield n, dim, elem, nq, cap, budget


def line(point):
    p = plan(*point)
    return " ".join(str(int(v)) for v in tuple(point) + tuple(p))
