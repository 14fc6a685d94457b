"""The cases of tests/test_gpu_hnsw_plan_edges.py: the graphs, one table of cases with the route values each case is there
for, the inputs, the oracle's answers and the checkers.  tests/test_hnsw_plan_cpu.py holds every case's route to the
restatement (tests/hnsw_plan_ref.py), asserts the conditions on the inputs from the oracle alone, and feeds the checkers
corrupted answers.

Rows and queries are integers in [-8, 8] (bytes in [0, 16] for l2sqr_sift): every partial sum of every distance is exact in
f32 in any order, so the kernels and the oracle (oracle/knn_oracle.c, on the same graph) compute the same bits, and ids,
distance bits, counts, ndc and hops are compared with assert_array_equal.

Long rows.  The planner's switches on the row length need rows of 1552 .. 40 704 floats; what such a case is about is the LDS
carve-up, not the arithmetic.  Its rows are zero behind the first d0 columns, so the oracle builds and searches the graph of
the first d0 columns: the distances are the same numbers, at a hundredth of the cost."""
import functools
from collections import namedtuple

import numpy as np

from tests import hnsw_plan_ref as hpr
from tests import orc

# threads = 1: the host builder in the reference's order, the same graph as orc.HnswGraph.build gives
# span: the rows are integers in [-span, span]
Graph = namedtuple("Graph", "name space n D d0 M maxM maxM0 efc delaunay threads span")
# expect: fields of hnsw_plan_ref.Route that the case is there for.  mw: the NMSLIB_HNSW_MW settings the case runs under
# (None: as the process has it)
Case = namedtuple("Case", "name graph nq k ef algo rows mw expect")


def _graph(name, space, n, D, M, efc=40, d0=None, maxM=None, maxM0=None, delaunay=2, threads=1, span=8):
    return Graph(name, space, n, D, D if d0 is None else d0, M, M if maxM is None else maxM,
                 2 * M if maxM0 is None else maxM0, efc, delaunay, threads, span)


def seed_of(name):
    import zlib
    return zlib.crc32(name.encode()) & 0x7fffffff


def _int_rows(space, n, d, seed, span=8):
    rng = np.random.default_rng(seed)
    if space == hpr.SIFT:
        return rng.integers(0, 17, size=(n, d)).astype(np.uint8)
    return rng.integers(-span, span + 1, size=(n, d)).astype(np.float32)


def _float_rows(n, d, seed):
    """low-rank float rows (the cosine and angular cases)"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 8)) @ rng.standard_normal((8, d)) + 0.1 * rng.standard_normal((n, d))).astype(np.float32)


FLOAT_DATA = ("cosinesimil", "angulardist")


def _padded(g, x):
    if g.d0 == g.D:
        return x
    out = np.zeros((x.shape[0], g.D), x.dtype)
    out[:, :g.d0] = x
    return out


@functools.lru_cache(maxsize=None)
def short_rows(g):
    """the first d0 columns of the rows (all of them unless the rows are long)"""
    if g.space in FLOAT_DATA:
        return _float_rows(g.n, g.d0, seed_of(g.name))
    return _int_rows(g.space, g.n, g.d0, seed_of(g.name), g.span)


def rows(g):
    return _padded(g, short_rows(g))


@functools.lru_cache(maxsize=None)
def short_queries(g, nq, tag=""):
    if g.space in FLOAT_DATA:
        return _float_rows(nq, g.d0, seed_of(g.name + "/q" + tag))
    if g.span > 8:
        # the tie-free graphs: of a pool, the first nq queries that have no two rows at the same distance
        pool = _int_rows(g.space, 8 * nq, g.d0, seed_of(g.name + "/q" + tag), g.span)
        return pool[np.nonzero(distinct_distances(g, pool))[0][:nq]]
    return _int_rows(g.space, nq, g.d0, seed_of(g.name + "/q" + tag))


def distinct_distances(g, Q):
    """per query: no two rows of the graph lie at the same (l2) distance"""
    X = short_rows(g).astype(np.int64)
    d = ((X[None, :, :] - Q.astype(np.int64)[:, None, :]) ** 2).sum(axis=2)
    return np.array([len(np.unique(r)) == len(r) for r in d])


def queries(g, nq, tag=""):
    return _padded(g, short_queries(g, nq, tag))


def index_params(g):
    p = dict(M=g.M, efConstruction=g.efc, delaunay_type=g.delaunay)
    p["indexThreadQty"] = g.threads
    if (g.maxM, g.maxM0) != (g.M, 2 * g.M):
        p.update(maxM=g.maxM, maxM0=g.maxM0)
    return p


@functools.lru_cache(maxsize=None)
def oracle_graph(g):
    """the oracle's build of a sequential graph (computed once, never modified)"""
    return orc.HnswGraph.build(g.space, short_rows(g), g.M, g.efc, maxM=g.maxM, maxM0=g.maxM0, delaunay_type=g.delaunay)


def oracle_from_saved(g, saved):
    """the oracle over the graph of a saved index (refio.parse_optimized_index) and the first d0 columns of the rows"""
    return orc.HnswGraph.from_arrays(g.space, short_rows(g), int(saved["maxM"]), int(saved["maxM0"]), int(saved["maxlevel"]),
                                     int(saved["enterpoint"]), saved["levels"], saved["links0"], saved["up_off"],
                                     saved["up_links"])


def widen_optimized_index(src, dst, D):
    """The optimized index file `src` (hnsw.cc:774-806: a 68-byte header, then per row the object -- id, data length, the
    floats -- followed by its level-0 list, then the upper lists) with every row padded with zeros to D floats -> `dst`."""
    import struct
    with open(src, "rb") as f:
        raw = f.read()
    hdr = list(struct.unpack_from("<IIQQQiIQQiQ", raw, 0))
    flag, n, mem, off_l0, off_data = hdr[:5]
    d0 = (off_l0 - off_data - 16) // 4
    assert flag == 1 and off_data < off_l0 and D >= d0
    extra = (D - d0) * 4
    blk = np.frombuffer(raw, np.uint8, n * mem, 68).reshape(n, mem)
    out = np.zeros((n, mem + extra), np.uint8)
    out[:, :off_l0] = blk[:, :off_l0]
    out[:, off_l0 + extra:] = blk[:, off_l0:]
    out[:, off_data + 8:off_data + 16] = np.frombuffer(struct.pack("<Q", D * 4), np.uint8)
    hdr[2], hdr[3] = mem + extra, off_l0 + extra
    with open(dst, "wb") as f:
        f.write(struct.pack("<IIQQQiIQQiQ", *hdr))
        f.write(out.tobytes())
        f.write(raw[68 + n * mem:])


def arrays_of(og):
    """an oracle graph in the keys of refio.parse_optimized_index that a graph needs"""
    up_off, up_links = og.flat_upper()
    return dict(maxM=og.maxM, maxM0=og.maxM0, maxlevel=og.maxlevel, enterpoint=og.enterpoint, levels=og.levels(),
                links0=og.links0(), up_off=up_off, up_links=up_links)


def oracle_answer(og, g, Qshort, k, ef, algo):
    """-> (ids, dists, counts, ndc, hops) as the index reports them (ids are positions: the cases add rows without ids)"""
    # (angulardist has no optimized-index distance: the reference searches it on the generic path, hnsw.cc:369-412)
    return og.search(Qshort, k, ef, optimized=g.space != "angulardist", algo="old" if hpr.search_old(algo, ef) else "v1merge")


_memo = {}


def reference(case):
    """the oracle's answer of a case on a sequential graph, computed once"""
    if case.name not in _memo:
        g = case.graph
        _memo[case.name] = oracle_answer(oracle_graph(g), g, short_queries(g, case.nq), case.k, case.ef, case.algo)
    return _memo[case.name]


def route_of(case, mw=None):
    g = case.graph
    return hpr.route(g.space, g.n, g.D, g.maxM, g.maxM0, case.nq, case.k, case.ef, case.algo, case.rows, mw)


# ---- the checkers ------------------------------------------------------------------------------------------------------
def check_exact(got, want, counters=True):
    """got, want: (ids, dists, counts, ndc, hops).  Ids, the bits of the distances, the counts and (-1, +inf) behind them,
    and the work counters."""
    ids, ds, cnt, ndc, hops = got
    wids, wds, wcnt, wndc, whops = want
    np.testing.assert_array_equal(cnt, wcnt)
    np.testing.assert_array_equal(ids, wids)
    np.testing.assert_array_equal(np.ascontiguousarray(ds, np.float32).view(np.uint32),
                                  np.ascontiguousarray(wds, np.float32).view(np.uint32))
    k = ids.shape[1]
    past = np.arange(k)[None, :] >= np.asarray(cnt)[:, None]
    assert (ids[past] == -1).all() and np.isposinf(ds[past]).all(), "a slot behind the count holds a result"
    assert (ids[~past] >= 0).all()
    if counters:
        np.testing.assert_array_equal(np.asarray(ndc, np.int64), np.asarray(wndc, np.int64))
        np.testing.assert_array_equal(np.asarray(hops, np.int64), np.asarray(whops, np.int64))


def check_float(space, got, want):
    """the cosine / angular cases: the helpers of tests/gpuutil.py at their settings"""
    from tests.gpuutil import close_rel, ids_match_modulo_ties, sim_close
    ids, ds, cnt, _, _ = got
    wids, wds, wcnt, _, _ = want
    np.testing.assert_array_equal(cnt, wcnt)
    real = wids >= 0
    assert np.isfinite(wds[real]).all()
    if space == "angulardist":
        # d = acos(s): the similarity within 4 ulp everywhere; 1e-5 relative on d where acos is well conditioned
        assert sim_close(np.cos(ds[real].astype(np.float64)), np.cos(wds[real].astype(np.float64)), ulps=4)
        mid = real & (wds > 0.3) & (wds < 2.8)
        assert close_rel(ds[mid], wds[mid])
    else:
        assert close_rel(ds[real], wds[real])
    assert ids_match_modulo_ties(ids, ds, wids, wds)
    assert (ids[~real] == -1).all() and np.isposinf(ds[~real]).all()


def check_under_ties(g, Qshort, got, want):
    """A wide-list v1merge walk over rows with equal keys (l2, integer rows): what holds whatever order equal keys enter the
    sorted array in.  The counts; every distance is the exact distance of its id, bit for bit; ascending; no id twice.
    NOT the oracle's ids, not even outside groups of equal distance (ids_match_modulo_ties fails on 3 of 64 queries of
    list128ties_v1merge): the array holds cap items, and which of two equal keys takes its last slot decides which row is
    expanded later, so two correct walks that differ only in the order of equal keys can end with different rows."""
    ids, ds, cnt, _, _ = got
    wcnt = want[2]
    np.testing.assert_array_equal(cnt, wcnt)
    X, Q = short_rows(g).astype(np.int64), np.asarray(Qshort).astype(np.int64)
    for q in range(len(Q)):
        c = int(cnt[q])
        assert len(set(ids[q, :c].tolist())) == c and (ids[q, :c] >= 0).all() and (ids[q, c:] == -1).all(), q
        # (l2 on the optimized index: the squared distance, hnsw_distfunc_opt.cc; an integer below 2^24)
        exact = ((X[ids[q, :c]] - Q[q]) ** 2).sum(axis=1).astype(np.float32)
        np.testing.assert_array_equal(np.ascontiguousarray(ds[q, :c], np.float32).view(np.uint32), exact.view(np.uint32))
        assert (np.diff(ds[q, :c]) >= 0).all() and np.isposinf(ds[q, c:]).all(), q


def check_redone(redone, predicted):
    assert int(redone) == int(predicted), f"hnsw_redone {redone}, the oracle predicts {predicted} overflowing queries"


# ---- the overflow of the LDS visited table ------------------------------------------------------------------------------
def upper_evaluations(saved, Xshort, Qshort):
    """Distance evaluations of the greedy descent above level 0, the entry point's own not counted: per query, the sum of
    the list lengths of the nodes the descent stands on, once per look (hnsw_distfunc_opt.cc:168-198: a look evaluates the
    whole list of the node it started on and moves to the first entry of the smallest distance, if that is smaller).
    Integer rows: exact in float64."""
    maxM, up_off, up = int(saved["maxM"]), saved["up_off"], saved["up_links"]
    X = np.asarray(Xshort, np.float64)
    out = np.zeros(len(Qshort), np.int64)
    for qi, q in enumerate(np.asarray(Qshort, np.float64)):
        cur = int(saved["enterpoint"])
        curd = ((X[cur] - q) ** 2).sum()
        for lvl in range(int(saved["maxlevel"]), 0, -1):
            changed = True
            while changed:
                changed = False
                blk = up[up_off[cur] + (lvl - 1) * (maxM + 1):up_off[cur] + lvl * (maxM + 1)]
                cnt = int(blk[0])
                out[qi] += cnt
                if cnt:
                    nb = blk[1:1 + cnt]
                    d = ((X[nb] - q) ** 2).sum(axis=1)
                    j = int(np.argmin(d))
                    if d[j] < curd:
                        curd, cur, changed = d[j], int(nb[j]), True
    return out


def marked_rows(ndc, upper):
    """What a walk has marked in its visited set when it ends: the entry point of level 0 and every row evaluated on level
    0.  The kernels count exactly that (nvisited = 1, then += the unvisited neighbours of every expansion, hnsw_search_body
    and hnsw_search_mw_kernel; the pipelined filter runs only for a node that IS the next expansion), and ndc = 1 for the
    entry point + the evaluations above level 0 + those on level 0: marked = ndc - upper, exactly."""
    return np.asarray(ndc, np.int64) - np.asarray(upper, np.int64)


def overflows(ndc, upper, table_size):
    """the queries the LDS-table launch gives up on: the count passes 7/8 of the table at some expansion iff it does at
    the end (it only grows)"""
    return marked_rows(ndc, upper) > hpr.overflow_threshold(table_size)


def pick_batches(over):
    """From a pool of queries, by the oracle's prediction: (a) 300 queries of which as many as the pool gives, up to 220,
    overflow -- more than the 128 workgroups of the second launch, so slots are reused -- and the others do not; (b) 100
    queries, 30 overflowing among 70 that do not.  Interleaved, so that the list is not in query order by construction."""
    yes, no = np.nonzero(over)[0], np.nonzero(~over)[0]

    def mix(ny, nn):
        a, b = yes[:ny], no[:nn]
        order = np.random.default_rng(7).permutation(len(a) + len(b))
        return np.concatenate([a, b])[order]
    na = min(220, len(yes))
    return mix(na, min(300 - na, len(no))), mix(min(30, len(yes)), min(70, len(no)))


# ---- the graphs ----------------------------------------------------------------------------------------------------------
G8 = _graph("g8", "l2", 2000, 128, 8)
G16 = _graph("g16", "l2", 2000, 128, 16)
G8_SIFT = _graph("g8sift", hpr.SIFT, 2000, 128, 8)
G8_SPACE = {s: _graph("g8" + s, s, 1000, 21, 8) for s in ("l1", "linf", "negdotprod")}
G_FLOAT = {s: _graph("gf" + s, s, 1500, 40, 8) for s in FLOAT_DATA}
G_M31 = _graph("m31", "l2", 1000, 16, 31)
G_M32 = _graph("m32", "l2", 1000, 16, 32)
# Lists filled to the bound: delaunay_type 0 keeps the closest maxM0 of a node's candidates.  Integers in [-1000, 1000], four
# columns (sums below 2^24: still exact), and queries that have no two rows at one distance, because an expansion that accepts
# more than 64 rows is merged in rounds of 64 (hnsw_search_body, hnsw_search_big_kernel: "without equal keys the final array
# does not depend on the order"): with equal keys among them the kernels' arrays can differ from the reference's (DESIGN.md
# 4.4.1).  Rows with equal keys under such lists have cases of their own, WIDE_TIES_CASES.
# 62 / 63: the last list that is one word a lane and the first that is walked in chunks (hnsw_wide)
LIST_LENGTHS = (62, 63, 127, 128, 191, 192, 254, 255, 256)
# (rows, dimension, M, efConstruction at which the oracle's graph holds a list of exactly that length)
_LIST_SHAPE = {L: (600, 4, 40, 300) for L in (127, 128, 191, 192)}
_LIST_SHAPE.update({L: (600, 4, 31, 200) for L in (62, 63)})
_LIST_SHAPE.update({254: (1200, 4, 60, 400), 255: (1200, 4, 60, 400), 256: (900, 4, 40, 300)})
G_LIST = {L: _graph(f"list{L}", "l2", n, D, M, efc=efc, maxM=M, maxM0=L, delaunay=0, span=1000)
          for L, (n, D, M, efc) in _LIST_SHAPE.items()}
# The same with equal keys: rows in [-8, 8]^6 and lists of 128 entries (see WIDE_TIES_CASES)
G_LIST_TIES = _graph("list128ties", "l2", 600, 6, 40, efc=300, maxM=40, maxM0=128, delaunay=0)
G_FEW = {n: _graph(f"few{n}", "l2", n, 16, 4, efc=20) for n in (1, 2, 63, 64, 65)}
G_OLD_BIG = _graph("old9000", "l2", 9000, 16, 8)
G_HEAP = {n: _graph(f"heap{n}", "l2", n, 16, 8) for n in (2046, 2047)}
# long rows: the table shrinks (13 968 floats leave the LDS planner 2048 entries at cap 56, 13 976 trip its 64 KiB clause), the
# HBM-array kernel passes 64 KiB of LDS (16 128) and the workgroup's limit (40 704: refused)
G_LONG = {D: _graph(f"long{D}", "l2", 300, D, 8, efc=20, d0=24)
          for D in (13968, 13976, 16120, 16128, 40584, 40592, 40696, 40704)}
# The overflow graph: rows of 7928 floats leave both planners 2048 entries (the LDS planner wants 8192 for maxM0 = 62 and
# ef = 56; SearchOld's too), and a walk marks about 1770 rows.  One thread would build 6000 such rows for most of a minute, and
# a build by all threads gives another graph every time, so the index is built over the first 64 columns and its file widened
# with zeros (widen_optimized_index): the same distances, hence the same graph, in a second.
G_OVER = _graph("over", "l2", 6000, 7928, 31, efc=30, d0=64)
OVER_EF, OVER_POOL, OVER_TABLE = 56, 1000, 2048


def _c(name, graph, nq, k, ef, algo="v1merge", rows="f32", mw=(None,), **expect):
    return Case(name, graph, nq, k, ef, algo, rows, mw, expect)


def _cap_cases(tag, graph, plan, rows="f32"):
    """plan: cap -> (table, emax, kernel under NMSLIB_HNSW_MW=2); every cap once through ef and once through k > ef"""
    out = []
    for cap, (table, emax, kern) in plan.items():
        family = "big" if cap > 1024 else "f16" if rows == "f16" else "lds"
        mw = ("0", "2") if table else (None,)
        for way, k, ef in (("ef", 10, cap), ("k", cap, 5)):
            out.append(_c(f"{tag}_cap{cap}_by_{way}", graph, 64, k, ef, rows=rows, mw=mw, family=family, table=table,
                          emax=emax, kernel=kern))
    return out


# table / bitset flips of the M = 8 graph (maxM0 = 16) and of the M = 16 graph (maxM0 = 32), D = 128; EMAX 2 -> 4 at 128 / 129,
# 4 -> 16 (and multi-wave -> one-wave) at 256 / 257, LDS -> HBM array at 1024 / 1025
PLAN_M8 = {56: (2048, 2, "mw"), 57: (0, 2, "one"), 64: (0, 2, "one"), 65: (4096, 2, "mw"), 113: (4096, 2, "mw"),
           114: (0, 2, "one"), 128: (0, 2, "one"), 129: (8192, 4, "mw"), 227: (8192, 4, "mw"), 228: (0, 4, "one")}
PLAN_M16 = {32: (2048, 2, "mw"), 33: (4096, 2, "mw"), 64: (4096, 2, "mw"), 65: (8192, 2, "mw"), 227: (8192, 4, "mw"),
            228: (0, 4, "one"), 256: (0, 4, "one"), 257: (0, 16, "one"), 1024: (0, 16, "one"), 1025: (0, 0, "big")}
PAIRS = {c: PLAN_M8[c] for c in (56, 57, 227, 228)}
CAP_CASES = (_cap_cases("m8", G8, PLAN_M8) + _cap_cases("m16", G16, PLAN_M16) +
             # no multi-wave kernel for bytes; the fp16 walk
             _cap_cases("sift", G8_SIFT, {c: (t, e, "one") for c, (t, e, _) in PAIRS.items()}) +
             _cap_cases("f16", G8, PAIRS, rows="f16"))
SPACE_CASES = [_c(f"{s}_cap{cap}", g, 64, 10, cap, mw=("0", "2") if table else (None,), family="lds", table=table)
               for s, g in G8_SPACE.items() for cap, table in ((56, 2048), (57, 0))]
# cosine and angular: one case per kernel family (multi-wave and one-wave through mw, HBM array, SearchOld, fp16 walk)
FLOAT_CASES = [c for s, g in G_FLOAT.items() for c in (
    _c(f"{s}_lds", g, 64, 10, 56, mw=("0", "2"), family="lds", table=2048),
    _c(f"{s}_big", g, 64, 10, 1100, family="big"),
    _c(f"{s}_old", g, 64, 10, 56, algo="old", family="old"))]

LIST_CASES = ([_c("maxM0_62", G_M31, 64, 10, 40, mw=("0", "2"), family="lds", wide=False, kernel="mw", table=8192),
               _c("maxM0_64", G_M32, 64, 10, 40, mw=("0", "2"), family="lds", wide=True, kernel="one", table=8192)] +
              # (62 / 63: a table plan, so both kernels at 62; 63 has the one-wave kernel under either setting)
              [_c(f"list{L}_v1merge", G_LIST[L], 64, 10, 40, mw=("0", "2"), family="lds", wide=L > 62,
                  kernel="mw" if L == 62 else "one", table=8192) for L in (62, 63)] +
              [_c(f"list{L}_old", G_LIST[L], 64, 10, 40, algo="old", family="old", wide=L > 62) for L in (62, 63)] +
              [_c(f"list{L}_{algo}", G_LIST[L], 64, 10, 40, algo=algo, wide=True,
                  family="old" if algo == "old" else "big" if L > 255 else "lds")
               for L in LIST_LENGTHS if L > 63 for algo in ("v1merge", "old")])
# Wide lists over rows with equal keys.  An expansion that accepts more than 64 rows is merged into the sorted array in
# rounds of 64, each sorted on its own, where the reference sorts them all together: equal keys can enter in another order, so
# v1merge walks need not equal the oracle's id for id.  What holds under any order of equal keys is checked
# (check_under_ties); SearchOld inserts one by one and equals the oracle exactly.
WIDE_TIES_CASES = [_c("list128ties_v1merge", G_LIST_TIES, 64, 10, 40, family="lds", wide=True),
                   _c("list128ties_big", G_LIST_TIES, 64, 10, 1025, family="big", wide=True),
                   _c("list128ties_old", G_LIST_TIES, 64, 10, 40, algo="old", family="old", wide=True)]
FEW_CASES = [_c(f"few{n}_cap{cap}", g, 64, 70, cap, family="big" if cap > 1024 else "lds", emax=hpr.emax_of(cap) if cap <= 1024 else 0)
             for n, g in G_FEW.items() for cap in (128, 256, 1025)]
LONG_CASES = [
    _c("long_table_2048", G_LONG[13968], 64, 10, 56, mw=("0", "2"), family="lds", table=2048),
    _c("long_clause_64k", G_LONG[13976], 64, 10, 56, family="lds", table=0),
    _c("long_big_below_64k", G_LONG[16120], 64, 10, 1025, family="big"),
    _c("long_big_past_64k", G_LONG[16128], 64, 10, 1025, family="big"),
    _c("long_lds_at_limit", G_LONG[40584], 64, 10, 56, family="lds", table=0),
    _c("long_big_at_limit", G_LONG[40696], 64, 10, 1025, family="big"),
]
LONG_REFUSED = _c("long_refused", G_LONG[40704], 64, 10, 1025, family="big")
# rows the HBM-array kernel still stages (long_big_at_limit) leave the LDS kernels and SearchOld no room for their arrays
LONG_LDS_REFUSED = _c("long_lds_refused", G_LONG[40592], 64, 10, 56, family="lds", table=0)
LONG_OLD_REFUSED = _c("long_old_refused", G_LONG[40592], 64, 10, 56, algo="old", family="old")
OLD_CASES = [
    _c("old_ef8192", G_OLD_BIG, 8, 10, 8192, algo="old", family="old"),
    _c("old_ef8193", G_OLD_BIG, 8, 10, 8193, algo="old", family="old"),
    _c("old_k2048", G_OLD_BIG, 8, 2048, 2100, algo="old", family="old"),
    _c("old_k2049", G_OLD_BIG, 8, 2049, 2100, algo="old", family="old"),
    _c("old_heap_2047", G_HEAP[2046], 64, 10, 100, algo="old", family="old"),
    _c("old_heap_2048", G_HEAP[2047], 64, 10, 100, algo="old", family="old"),
    _c("hybrid_ef999", G16, 64, 10, 999, algo="hybrid", family="lds", emax=16, table=0),
    _c("hybrid_ef1000", G16, 64, 10, 1000, algo="hybrid", family="old"),
]
EXACT_CASES = CAP_CASES + SPACE_CASES + LIST_CASES + FEW_CASES + LONG_CASES + OLD_CASES
ALL_CASES = EXACT_CASES + FLOAT_CASES + WIDE_TIES_CASES + [LONG_REFUSED, LONG_LDS_REFUSED, LONG_OLD_REFUSED]


# ---- corrupted answers (tests/test_hnsw_plan_cpu.py) ---------------------------------------------------------------------
def corrupt(answer, what, q=0):
    ids, ds, cnt, ndc, hops = (np.array(a, copy=True) for a in answer)
    if what == "ids_swapped":
        ids[q, [0, 1]] = ids[q, [1, 0]]
    elif what == "distance_one_ulp":
        ds = np.ascontiguousarray(ds, np.float32)
        ds.view(np.uint32)[q, 1] += 1
    elif what == "count_off":
        cnt[q] -= 1
    elif what == "ndc_off":
        ndc[q] += 1
    elif what == "hops_off":
        hops[q] -= 1
    elif what == "first_launch_output":       # an overflowed query as the LDS-table launch leaves it: no results
        ids[q], ds[q], cnt[q] = -1, np.inf, 0
    else:
        raise ValueError(what)
    return ids, ds, cnt, ndc, hops
