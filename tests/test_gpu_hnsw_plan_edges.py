"""-m gpu: the dense HNSW search at every switch of its launch layer (hnsw_plan.cpp, hnsw_search.cpp, the launch functions of
kernels/hnsw_kernels.hip): table or bitset on either side of every flip, the three array widths, narrow and wide lists up
to the frontier arrays' bound, both kernels of a table plan, fewer rows than the array, long rows, a visited table that
really overflows, and SearchOld's queue placements.

The cases, their graphs, inputs, oracle answers and checkers are tests/hnsw_edge_cases.py; tests/test_hnsw_plan_cpu.py holds
every case's route to the planner, so a case stands on the switch it names.  Integer rows: ids, distance bits, counts, the
(-1, +inf) padding, ndc and hops equal the oracle's on the same graph, without tolerance."""
import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import hnsw_edge_cases as hec, hnsw_plan_ref as hpr, refio
from tests.gpuutil import make_index

pytestmark = pytest.mark.gpu

by_name = lambda c: c.name   # noqa: E731
# graphs whose file is read back and compared with the oracle's build, list for list (the others are built the same way; a
# long-row file holds the rows: one of them)
COMPARED = {g.name for g in (hec.G8, hec.G16, hec.G8_SIFT, hec.G_M32, hec.G_LONG[13968], hec.G_FEW[2], hec.G_FEW[65],
                             hec.G_HEAP[2046])} | {g.name for g in hec.G_LIST.values()}


def saved_graph(idx, tmp_path_factory, name):
    p = str(tmp_path_factory.mktemp("graph") / (name + ".idx"))
    idx.save(p, save_data=False)
    return refio.parse_index(p)


@pytest.fixture(scope="module")
def index_of(tmp_path_factory):
    """the index of a graph, built once per module"""
    built = {}

    def get(g):
        if g.name not in built:
            idx = make_index(g.space, "hnsw", hec.rows(g), **hec.index_params(g))
            built[g.name] = idx
            if g.name in COMPARED:
                got, want = saved_graph(idx, tmp_path_factory, g.name), hec.arrays_of(hec.oracle_graph(g))
                assert (int(got["maxlevel"]), int(got["enterpoint"])) == (want["maxlevel"], want["enterpoint"])
                np.testing.assert_array_equal(got["levels"], want["levels"])
                np.testing.assert_array_equal(got["links0"], want["links0"])
        return built[g.name]
    yield get
    for idx in built.values():
        idx.close()


def search(idx, Q, case, mw, monkeypatch):
    """-> (ids, dists, counts, ndc, hops), stats"""
    if mw is None:
        monkeypatch.delenv("NMSLIB_HNSW_MW", raising=False)
    else:
        monkeypatch.setenv("NMSLIB_HNSW_MW", mw)
    monkeypatch.delenv("NMSLIB_HNSW_MW_MAXQ", raising=False)
    idx.setQueryTimeParams(efSearch=case.ef, algoType=case.algo, gpu_rows=case.rows)
    ids, ds, cnt = idx.knnQueryBatch(Q, case.k)
    ndc, hops, _ = (x.astype(np.int64) for x in idx.read_counters(len(Q)))
    return (ids, ds, cnt, ndc, hops), idx.stats()


def run_case(case, index_of, monkeypatch, check):
    g = case.graph
    idx = index_of(g)
    want = hec.reference(case)
    for mw in case.mw:
        got, st = search(idx, hec.queries(g, case.nq), case, mw, monkeypatch)
        assert st["last_path"] == hec.route_of(case, mw).path, (mw, st)
        if hec.route_of(case, mw).table:
            # no walk of these cases fills its table: nothing is re-run, the kernel named is the one compared
            assert st["hnsw_redone"] == 0, (mw, st)
        check(got, want)


@pytest.mark.parametrize("case", hec.CAP_CASES, ids=by_name)
def test_cap_on_both_sides_of_every_flip(case, index_of, monkeypatch):
    """table <-> bitset at 56/57, 64/65, 113/114, 128/129, 227/228 (M = 8) and 32/33, 64/65, 227/228 (M = 16); EMAX 2 -> 4 ->
    16 at 128/129 and 256/257; LDS -> HBM array at 1024/1025; each cap once through ef and once through k > ef; a table plan
    under NMSLIB_HNSW_MW=0 and =2; the 56/57 and 227/228 pairs again on bytes and on the fp16 walk"""
    run_case(case, index_of, monkeypatch, hec.check_exact)


@pytest.mark.parametrize("case", hec.SPACE_CASES, ids=by_name)
def test_other_spaces_at_the_first_flip(case, index_of, monkeypatch):
    run_case(case, index_of, monkeypatch, hec.check_exact)


@pytest.mark.parametrize("case", hec.LIST_CASES, ids=by_name)
def test_list_lengths(case, index_of, monkeypatch):
    """maxM0 62 / 64 and a longest list of exactly 62 / 63 entries: narrow -> wide lists, which ends the multi-wave kernel; a
    longest list of exactly 127, 128, 191, 192, 254 and 255 entries in the LDS kernels' frontier arrays (64 .. 256 entries), 256 in the HBM-array kernel; SearchOld on
    the same graphs"""
    run_case(case, index_of, monkeypatch, hec.check_exact)


@pytest.mark.parametrize("case", hec.WIDE_TIES_CASES, ids=by_name)
def test_wide_lists_over_rows_with_equal_keys(case, index_of, monkeypatch):
    """Lists of 128 entries over rows in [-8, 8]^6: expansions accept more than 64 rows, among them rows at equal distances.
    The LDS and the HBM-array kernel merge those in rounds of 64 and may take equal keys in another order than the reference
    (DESIGN.md 4.4.1): their answers are held to what no such order changes (hec.check_under_ties), and the number of queries
    that differ from the oracle is printed, not asserted (list128ties_v1merge: 3 of 64).  SearchOld equals the oracle exactly."""
    g = case.graph
    want = hec.reference(case)
    got, st = search(index_of(g), hec.queries(g, case.nq), case, None, monkeypatch)
    assert st["last_path"] == 4
    differ = int((got[0] != want[0]).any(axis=1).sum())
    print(f"{case.name}: {differ} of {case.nq} queries differ from the oracle in an id, "
          f"{int((got[3] != want[3]).sum())} in ndc")
    if case.algo == "old":
        hec.check_exact(got, want)
    else:
        hec.check_under_ties(g, hec.short_queries(g, case.nq), got, want)


@pytest.mark.parametrize("case", hec.FEW_CASES, ids=by_name)
def test_fewer_rows_than_the_array(case, index_of, monkeypatch):
    run_case(case, index_of, monkeypatch, hec.check_exact)


@pytest.mark.parametrize("case", hec.LONG_CASES, ids=by_name)
def test_long_rows(case, index_of, monkeypatch):
    """the smallest table kept up to 64 KiB of LDS and the bitset beyond; the HBM-array kernel below and past 64 KiB of
    dynamic LDS; both kernel families at the longest rows a workgroup's LDS holds"""
    run_case(case, index_of, monkeypatch, hec.check_exact)


def test_rows_beyond_a_workgroups_lds_are_refused(index_of):
    case = hec.LONG_REFUSED
    idx = index_of(case.graph)
    idx.setQueryTimeParams(efSearch=case.ef, algoType=case.algo)
    with pytest.raises(nz.NmslibError) as e:
        idx.knnQueryBatch(hec.queries(case.graph, 8), case.k)
    assert e.value.code == 6, e.value
    idx.setQueryTimeParams(efSearch=20)
    with pytest.raises(nz.NmslibError) as e:
        idx.knnQueryBatch(hec.queries(case.graph, 8), 5)
    assert e.value.code == 6, e.value


@pytest.mark.parametrize("case", [hec.LONG_LDS_REFUSED, hec.LONG_OLD_REFUSED], ids=by_name)
def test_rows_that_fit_only_the_hbm_array_kernel(case, index_of, monkeypatch):
    """8 floats past long_lds_at_limit: the LDS kernels' plan and SearchOld's pass a workgroup's LDS and are refused by name
    (QueryTooLarge, 6), not with a HIP error; the HBM-array kernel (cap > 1024) still answers on the same index"""
    g = case.graph
    idx = index_of(g)
    idx.setQueryTimeParams(efSearch=case.ef, algoType=case.algo)
    with pytest.raises(nz.NmslibError) as e:
        idx.knnQueryBatch(hec.queries(g, case.nq), case.k)
    assert e.value.code == 6, e.value
    big = case._replace(name="long_big_behind_" + case.name, ef=1025, algo="v1merge", expect={})
    got, st = search(idx, hec.queries(g, big.nq), big, None, monkeypatch)
    assert hec.route_of(big).family == "big"
    hec.check_exact(got, hec.reference(big))


@pytest.mark.parametrize("case", hec.OLD_CASES, ids=by_name)
def test_search_old_queue_placement_and_hybrid(case, index_of, monkeypatch):
    """closest queue in LDS / HBM at ef 8192 / 8193, result queue at k 2048 / 2049, the whole heap in LDS at n + 1 = 2047
    against 2048, hybrid at ef 999 (the LDS kernel, EMAX 16) and 1000 (SearchOld)"""
    run_case(case, index_of, monkeypatch, hec.check_exact)


@pytest.mark.parametrize("case", hec.FLOAT_CASES, ids=by_name)
def test_cosine_and_angular_once_per_kernel_family(case, index_of, monkeypatch):
    run_case(case, index_of, monkeypatch, lambda got, want: hec.check_float(case.graph.space, got, want))


# ---- a visited table that overflows ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def over(tmp_path_factory, request):
    """The overflow index (rows of 7928 floats: 2048 table entries where 8192 are wanted): built by one thread over the first
    64 columns, its file widened with zeros and loaded; the pool of queries with the oracle's answers and its prediction of
    who overflows; the two batches"""
    g = hec.G_OVER
    tmp = tmp_path_factory.mktemp("over")
    short = make_index(g.space, "hnsw", hec.short_rows(g), **hec.index_params(g))
    short.save(str(tmp / "short.idx"), save_data=False)
    short.close()
    saved = refio.parse_optimized_index(str(tmp / "short.idx"))
    og = hec.oracle_graph(g)
    np.testing.assert_array_equal(saved["links0"], og.links0())
    np.testing.assert_array_equal(saved["levels"], og.levels())
    hec.widen_optimized_index(str(tmp / "short.idx"), str(tmp / "long.idx"), g.D)
    idx = nz.Index.load(str(tmp / "long.idx"), load_data=False)
    request.addfinalizer(idx.close)
    Q = hec.short_queries(g, hec.OVER_POOL)
    answer = og.search(Q, 10, hec.OVER_EF)
    upper = hec.upper_evaluations(saved, hec.short_rows(g), Q)
    is_over = hec.overflows(answer[3], upper, hec.OVER_TABLE)
    return dict(idx=idx, og=og, answer=answer, upper=upper, over=is_over, batches=dict(zip("ab", hec.pick_batches(is_over))))


@pytest.mark.parametrize("mw", ["2", "0"])
@pytest.mark.parametrize("batch", ["a", "b"])
def test_visited_table_overflow(over, batch, mw, monkeypatch):
    """Batch a: more overflowing queries than the 128 workgroups of the second launch, so workgroups take a second query
    from the list and clear and reuse their bitset; batch b: overflowing queries among others.  The first launch runs the
    multi-wave kernel (mw 2) or the one-wave kernel (mw 0).

    A walk gives up once it has marked more than 7/8 of its table's 2048 entries, 1792.  What it has marked is the entry
    point of level 0 and every row evaluated on level 0 (hec.marked_rows), and ndc counts those evaluations, the entry
    point's and the descent's, so marked = ndc - (evaluations above level 0): exact, from the oracle's ndc on the same
    graph and a restatement of the descent.  hnsw_redone equals the predicted count; every query, re-run or not, equals
    the oracle."""
    g, sel = hec.G_OVER, over["batches"][batch]
    predicted = int(over["over"][sel].sum())
    marked = hec.marked_rows(over["answer"][3], over["upper"])
    print(f"batch {batch}: {len(sel)} queries, {predicted} predicted to overflow; rows marked over the pool "
          f"{marked.min()} / {np.median(marked)} / {marked.max()}")
    assert (predicted > hpr.FIX_SLOTS and len(sel) == 300) if batch == "a" else (0 < predicted < len(sel) == 100)
    assert predicted < len(sel)
    case = hec.Case("over_" + batch, g, len(sel), 10, hec.OVER_EF, "v1merge", "f32", (mw,), {})
    r = hec.route_of(case, mw)
    assert (r.table, r.kernel, r.fix_slots) == (hec.OVER_TABLE, "mw" if mw == "2" else "one", min(len(sel), 128))
    got, st = search(over["idx"], hec.queries(g, hec.OVER_POOL)[sel], case, mw, monkeypatch)
    print(f"hnsw_redone {st['hnsw_redone']}")
    hec.check_redone(st["hnsw_redone"], predicted)
    hec.check_exact(got, tuple(x[sel] for x in over["answer"]))


def test_search_old_retries_with_bitsets(over, monkeypatch):
    """SearchOld's planner leaves the same 2048 entries on these rows.  Its kernel counts as the LDS kernels do (nvisited = 1,
    then += the unvisited neighbours of every expansion; status 1 once that passes 7/8 of the table), and ndc = 1 + the
    descent's evaluations + the same sum, so the oracle's SearchOld ndc predicts exactly which queries of the batch report
    status 1 in the first attempt.  The host then runs the batch again with bitsets; the engine reports the number of those
    queries as hnsw_redone, which is how the retry is observed: it equals the prediction, and the answers equal the oracle."""
    g, sel = hec.G_OVER, over["batches"]["a"][:64]
    Q = hec.short_queries(g, hec.OVER_POOL)[sel]
    want = over["og"].search(Q, 10, hec.OVER_EF, algo="old")
    assert hec.overflows(want[3], over["upper"][sel], hec.OVER_TABLE).any()
    assert hpr.make_plan_old(False, g.n, g.D, g.maxM, g.maxM0, 10, hec.OVER_EF).table_size == hec.OVER_TABLE
    case = hec.Case("over_old", g, len(sel), 10, hec.OVER_EF, "old", "f32", (None,), {})
    got, st = search(over["idx"], hec.queries(g, hec.OVER_POOL)[sel], case, None, monkeypatch)
    predicted = int(hec.overflows(want[3], over["upper"][sel], hec.OVER_TABLE).sum())
    print(f"SearchOld: hnsw_redone {st['hnsw_redone']}, predicted {predicted} of {len(sel)}")
    hec.check_redone(st["hnsw_redone"], predicted)
    hec.check_exact(got, want)
    # a batch that fills no table reports none
    calm = hec.Case("over_old_calm", g, 8, 10, 10, "old", "f32", (None,), {})
    got, st = search(over["idx"], hec.queries(g, hec.OVER_POOL)[sel[:8]], calm, None, monkeypatch)
    assert st["hnsw_redone"] == 0
    hec.check_exact(got, over["og"].search(Q[:8], 10, 10, algo="old"))
