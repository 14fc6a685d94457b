"""The plan of the exact scans over sparse, string and divergence rows (scan_make_plan, nmslib_zig_amd/csrc/kernels/
kernels.hpp) without a GPU: the Python restatement against the C++ on a grid, the plan's invariants, the plan of every case
of tests/scan_edge_cases.py, the conditions on those cases' inputs, and the checkers against corrupted answers."""
import os
import subprocess

import numpy as np
import pytest

from tests import diverg_ref, scan_edge_cases as sec, scan_plan_ref as spr, string_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRID_N = (1, 63, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 12289, 100000)
GRID_NQ = (1, 7, 8, 9, 15, 16, 17, 16376, 16377, 32752, 32753)
GRID_K = (1, 256, 257, 768, 769, 1024, 1025, 2730, 2731, 4096, 4097, 8192, 8193)
GRID_TQ = (1, 8, 16)


@pytest.fixture(scope="module")
def printed_plans(tmp_path_factory):
    """tests/scan_plan_check.cpp includes kernels.hpp as it is and prints scan_make_plan over the grid; built as a
    stand-alone program under the host sanitizers"""
    exe = str(tmp_path_factory.mktemp("scan_plan") / "scan_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(ROOT, "tests", "scan_plan_check.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "scan plan ok" in run.stdout, run.stdout[-2000:] + run.stderr[-2000:]
    plans = {}
    for line in run.stdout.splitlines():
        f = line.split()
        if len(f) == 9:
            v = [int(x) for x in f]
            plans[tuple(v[:4])] = tuple(v[4:])
    return plans


def test_restatement_equals_the_planner_on_the_grid(printed_plans):
    want = {(n, nq, k, tq) for n in GRID_N for nq in GRID_NQ for k in GRID_K for tq in GRID_TQ}
    assert set(printed_plans) == want
    for (n, nq, k, tq), got in printed_plans.items():
        p = spr.plan(n, nq, k, tq)
        assert (p.nsplit, p.rows_per_split, p.kl, p.P, p.tq) == got, (n, nq, k, tq)


def test_plan_invariants_on_the_grid(printed_plans):
    for (n, nq, k, tq), (nsplit, rps, kl, P, tq_out) in printed_plans.items():
        at = (n, nq, k, tq)
        assert nsplit >= 1 and nsplit * rps >= n and (nsplit - 1) * rps < n, at
        assert kl <= rps and kl == min(k, rps), at
        assert P >= kl + 256 and P & (P - 1) == 0, at
        if k <= 4096:
            assert nsplit * k <= 8192, at
        assert tq_out in (1, tq) and (tq_out == 1 or P <= 1024), at
        last = spr.plan(n, nq, k, tq).last_rows
        assert 1 <= last <= rps, at


def test_the_switches_fall_where_the_cases_stand():
    """the switches of the planner, one by one, from the restatement (which the grid test holds to the C++)"""
    assert (spr.plan(1024, 1, 10, 8).nsplit, spr.plan(1025, 1, 10, 8).nsplit) == (1, 2)            # the row floor
    assert (spr.plan(2049, 8, 256, 8).P, spr.plan(2049, 8, 257, 8).P) == (512, 1024)               # key buffer
    for tq in (8, 16):                                                                               # tile size
        assert (spr.plan(3000, 9, 768, tq).tq, spr.plan(3000, 9, 769, tq).tq) == (tq, 1)
        assert (spr.plan(3000, 9, 768, tq).P, spr.plan(3000, 9, 769, tq).P) == (1024, 2048)
    assert (spr.plan(3000, 3, 2730, 8).nsplit, spr.plan(3000, 3, 2731, 8).nsplit) == (3, 2)        # merge bound 8192 / k
    assert (spr.plan(5000, 3, 4096, 8).rows_per_split, spr.plan(5000, 3, 4097, 8).rows_per_split) == (2500, 4096)
    assert (spr.merge_route(1, 8192), spr.merge_route(1, 8193)) == ("lds", "bisect")               # merge kernel
    assert (spr.merge_route(2, 4096), spr.merge_route(2, 4097)) == ("lds", "bisect")
    assert (spr.plan(1100, 16376, 5, 8).nsplit, spr.plan(1100, 16377, 5, 8).nsplit) == (2, 1)      # 2047 / 2048 tiles
    # the slices of a batch: 32 768 queries, 2^25 split keys
    assert [(q0, m) for q0, m, _ in spr.slices(50, 33000, 5, 8)] == [(0, 32768), (32768, 232)]
    assert [(q0, m) for q0, m, _ in spr.slices(4097, 4100, 4097, 16)] == [(0, 2050), (2050, 2050)]
    assert 2 * 4100 * 4097 > spr.SLICE_KEYS and 2050 % 16 != 0


def test_every_case_names_the_plan_it_takes():
    names = [c.name for c in sec.ALL_CASES]
    assert len(set(names)) == len(names)
    for c in sec.ALL_CASES:
        nq = c.opts["slices"][0][1] if "slices" in c.opts else c.nq
        if "slices" in c.opts:
            got = spr.slices(c.n, c.nq, c.k, c.tq_asked)
            assert tuple((q0, m) for q0, m, _ in got) == c.opts["slices"], c.name
            assert all(p == c.plan for _, _, p in got), c.name
        assert spr.plan(c.n, nq, c.k, c.tq_asked) == c.plan, c.name
        assert spr.merge_route(c.plan.nsplit, c.k) == c.merge, c.name
    # the tiles the engine asks for: 8 for bit_hamming, sparse and one-block leven batches, 1 for multi-block leven
    # batches, 16 for the divergences
    for c in sec.ALL_CASES:
        mw = c.kind == "leven" and c.opts["qlen"] > 64
        assert c.tq_asked == {"ham": 8, "sparse": 8, "leven": 1 if mw else 8, "diverg": 16}[c.kind], c.name
    # the staging edges
    assert sorted(c.opts["bits"] for c in sec.HAM_WIDTHS) == [1, 31, 33, 96, 128, 160, 16384, 16385]
    assert [(c.opts["bits"] + 31) // 32 for c in sec.HAM_WIDTHS] == [1, 1, 2, 3, 4, 5, 512, 513]
    assert [(m + 63) // 64 for m in sec.LEVEN_MW_LENGTHS] == [1, 4, 5, 8, 9, 10]     # kStrMwLds = 4, 8 blocks = 16 KiB of Peq
    # the 256-row chunks of the long-row case: the first two exceed the 16 KiB row stage (kStrRowStage), in split 0 only
    long_case = sec.LEVEN_CASES[4]
    lens = np.array([len(r) for r in sec.leven_inputs(long_case)[0]])
    chunk = np.add.reduceat(lens, np.arange(0, long_case.n, 256))
    assert (chunk[:2] > 16384).all() and (chunk[2:] + 3 <= 16384).all() and long_case.plan.rows_per_split == 1024
    for c in sec.LEVEN_CASES[:4]:
        assert max(len(r) for r in sec.leven_inputs(c)[0]) <= 12
    for c in sec.SPARSE_STAGE_CASES:
        assert sum(len(q[0]) for q in sec.sparse_inputs(c)[1]) == c.opts["q_elems"] and c.nq == 8


# ---- the references ----------------------------------------------------------------------------------------------------
def test_vectorised_references_equal_the_plain_ones_on_a_sample():
    rng = np.random.default_rng(5)
    for case in (sec.HAM_WIDTHS[2], sec.HAM_WIDTHS[4], sec.HAM_PRESSURE[0]):
        B, Q = sec.ham_inputs(case)
        R, QW = sec.pack_words(B), sec.pack_words(Q)
        text_r, text_q = sec.bits_text(B), sec.bits_text(Q)
        d = sec.ham_distances(R, QW)
        for r in rng.integers(0, case.n, size=12).tolist() + [case.n - 1]:
            obj = string_ref.bit_object(text_r[r])
            np.testing.assert_array_equal(obj[:-1], R[r])
            assert obj[-1] == case.opts["bits"]
            for q in (0, case.nq - 1):
                assert d[q, r] == string_ref.bit_hamming(obj, string_ref.bit_object(text_q[q]))
    for case in (sec.LEVEN_CASES[0], sec.LEVEN_CASES[4], sec.LEVEN_MW_CASES[-1]):
        rows, qs = sec.leven_case_inputs(case)
        for q in (qs[0], qs[-1]):
            d = sec.leven_rows_to_query(rows, q)
            for r in rng.integers(0, case.n, size=8).tolist() + [0, 1023, 1024]:
                assert d[r] == string_ref.levenshtein(rows[r], q), (case.name, r)
    d = np.array([[3, 1, 3, 1, 0], [2, 2, 2, 2, 2]])
    pos, dist = sec.topk_exact(d, 7)
    assert pos.tolist() == [[4, 1, 3, 0, 2, -1, -1], [0, 1, 2, 3, 4, -1, -1]]
    assert dist[0].tolist() == [0, 1, 1, 3, 3, np.inf, np.inf]


def _reference(case, k=None):
    return {"ham": sec.ham_reference, "leven": sec.leven_reference, "sparse": sec.sparse_reference}[case.kind](case, k)


def test_multi_block_distances_depend_on_the_rows_letters():
    """a long query against rows of 1-11 bytes: were every row a subsequence of the query, each distance would be the
    difference of the lengths and the blocks' arithmetic would go unchecked.  At most half of the rows may be."""
    rows, by_len = sec.leven_mw_inputs()
    lens = np.array([len(r) for r in rows])
    for m in sec.LEVEN_MW_LENGTHS[1:]:
        for q in by_len[m]:
            d = sec.leven_rows_to_query(rows, q)
            assert (d >= m - lens).all() and (d <= m).all()
            assert np.mean(d == m - lens) <= 0.5, (m, np.mean(d == m - lens))
            assert len(np.unique(d - (m - lens))) >= 5


# ---- conditions on the inputs, from the references alone ----------------------------------------------------------------
@pytest.mark.parametrize("case", sec.INTEGER_CASES, ids=lambda c: c.name)
def test_integer_cases_hold_a_tie_group_across_a_split_boundary(case):
    """every query: two rows of equal distance in different splits, both inside the top k -- otherwise the order of equal
    keys of two split lists goes untested.  (A case of one split has no boundary.)"""
    pos, dist = _reference(case)
    assert np.isfinite(dist[pos >= 0]).all() and (dist[pos >= 0] == np.round(dist[pos >= 0])).all()   # exact in float32
    assert np.abs(dist[pos >= 0]).max() < 2 ** 24
    if case.plan.nsplit == 1 or case.name in sec.NO_BOUNDARY_TIE:
        return
    ok = sec.has_boundary_tie(pos, dist, case.plan.rows_per_split)
    assert ok.all(), f"{case.name}: queries {np.nonzero(~ok)[0][:10].tolist()} hold no tie across a split boundary"
    if case.plan.last_rows == 1:      # the single row of the last split is inside every query's list
        assert (pos == case.n - 1).any(axis=1).all(), case.name


def test_pressure_rows_all_pass_the_running_threshold():
    """query 0 of the append-pressure cases: the distance falls strictly from one pair of rows to the next, so at every
    compaction the kl-th best key so far is worse than every later row (kl >= 2)"""
    for case in sec.HAM_PRESSURE:
        B, Q = sec.ham_inputs(case)
        d = sec.ham_distances(sec.pack_words(B), sec.pack_words(Q[:1]))[0]
        assert (np.diff(d) <= 0).all() and (d[2:] < d[:-2]).all() and d[-1] == d[-2] == 1
        assert case.plan.kl >= 2 and (case.plan.P == case.plan.kl + 256 or case.k == 10)


@pytest.mark.parametrize("space", sec.DIVERG_SPACES)
def test_divergence_cases_hide_at_most_one_percent_of_the_ranks(space):
    for case in sec.DIVERG_SHAPES + [sec.DIVERG_SLICED]:
        pos, d, b = sec.diverg_reference(case, space, case.k)
        assert np.isfinite(d).all() and pos.shape[1] == min(case.k, case.n)
        share = diverg_ref.near_tie_mask(d, b).mean()
        assert share <= 0.01, f"{case.name} {space}: {share:.4f} of the ranks lie inside near_tie_mask"
    s = sec.diverg_sample(sec.DIVERG_SLICED)
    assert len(s) == len(set(s.tolist())) == sec.DIVERG_SAMPLE and {0, 2049, 2050, 4099} <= set(s.tolist())


def test_cosine_case_is_judged_on_distinct_distances():
    """the float case: ids_match_within_ties compares ids where the expected distance is unique -- most ranks here"""
    pos, dist = sec.sparse_reference(sec.SPARSE_COSINE)
    unique = np.mean([len(np.unique(r)) for r in dist]) / dist.shape[1]
    assert unique >= 0.9, unique


# ---- the checkers reject corrupted answers --------------------------------------------------------------------------------
def _rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _tied_ranks(pos, dist, rps):
    """(query, i): ranks i and i + 1 hold equal distances in different splits"""
    split = pos // rps
    q, i = np.nonzero((dist[:, 1:] == dist[:, :-1]) & (pos[:, 1:] >= 0) & (split[:, 1:] != split[:, :-1]))
    return int(q[0]), int(i[0])


EXACT_CORRUPTIBLE = [sec.HAM_SWEEP[3], sec.HAM_SWEEP[13], sec.HAM_SWEEP[19], sec.LEVEN_CASES[0], sec.LEVEN_MW_CASES[-1],
                     sec.SPARSE_CASES[0], sec.SPARSE_STAGE_CASES[1]]


@pytest.mark.parametrize("case", EXACT_CORRUPTIBLE, ids=lambda c: c.name)
def test_exact_checker_rejects_corrupted_answers(case):
    assert case.plan.last_rows == 1
    n, k = case.n, case.k
    want = _reference(case)
    good = sec.answer_of(*want, n)
    sec.check_exact(good, want, n)
    q, i = _tied_ranks(*want, case.plan.rows_per_split)
    assert _rejects(sec.check_exact, sec.swap_ranks(good, q, i, i + 1), want, n), "two tied ids swapped"
    k1 = sec.answer_of(*_reference(case, k + 1), n)
    dropped = sec.drop_row(k1, q, 0, n)                  # position n - 1 is reported as id 0
    assert dropped[0].shape == (case.nq, k) and 0 not in dropped[0][q]
    assert _rejects(sec.check_exact, dropped, want, n), "the single row of the last split dropped"
    for by in (1, -1):
        assert _rejects(sec.check_exact, sec.count_off(good, case.nq - 1, by), want, n), "a count off by one"
    if k > n:
        assert _rejects(sec.check_exact, sec.fill_padding(good, q, n), want, n), "a padding slot holding a real id"
        pad = tuple(a.copy() for a in good)
        pad[1][q, k - 1] = np.float32(3.0)
        assert _rejects(sec.check_exact, pad, want, n), "a padding slot holding a distance"
    else:
        assert not (want[0] < 0).any()


def test_exact_checker_rejects_a_filled_padding_slot_in_every_kind():
    ks = {c.kind for c in EXACT_CORRUPTIBLE if c.k > c.n}
    assert ks == {"ham", "leven"}
    case = sec.SPARSE_CASES[4]                           # sparse, k = 8193 > n = 3000, one list
    want = _reference(case)
    good = sec.answer_of(*want, case.n)
    sec.check_exact(good, want, case.n)
    assert _rejects(sec.check_exact, sec.fill_padding(good, 1, case.n), want, case.n)
    assert _rejects(sec.check_exact, sec.count_off(good, 0, 1), want, case.n)


def test_float_sparse_checker_rejects_corrupted_answers():
    """ids_match_within_ties accepts any order inside a group of EQUAL expected distances by design, so the swap is of two
    ranks whose expected distances differ"""
    case = sec.SPARSE_COSINE
    n, k = case.n, case.k
    want = _reference(case)
    good = sec.answer_of(*want, n)
    sec.check_sparse_float(good, want, n)
    q = 0
    i = int(np.nonzero(np.diff(want[1][q]) > 0)[0][0])
    assert _rejects(sec.check_sparse_float, sec.swap_ranks(good, q, i, i + 1), want, n)
    k1 = sec.answer_of(*_reference(case, k + 1), n)
    victim = int(good[0][q, 3])
    assert _rejects(sec.check_sparse_float, sec.drop_row(k1, q, victim, n), want, n)
    assert _rejects(sec.check_sparse_float, sec.count_off(good, q, -1), want, n)
    off = tuple(a.copy() for a in good)
    off[1][q, 5] *= np.float32(1 + 3e-5)
    assert _rejects(sec.check_sparse_float, off, want, n), "a distance 3e-5 off"


@pytest.mark.parametrize("space", sec.DIVERG_SPACES)
def test_divergence_checker_rejects_corrupted_answers(space):
    def answer(pos, d):
        dist = np.sqrt(d) if diverg_ref.is_metr(space) else d
        return sec.answer_of(pos, dist, case.n)

    case = sec.DIVERG_SHAPES[6]                          # n = k = 4097, a one-row last split
    n, k = case.n, case.k
    want = sec.diverg_reference(case, space, k)
    good = answer(want[0], want[1])
    sec.check_diverg(space, good, want, n)
    ties = diverg_ref.near_tie_mask(want[1], want[2])
    q = 1
    i = int(np.nonzero(~ties[q, :-1] & ~ties[q, 1:])[0][0])
    assert _rejects(sec.check_diverg, space, sec.swap_ranks(good, q, i, i + 1), want, n), "two ids swapped"
    k1 = sec.diverg_reference(case, space, k + 1)       # k + 1 > n: the list ends one slot early
    pad = lambda a, v: np.concatenate([a, np.full((case.nq, 1), v, a.dtype)], axis=1)    # noqa: E731
    ans1 = answer(pad(k1[0], -1), pad(k1[1], np.inf))
    assert _rejects(sec.check_diverg, space, sec.drop_row(ans1, q, 0, n), want, n), "the row of the last split dropped"
    assert _rejects(sec.check_diverg, space, sec.count_off(good, q, -1), want, n), "a count off by one"
    case = sec.DIVERG_SHAPES[0]                          # n = 63: k = 70 > n
    want = sec.diverg_reference(case, space, 70)
    pad = lambda a, v: np.concatenate([a, np.full((case.nq, 7), v, a.dtype)], axis=1)    # noqa: E731
    good = answer(pad(want[0], -1), pad(want[1], np.inf))
    assert good[0].shape == (case.nq, 70) and (good[2] == 63).all()
    sec.check_diverg(space, good, want, case.n)
    assert _rejects(sec.check_diverg, space, sec.fill_padding(good, 0, 63), want, case.n), "a padding slot holding a real id"
    assert _rejects(sec.check_diverg, space, sec.count_off(good, 2, 1), want, case.n), "a count off by one"
