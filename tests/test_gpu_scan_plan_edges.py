"""-m gpu: the exact scans over sparse vectors, strings and the divergence spaces at every switch of the plan they share
(scan_make_plan, Engine::scan_slices, launch_merge_topk_ex) and at the staging edges of their kernels.

The cases, their inputs, references and checkers are tests/scan_edge_cases.py; tests/test_scan_plan_cpu.py holds every
case's plan to the planner, so a case stands on the switch it names.  Every case checks ids, distances, counts, the
(-1, +inf) padding past the count, and that knnQuery of the first and the last query equals its row of the batch bit for
bit.  External ids run against the positions: equal distances are ordered by position, not by the reported id."""
import pytest

import nmslib_zig_amd as nz
from tests import scan_edge_cases as sec

pytestmark = pytest.mark.gpu

by_name = lambda c: c.name   # noqa: E731


def string_index(space, rows):
    idx = nz.Index(space, "seq_search", data_type="ObjectAsString", dist_type="Int")
    idx.addStringBatch(rows, ids=sec.ext_ids(len(rows)))
    idx.buildIndex()
    return idx


def one_query_equals_its_batch_row(idx, queries, got, k, which=(0, -1)):
    ids, ds, cnt = got
    for q in which:
        i1, d1 = idx.knnQuery(queries[q], k)
        c = int(cnt[q])
        assert len(i1) == c, f"query {q}: knnQuery gives {len(i1)} results, the batch {c}"
        assert i1.tobytes() == ids[q, :c].tobytes(), f"query {q}: ids of knnQuery differ from the batch row"
        assert d1.tobytes() == ds[q, :c].tobytes(), f"query {q}: distances of knnQuery differ from the batch row"


def run_exact(idx, case, queries, want):
    got = idx.knnQueryBatch(queries, case.k)
    sec.check_exact(got, want, case.n)
    one_query_equals_its_batch_row(idx, queries, got, case.k)


# ---- bit_hamming -------------------------------------------------------------------------------------------------------
def run_ham(case):
    B, Q = sec.ham_inputs(case)
    idx = string_index("bit_hamming", sec.bits_text(B))
    run_exact(idx, case, sec.bits_text(Q), sec.ham_reference(case))
    idx.close()


@pytest.mark.parametrize("case", sec.HAM_SWEEP, ids=by_name)
def test_bit_hamming_at_every_plan_switch(case):
    run_ham(case)


def test_bit_hamming_2047_and_2048_tiles():
    """16 376 queries are 2047 tiles and two splits, 16 377 queries 2048 tiles and one split: every query is checked"""
    a, b = sec.HAM_TILES
    B, Q = sec.ham_inputs(b)
    idx = string_index("bit_hamming", sec.bits_text(B))
    text = sec.bits_text(Q)
    for case in (a, b):
        run_exact(idx, case, text[:case.nq], sec.ham_reference(case))
    idx.close()


@pytest.mark.parametrize("case", sec.HAM_PRESSURE, ids=by_name)
def test_bit_hamming_append_pressure(case):
    """every row passes query 0's running threshold: its key buffer fills to P before a compaction, next to the buffers
    of queries 1-7"""
    run_ham(case)


@pytest.mark.parametrize("case", sec.HAM_WIDTHS, ids=by_name)
def test_bit_hamming_widths(case):
    """W = 1-5 words (16-byte loads when W % 4 == 0, else word by word) and W = 512 / 513 (queries staged / in HBM)"""
    run_ham(case)


# ---- leven -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sec.LEVEN_CASES, ids=by_name)
def test_leven_one_block_queries(case):
    rows, qs = sec.leven_inputs(case)
    idx = string_index("leven", rows)
    run_exact(idx, case, qs, sec.leven_reference(case))
    idx.close()


@pytest.mark.parametrize("k", [10, 1030])
def test_leven_multi_block_queries_over_two_splits(k):
    """256 / 257 bytes: the blocks' state in LDS / HBM; 512 / 513 bytes: Peq staged / in HBM; two queries per length, so
    blockIdx.y > 0 in each; the second split holds one row.  One call of knnQueryBatch: the wrapper sends one batch per
    length (the C ABI gives the queries of a batch one length)."""
    rows, by_len = sec.leven_mw_inputs()
    idx = string_index("leven", rows)
    cases = [c for c in sec.LEVEN_MW_CASES if c.k == k]
    assert [c.opts["qlen"] for c in cases] == list(sec.LEVEN_MW_LENGTHS)
    qs = [q for c in cases for q in by_len[c.opts["qlen"]]]
    ids, ds, cnt = idx.knnQueryBatch(qs, k)
    for j, c in enumerate(cases):
        at = slice(j * c.nq, (j + 1) * c.nq)
        got = (ids[at], ds[at], cnt[at])
        sec.check_exact(got, sec.leven_reference(c), c.n)
        one_query_equals_its_batch_row(idx, qs[at], got, k)
    idx.close()


# ---- sparse ------------------------------------------------------------------------------------------------------------
def sparse_index(case, rows):
    idx = nz.Index(case.opts["space"], "seq_search", data_type="SparseVector")
    idx.addSparseBatch(rows, sec.ext_ids(len(rows)))
    idx.buildIndex()
    return idx


@pytest.mark.parametrize("case", sec.SPARSE_CASES + sec.SPARSE_STAGE_CASES, ids=by_name)
def test_sparse_integer_values(case):
    """l1 and the dot product over integer values are exact: equality in (distance, position) order.  The staging
    cases: the eight queries of the one tile hold 4096 elements together (staged in LDS) and 4097 (read from HBM)."""
    rows, qs = sec.sparse_inputs(case)
    idx = sparse_index(case, rows)
    run_exact(idx, case, qs, sec.sparse_reference(case))
    idx.close()


def test_sparse_cosine_float_values():
    case = sec.SPARSE_COSINE
    rows, qs = sec.sparse_inputs(case)
    idx = sparse_index(case, rows)
    got = idx.knnQueryBatch(qs, case.k)
    sec.check_sparse_float(got, sec.sparse_reference(case), case.n)
    one_query_equals_its_batch_row(idx, qs, got, case.k)
    idx.close()


# ---- divergences -------------------------------------------------------------------------------------------------------
def diverg_index(space, rows):
    idx = nz.Index(space, "seq_search")
    idx.addDenseBatch(rows, sec.ext_ids(len(rows)))
    idx.buildIndex()
    return idx


@pytest.mark.parametrize("space", sec.DIVERG_SPACES)
@pytest.mark.parametrize("case", sec.DIVERG_SHAPES, ids=by_name)
def test_divergences(case, space):
    rows, qs = sec.diverg_inputs(case)
    idx = diverg_index(space, rows)
    got = idx.knnQueryBatch(qs, case.k)
    sec.check_diverg(space, got, sec.diverg_reference(case, space, case.k), case.n)
    one_query_equals_its_batch_row(idx, qs, got, case.k)
    idx.close()


def test_divergence_batch_cut_into_slices():
    """2 * 4100 * 4097 split keys > 2^25: the batch goes through in two slices of 2050 queries, no multiple of the tile;
    40 queries are checked, the first and the last of each slice among them"""
    case, space = sec.DIVERG_SLICED, "kldivfast"
    rows, qs = sec.diverg_inputs(case)
    idx = diverg_index(space, rows)
    ids, ds, cnt = idx.knnQueryBatch(qs, case.k)
    assert (cnt == case.n).all() and ids.shape == (case.nq, case.k)
    s = sec.diverg_sample(case)
    got = (ids[s], ds[s], cnt[s])
    sec.check_diverg(space, got, sec.diverg_reference(case, space, case.k), case.n)
    one_query_equals_its_batch_row(idx, qs[s], got, case.k)
    idx.close()
