"""-m gpu: the HNSW search that filters inside the walk (query-time parameter gpu_inwalk=1).

The yardstick is exact: the rule is written down as plain sequential Python (tests/inwalk_ref.py, itself checked by
tests/test_hnsw_inwalk_cpu.py) and run over the graph the index saves and the rows.  Ids, distances, counts and the
counters ndc / hops / hops_up must be equal bit for bit, and every such batch must report last_path 8.  The inputs are ones
on which f32 sums are exact in any order (tests/batched_ref.py); the ties such inputs have stay in.  angulardist gets no
exact comparison (the device's acosf is not the host's): eligibility, order and counts.

Every case asserts what it is there for from the restatement's own counters (tests/test_hnsw_inwalk_cpu.py lists what they
reach), the 1-in-8 filter also from the device: the same batch with gpu_inwalk=0 returns fewer than k results."""
import numpy as np
import pytest

from tests import batched_ref as br
from tests import inwalk_ref as ir
from tests import refio
from tests.gpuutil import knn_on_stream, make_index, same_bits

pytestmark = pytest.mark.gpu

HOST, GPU = dict(indexThreadQty=1), dict(gpu_build=1)


def run(idx, Q, k, flt=None):
    """-> (ids, dists, counts), (ndc, hops, hops_up)"""
    res = idx.knnQueryBatch(Q, k) if flt is None else idx.knnQueryBatchFiltered(flt, Q, k)
    return res, tuple(x.copy() for x in idx.read_counters(len(Q)))


def saved_graph(idx, tmp_path, name="g.idx"):
    p = str(tmp_path / name)
    idx.save(p, save_data=False)
    return refio.parse_index(p)


def same_answer(got, ctr, want):
    same_bits(got, want[0])
    for nm, g, w in zip(("ndc", "hops", "hops_up"), ctr, want[1]):
        np.testing.assert_array_equal(g, w, err_msg=nm)


class Case:
    """A case of inwalk_ref.CASES on the device: the index, its graph saved before anything is deleted, the rows marked, the
    filter made, gpu_inwalk=1 set."""

    def __init__(self, name, tmp_path, builder=HOST, **more):
        (self.space, self.X, self.Q, self.ids, build, self.ef, self.k, self.allow, self.dead, _) = ir.case(name)
        self.name = name
        self.idx = make_index(self.space, "hnsw", self.X, self.ids, **dict(build, **builder), **more)
        assert self.idx.graphBuilder() == (1 if builder is HOST else 2)
        self.g = saved_graph(self.idx, tmp_path)
        self.eligible = ir.eligible_of(len(self.X), self.allow, self.dead)
        if builder is HOST:
            np.testing.assert_array_equal(self.g["links0"], ir.host_graph(name)["links0"])   # (the builder is deterministic)
            self.want = ir.restated(name)
        else:
            self.want = ir.search(self.space, self.X, self.Q, self.g, self.k, self.ef, self.eligible, self.ids)
        ir.check_witness(name, self.g, self.want, self.want[2], self.eligible, self.k, self.ef)
        if len(self.dead):
            assert self.idx.deleteIds(self.ids[self.dead]) == len(self.dead)
        self.flt = self.idx.makeFilter(self.allow) if self.allow is not None else None
        self.idx.setQueryTimeParams(efSearch=self.ef, gpu_inwalk=1)

    def run(self, inwalk=1):
        self.idx.setQueryTimeParams(efSearch=self.ef, gpu_inwalk=inwalk)
        return run(self.idx, self.Q, self.k, self.flt)

    def close(self):
        if self.flt is not None:
            self.flt.close()
        self.idx.close()


# ---- exact cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ir.CASES))
def test_equals_the_restatement(name, tmp_path):
    c = Case(name, tmp_path)
    got, ctr = c.run()
    assert c.idx.stats()["last_path"] == 8
    same_answer(got, ctr, c.want)
    c.close()


@pytest.mark.parametrize("builder", [HOST, GPU], ids=["host-built", "gpu-built"])
def test_one_in_eight_filter_returns_k_where_the_two_stages_do_not(builder, tmp_path):
    c = Case("filter-1in8", tmp_path, builder)
    got, ctr = c.run()
    assert c.idx.stats()["last_path"] == 8
    same_answer(got, ctr, c.want)
    assert (got[2] == c.k).all()
    two, _ = c.run(inwalk=0)
    assert c.idx.stats()["last_path"] == 4
    print("counts of the two stages:", np.bincount(two[2], minlength=c.k + 1))
    assert (two[2] < c.k).any()                                  # without it the case shows nothing
    c.close()


def test_rows_appended_after_the_filter_are_walked_but_not_eligible(tmp_path):
    n0, n1 = 1000, 1500
    X, Q = br.make_rows("d16", n1), br.make_rows("d16", ir.NQ, seed=12)
    ids = ir.ext_ids(n1)
    idx = make_index("l2", "hnsw", X[:n0], ids[:n0], gpu_append=1, gpu_build_batch=256, gpu_build=1, **ir.BUILD)
    mask = ir.allow_mask(("share", 8, 41), X[:n0])
    flt = idx.makeFilter(mask)
    idx.addDenseBatch(X[n0:], ids[n0:])
    idx.finalize()
    assert idx.stats()["rows_appended"] == n1 - n0
    g = saved_graph(idx, tmp_path)
    assert g["n"] == n1
    want = ir.search("l2", X, Q, g, ir.K, ir.EF, ir.eligible_of(n1, mask, []), ids)
    # the same walk with the new rows eligible returns some of them: they are in reach, and left out by the filter's length
    every = ir.search("l2", X, Q, g, ir.K, ir.EF, np.r_[mask, np.ones(n1 - n0, bool)], ids)
    assert np.isin(every[0][0], ids[n0:]).any() and not np.isin(want[0][0], ids[n0:]).any()
    idx.setQueryTimeParams(efSearch=ir.EF, gpu_inwalk=1)
    got, ctr = run(idx, Q, ir.K, flt)
    assert idx.stats()["last_path"] == 8
    same_answer(got, ctr, want)
    flt.close()
    idx.close()


def test_an_f16_index_gives_the_bits_of_the_f32_index(tmp_path):
    c = Case("filter-1in8", tmp_path, gpu_rows="f16")
    got, ctr = c.run()
    assert c.idx.stats()["last_path"] == 8                       # (the in-walk kernel reads the f32 rows)
    same_answer(got, ctr, c.want)
    c.close()


# ---- property case -----------------------------------------------------------------------------------------------------
def test_angulardist_returns_k_eligible_rows_in_order():
    n = 1000
    X, Q = br.make_rows("d16", n), br.make_rows("d16", ir.NQ, seed=12)
    ids = ir.ext_ids(n)
    mask = ir.allow_mask(("share", 8, 42), X)
    idx = make_index("angulardist", "hnsw", X, ids, indexThreadQty=1, **ir.BUILD)
    flt = idx.makeFilter(mask)
    idx.setQueryTimeParams(efSearch=ir.EF, gpu_inwalk=1)
    (gi, gd, cnt), _ = run(idx, Q, ir.K, flt)
    assert idx.stats()["last_path"] == 8
    assert (cnt == ir.K).all()
    assert np.isin(gi, ids[mask]).all()
    for q in range(len(Q)):
        assert len(set(gi[q].tolist())) == ir.K
        keys = list(zip(gd[q].tolist(), gi[q].tolist()))         # (ids grow with positions)
        assert keys == sorted(keys), q
    flt.close()
    idx.close()


# ---- fallbacks: the bits of gpu_inwalk=0 -------------------------------------------------------------------------------
def both_settings(idx, Q, k, flt, ef, **params):
    out = []
    for inwalk in (0, 1):
        idx.setQueryTimeParams(efSearch=ef, gpu_inwalk=inwalk, **params)
        out.append(run(idx, Q, k, flt) + (idx.stats()["last_path"],))
    return out


@pytest.mark.parametrize("params", [{}, dict(algoType="v1merge")], ids=["old-by-ef", "hbm-array"])
def test_ef_1025_falls_back_to_the_two_stages(params, tmp_path):
    c = Case("tombstones", tmp_path)                             # (a filter of fewer rows than efSearch would be scanned)
    (r0, c0, p0), (r1, c1, p1) = both_settings(c.idx, c.Q, c.k, c.flt, 1025, **params)
    assert p0 == p1 == 4
    same_bits(r1, r0)
    for a, b in zip(c1, c0):
        np.testing.assert_array_equal(a, b)
    # ... and efSearch = 1024 on the same index is served
    c.idx.setQueryTimeParams(efSearch=1024, gpu_inwalk=1, **params)
    run(c.idx, c.Q, c.k, c.flt)
    assert c.idx.stats()["last_path"] == 8
    c.close()


def test_lists_beyond_254_fall_back_to_the_two_stages():
    n = 600
    X, Q = br.make_rows("d16", n), br.make_rows("d16", ir.NQ, seed=12)
    ids = ir.ext_ids(n)
    idx = make_index("l2", "hnsw", X, ids, M=128, efConstruction=100, delaunay_type=0, indexThreadQty=1)
    flt = idx.makeFilter(ir.allow_mask(("share", 8, 43), X))
    (r0, c0, p0), (r1, c1, p1) = both_settings(idx, Q, ir.K, flt, ir.EF)
    assert p0 == p1 == 4
    same_bits(r1, r0)
    for a, b in zip(c1, c0):
        np.testing.assert_array_equal(a, b)
    flt.close()
    idx.close()


@pytest.mark.parametrize("rows,path", [("f32", 4), ("f16", 5)])
def test_no_tombstone_and_no_filter_runs_what_it_ran(rows, path):
    n = 1000
    X, Q = br.make_rows("d16", n), br.make_rows("d16", ir.NQ, seed=12)
    idx = make_index("l2", "hnsw", X, ir.ext_ids(n), indexThreadQty=1, gpu_rows=rows, **ir.BUILD)
    (r0, c0, p0), (r1, c1, p1) = both_settings(idx, Q, ir.K, None, ir.EF)
    assert p0 == p1 == path
    same_bits(r1, r0)
    for a, b in zip(c1, c0):
        np.testing.assert_array_equal(a, b)
    idx.close()


# ---- other checks ------------------------------------------------------------------------------------------------------
def test_the_subset_route_keeps_precedence():
    n = 1000
    X, Q = br.make_rows("d16", n), br.make_rows("d16", ir.NQ, seed=12)
    idx = make_index("l2", "hnsw", X, ir.ext_ids(n), indexThreadQty=1, **ir.BUILD)
    flt = idx.makeFilter(ir.allow_mask(("near", 7, 20), X))
    assert flt.allowed == 20
    (r0, c0, p0), (r1, c1, p1) = both_settings(idx, Q, ir.K, flt, ir.EF)
    assert p0 == p1 == 7
    same_bits(r1, r0)
    flt.close()
    idx.close()


def test_slices_give_the_bits_of_one_slice(monkeypatch, tmp_path):
    """70 queries cut at 7 through NMSLIB_HNSW_SLICE_MAXQ: results, counts and counters at their offsets"""
    c = Case("tombstones-filter", tmp_path)
    monkeypatch.setenv("NMSLIB_HNSW_SLICE_MAXQ", "7")
    got, ctr = c.run()
    assert c.idx.stats()["last_path"] == 8
    same_answer(got, ctr, c.want)
    c.close()


def test_a_batch_run_twice_gives_equal_bits(tmp_path):
    c = Case("cosinesimil", tmp_path)
    (a, ca), (b, cb) = c.run(), c.run()
    same_bits(a, b)
    for x, y in zip(ca, cb):
        np.testing.assert_array_equal(x, y)
    c.close()


def test_the_device_entry_on_another_stream_equals_the_host_entry(tmp_path):
    c = Case("tombstones", tmp_path)
    got = knn_on_stream(c.idx, c.Q, c.k, q_off=8, out_off=3)
    assert c.idx.stats()["last_path"] == 8
    same_bits(got, c.want[0])
    c.close()
