"""The host model of a mutable GPU-built HNSW index (tests/lifecycle_ref.py) without a GPU: it is what
tests/test_gpu_hnsw_lifecycle.py holds the engine to after every append, delete and consolidate, so its parts are held to

  * the builder's restatement: resuming it at `c` on the state a build has there (orc_hnsw_insert_batched) gives the graph
    of the build with a batch boundary at `c`, list for list -- the equality the engine's append claims,
  * composition: a chain of resumes does not depend on how its first graph came about,
  * the consolidate's restatement with the builder's distance: on integer rows the graph of the int64 one it replaces,
  * the witnesses of every scripted sequence and the coverage of the seeded ones, at the row counts the GPU tests use."""
import numpy as np
import pytest

from tests import batched_ref as br
from tests import consolidate_ref, orc
from tests import lifecycle_ref as lr

RESUME_CASES = [name for name, case in br.CASES.items() if case[3].get("post", 0) == 0]


def same_graphs(a, b):
    """two graphs in the keys of refio.parse_index: every list with its padding, levels, offsets, top level, entry point"""
    assert a.keys() == b.keys()
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


def prefix(arrays, c):
    """the first c nodes of a graph whose later nodes have empty lists"""
    up = int(arrays["levels"][:c].sum()) * (arrays["maxM"] + 1)
    assert not arrays["links0"][c:].any() and not arrays["up_links"][up:].any()
    return dict(arrays, n=c, levels=arrays["levels"][:c], links0=arrays["links0"][:c], up_off=arrays["up_off"][:c],
                up_links=arrays["up_links"][:up])


def state_at(space, X, c, params):
    M = params["M"]
    return orc.HnswGraph.batched_state_at(space, X, c, M=M, efConstruction=params["efConstruction"], maxM0=params.get("maxM0"),
                                          delaunay_type=params.get("delaunay_type", 2), batch_div=params.get("gpu_build_div", 0),
                                          max_batch=params.get("gpu_build_batch", 0))


def cuts_of(full):
    """1, a position inside a batch, the last node that rises above the top level and the position before it, n - 1"""
    n, lv = full.n, full.levels()
    inside = int(np.nonzero(full.batch[:, 1] == 1)[0][-1])
    tops = np.maximum.accumulate(lv)
    promoting = int(np.nonzero(lv[1:] > tops[:-1])[0][-1]) + 1
    assert full.batch[inside - 1, 1] == 0 and lv[promoting] > lv[:promoting].max()
    return sorted({1, inside, promoting - 1, promoting, n - 1} - {0})


@pytest.mark.parametrize("name", RESUME_CASES)
def test_resume_equals_the_cut(name):
    space, X, params, _ = br.case_rows(name)
    params.pop("gpu_build_cut", None)
    params.pop("skip_optimized_index", None)
    n = len(X)
    cuts = cuts_of(br.restate(space, X, **params))
    assert len(cuts) >= 4
    for c in cuts:
        state = state_at(space, X, c, params).arrays()
        got = br.resume(space, X, prefix(state, c), c, state["levels"][c:], **params)
        want = br.restate(space, X, gpu_build_cut=c, **params)
        same_graphs(got.arrays(), want.arrays())
        np.testing.assert_array_equal(got.batch[c:, 1], want.batch[c:, 1], err_msg=f"cut {c}: index in the batch")


def test_resume_refuses_what_is_no_append_and_ends_at_once_when_nothing_is_left():
    X = br.make_rows("d16", 60)
    g = br.restate("l2", X, M=6, efConstruction=64)
    before = g.arrays()
    g.insert_batched(60, M=6, efConstruction=64)                 # first == n
    same_graphs(g.arrays(), before)
    for first in (0, 61, 30):                                    # no graph to start from; beyond the rows; lists not empty
        with pytest.raises(ValueError):
            g.insert_batched(first, M=6, efConstruction=64)
    same_graphs(g.arrays(), before)


@pytest.mark.parametrize("space,kind", [("l2", "d16"), ("cosinesimil", "unit"), ("l2sqr_sift", "bytes")])
def test_a_chain_is_a_composition(space, kind):
    """resume to c2 then to n: the same graph whether the graph over X[:c2] was restate(X[:c1]) + resume or the build of
    X[:c2] with a cut at c1"""
    n, c1, c2 = 300, 137, 171
    X, P = br.make_rows(kind, n), dict(lr.PARAMS)
    draws = orc.random_levels(n, P["M"])
    a = br.resume(space, X[:c2], br.restate(space, X[:c1], **P).arrays(), c1, draws[c1:c2], **P)
    b = br.restate(space, X[:c2], gpu_build_cut=c1, **P)
    same_graphs(a.arrays(), b.arrays())
    full = [br.resume(space, X, g.arrays(), c2, draws[c2:], **P).arrays() for g in (a, b)]
    same_graphs(full[0], full[1])
    np.testing.assert_array_equal(full[0]["levels"], draws)
    assert br.restate(space, X, gpu_build_cut=c1, **P).batch[c2, 1] != 0     # (c2 splits a batch of the build cut at c1)


@pytest.mark.parametrize("delaunay", [0, 1, 2])
def test_consolidate_restatement_gives_the_int64_graph_on_integer_rows(delaunay, monkeypatch):
    """the distance of tests/consolidate_ref.py is float64 now (it serves cosine and the dyadic rows); on rows with small
    integer entries it must give, entry for entry, the graph of the int64 squared distance it replaced"""
    n = 600
    X = np.random.default_rng(922).integers(-8, 9, (n, 16)).astype(np.float32)
    g = br.restate("l2", X, M=8, efConstruction=60, delaunay_type=delaunay).arrays()
    dead = np.sort(np.random.default_rng(923).permutation(n)[:n * 3 // 10])
    got, repaired = consolidate_ref.restate(g, X, dead, 60, delaunay)
    R = X.astype(np.int64)
    monkeypatch.setattr(consolidate_ref, "build_distance", lambda space, rows: lambda u, ws: ((R[ws] - R[u]) ** 2).sum(1))
    want, want_repaired = consolidate_ref.restate(g, X, dead, 60, delaunay)
    assert repaired == want_repaired > 0
    same_graphs(got, want)
    consolidate_ref.assert_same_graph(got, want)


def test_consolidate_distance_is_the_builders():
    for space, kind in (("l2", "d16"), ("cosinesimil", "unit"), ("l2sqr_sift", "bytes")):
        X = br.make_rows(kind, 40)
        br.check_exact_inputs(space, X)
        g = br.restate(space, X, M=6, efConstruction=64)
        dist = consolidate_ref.build_distance(space, X)
        for u in (0, 17, 39):
            np.testing.assert_array_equal(dist(u, np.arange(40)), [g.build_distance(u, w) for w in range(40)])


# ---- the scripted sequences --------------------------------------------------------------------------------------------
SCRIPT_ROWS = 300                         # the smallest of 300 / 600 / 1000 at which every script shows its witness


@pytest.mark.parametrize("name", list(lr.scripts(SCRIPT_ROWS)))
def test_script_shows_its_witness(name):
    X = br.make_rows("d16", SCRIPT_ROWS)
    br.check_exact_inputs("l2", X)
    model = lr.HnswModel("l2", **lr.PARAMS)
    w = lr.witness(name, lr.run_script(model, X, lr.scripts(SCRIPT_ROWS)[name]))
    print(name, w)
    assert not model.dead.any() and model.built == model.n       # the script ends in a state that can be saved


@pytest.mark.parametrize("name", ["repair-of-appended", "long"])
def test_small_cut_scripts_have_pools_beyond_the_cut(name):
    model = lr.HnswModel("l2", **lr.SMALL_CUT)
    records = lr.run_script(model, br.make_rows("d16", SCRIPT_ROWS), lr.scripts(SCRIPT_ROWS)[name])
    pools = [r["largest_pool"] for r in records if r["op"] == "consolidate"]
    print(name, lr.witness(name, records), pools)
    assert min(pools) > 12 == min(max(lr.SMALL_CUT["efConstruction"], 2 * lr.SMALL_CUT["M"]), 1024)


def test_the_chain_cuts_lie_inside_batches():
    """the second and third append of `chain` start inside what is one batch for the appends before them"""
    X = br.make_rows("d16", SCRIPT_ROWS)
    steps = lr.scripts(SCRIPT_ROWS)["chain"]
    for i in (2, 3):
        model = lr.HnswModel("l2", **lr.PARAMS)
        lr.run_script(model, X, steps[:i - 1] + [("append", steps[i - 1][1], SCRIPT_ROWS)])
        assert model.last.batch[steps[i][1], 1] != 0, i


@pytest.mark.parametrize("space,kind", [("cosinesimil", "unit"), ("l2sqr_sift", "bytes")])
def test_the_long_script_on_the_other_spaces(space, kind):
    X = br.make_rows(kind, SCRIPT_ROWS)
    br.check_exact_inputs(space, X)
    model = lr.HnswModel(space, **lr.PARAMS)
    print(space, lr.witness("long", lr.run_script(model, X, lr.long_script(SCRIPT_ROWS))))


def test_the_fp16_script_moves_the_scale():
    """rows appended at 8 times the scale stay dyadic (every sum still exact) and hold the largest element"""
    X = lr.f16_rows(SCRIPT_ROWS)
    br.check_exact_inputs("l2", X)
    a = SCRIPT_ROWS // 2
    assert np.abs(X[a:]).max() > 4 * np.abs(X[:a]).max()
    assert (X * 256 == np.round(X * 256)).all() and np.abs(X).max() <= 8


# ---- the seeded sequences ----------------------------------------------------------------------------------------------
def test_every_seed_appends_onto_a_mutated_graph_and_consolidates():
    X = br.make_rows("d16", lr.POOL)
    total = {}
    for seed in lr.SEEDS:
        steps = lr.random_script(seed)
        assert len(steps) == 9
        model = lr.HnswModel("l2", **lr.PARAMS)
        c = lr.random_coverage(lr.run_script(model, X, steps))
        print(seed, c)
        assert c["appends_onto_a_mutated_graph"] >= 1 and c["consolidates"] >= 1, (seed, c)
        assert not model.dead.any() and model.n > 0
        for key, v in c.items():
            total[key] = total.get(key, 0) + v
        total["last-append"] = total.get("last-append", 0) + sum(1 for s in steps if s[0] == "delete" and s[2] == "last-append")
    # an empty delete, a consolidate with nothing marked, a delete of everything an append brought, every row deleted and
    # the build in full that follows once they are consolidated away
    assert all(total[key] >= 1 for key in ("empty_deletes", "idle_consolidates", "last-append", "all_rows_dead",
                                           "rebuilds_from_nothing")), total
