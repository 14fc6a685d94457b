"""The sequential restatement of the batched GPU HNSW builder (orc_hnsw_build_batched, oracle/knn_oracle.c)
without a GPU: it is what tests/test_gpu_hnsw_build_exact.py holds the kernels to, so it is itself held to

  * the reference's sequential insertion (orc_hnsw_build, pinned against the reference) where the two rules coincide,
  * the prefix property of the schedule (a batch looks at nothing behind it),
  * its own witness counters at the row counts the GPU cases use,
  * the host sanitizers, as a stand-alone program (tests/hnsw_batched_ref_check.c).

The file readers and the comparison helper of tests/refio.py are checked here too, on files written from the restatement."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import batched_ref as br
from tests import orc, refio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def level_sets(g):
    lv = g.levels()
    l0 = g.links0()
    out = []
    for i in range(g.n):
        row = [frozenset(l0[i, 1:1 + l0[i, 0]].tolist())]
        for l in range(1, lv[i] + 1):
            L = g.links_up(i, l)
            row.append(frozenset(L[1:1 + L[0]].tolist()))
        out.append(row)
    return out


def tie_free_gauss(n, d):
    """iid Gaussian rows in which, seen from any row, no two distances are closer than 1e-6 relative -- far more than the
    few ulp by which two summation orders differ (the two builders sum differently), so both order every pair alike.
    The first seed that gives such rows; the criterion looks at the rows alone."""
    for seed in range(200):
        X = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
        Xd = X.astype(np.float64)
        D = ((Xd[:, None, :] - Xd[None, :, :]) ** 2).sum(-1)
        r = np.sort(D, axis=1)[:, 1:]
        if not (np.diff(r, axis=1) <= 1e-6 * r[:, 1:]).any():
            return X
    raise AssertionError("no tie-free rows found")


@pytest.mark.parametrize("delaunay", [0, 2])
@pytest.mark.parametrize("n", [60, 130, 200])
def test_one_node_batches_are_sequential_insertion(n, delaunay):
    """batch_div above n: every batch is one node; efConstruction >= n: every search returns its whole level; no distance
    ties: the batched rule is then Hnsw::add, and the restatement must give orc_hnsw_build's graph (lists as sets: the
    reference's delaunay_type 0 shrink keeps list order, the builder's re-sorts).  M = 4: lists overflow."""
    X = tie_free_gauss(n, 8)
    a = orc.HnswGraph.build("l2", X, M=4, efConstruction=256, delaunay_type=delaunay)
    b = orc.HnswGraph.build_batched("l2", X, M=4, efConstruction=256, delaunay_type=delaunay, batch_div=1 << 20)
    assert b.stats["largest_batch"] == 1 and b.stats["shrinks"] > 0 and b.stats["mates"] == 0
    np.testing.assert_array_equal(a.levels(), b.levels())
    assert (a.maxlevel, a.enterpoint) == (b.maxlevel, b.enterpoint)
    assert a.levels().max() > 0
    assert level_sets(a) == level_sets(b)


@pytest.mark.parametrize("params", [dict(M=6, efConstruction=100), dict(M=6, efConstruction=20, gpu_build_div=1),
                                    dict(M=3, maxM0=6, efConstruction=100, gpu_build_div=4, gpu_build_batch=48),
                                    dict(M=16, efConstruction=40, delaunay_type=1)],
                         ids=["default", "doubling", "tall-capped", "heuristic1"])
def test_prefix_property(params):
    """For a batch boundary m, the graph of X[:m] is the state the build of X with a cut at m has at m -- in list order,
    on every level, with the top level and the entry point: nothing in the schedule or the linking looks behind the batch.
    And a cut on a boundary changes nothing: the graph of X with that cut is the graph of X."""
    X = br.make_rows("d16", 300)
    full = br.restate("l2", X, **params)
    starts = np.nonzero(full.batch[:, 1] == 0)[0]                # first node of every batch = a boundary
    starts = [int(m) for m in starts if m >= 1]
    assert max(full.batch[:, 1]) >= 2 and len(starts) >= 8
    p = dict(M=params["M"], efConstruction=params["efConstruction"], maxM0=params.get("maxM0"),
             delaunay_type=params.get("delaunay_type", 2), batch_div=params.get("gpu_build_div", 0),
             max_batch=params.get("gpu_build_batch", 0))
    for m in starts[1::3] + starts[-1:]:
        pre = br.restate("l2", X[:m], **params)
        state = orc.HnswGraph.batched_state_at("l2", X, m, **p)
        assert (pre.maxlevel, pre.enterpoint) == (state.maxlevel, state.enterpoint), m
        np.testing.assert_array_equal(pre.levels(), state.levels()[:m])
        np.testing.assert_array_equal(pre.links0(), state.links0()[:m], err_msg=f"level 0, m={m}")
        assert not state.links0()[m:].any()
        for i in np.nonzero(pre.levels() > 0)[0]:
            for l in range(1, pre.levels()[i] + 1):
                np.testing.assert_array_equal(pre.links_up(i, l), state.links_up(i, l), err_msg=f"node {i} level {l}, m={m}")
    m = starts[len(starts) // 2]
    cut = br.restate("l2", X, gpu_build_cut=m, **params)
    np.testing.assert_array_equal(cut.links0(), full.links0())
    np.testing.assert_array_equal(cut.flat_upper()[1], full.flat_upper()[1])
    inside = int(np.nonzero(full.batch[:, 1] == 1)[0][-1])       # second node of a batch: a cut there splits the batch
    split = br.restate("l2", X, gpu_build_cut=inside, **params)
    assert split.stats["batches_at_cut"] == 1 and split.batch[inside, 1] == 0 and split.batch[inside - 1, 1] == 0


@pytest.mark.parametrize("name", list(br.CASES))
def test_case_shows_its_witness_at_its_row_count_and_not_below(name):
    """every case of the GPU comparison exercises what it is there for, by the restatement's own counters, at the smallest
    row count of batched_ref.ROWS that does (the cases with a cluster are given by what lies in front of it: `clustered`
    has about 1000 iid rows there, 1500 in all, although the count is reached with 300 in front); and its rows are exact
    in f32 in any summation order"""
    space, kind, n, params, witness = br.CASES[name]
    X = br.make_rows(kind, n)
    br.check_exact_inputs(space, X)
    g = br.restate(space, X, **params)
    assert all(g.stats[k] >= v for k, v in witness.items()), g.stats
    smaller = [r for r in br.ROWS if r < n]
    if smaller and kind != "cluster16":
        s = br.restate(space, br.make_rows(kind, smaller[-1]), **params)
        assert not all(s.stats[k] >= v for k, v in witness.items()), s.stats


def test_restatement_standalone_under_host_sanitizers(tmp_path):
    """tests/hnsw_batched_ref_check.c links oracle/knn_oracle.c and runs the restatement over three of the small
    configurations, the tiny graphs and one resumed build (orc_hnsw_insert_batched) under -fsanitize=address,undefined; the hash it prints for every graph is the one
    of the graph the library (no sanitizer) builds from the same rows."""
    exe = str(tmp_path / "hnsw_batched_ref_check")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I" + os.path.join(ROOT, "oracle"),
                           os.path.join(ROOT, "tests", "hnsw_batched_ref_check.c"),
                           os.path.join(ROOT, "oracle", "knn_oracle.c"), "-lm", "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "hnsw batched restatement ok" in run.stdout, run.stdout + run.stderr

    def rows(n, dim):
        x, out = 12345, np.zeros(n * dim, np.float32)
        for i in range(n * dim):
            x = (x * 1103515245 + 12345) & 0x7FFFFFFF
            out[i] = (((x >> 16) & 511) - 256) / 256.0
        return out.reshape(n, dim)

    def graph_hash(g):
        mask = (1 << 64) - 1
        h = (g.maxlevel * 1000003 + g.enterpoint) & mask
        lv, l0 = g.levels(), g.links0()
        for i in range(g.n):
            for l in range(lv[i] + 1):
                L = l0[i] if l == 0 else g.links_up(i, l)
                for j in range(L[0] + 1):
                    h = (h * 1000003 + int(L[j])) & mask
        return h

    want = [("core-narrow", 300, dict(M=6, efConstruction=100)),
            ("doubling-efc100", 300, dict(M=6, efConstruction=100, gpu_build_div=1)),
            ("post1-d1", 300, dict(M=6, efConstruction=100, delaunay_type=1, post=1))] + \
           [("tiny", n, dict(M=6, efConstruction=100, post=2)) for n in (1, 2, 3)] + \
           [("resume-at-137", 300, dict(M=6, efConstruction=100, gpu_build_cut=137))]
    lines = run.stdout.strip().splitlines()[:-1]
    assert len(lines) == len(want)
    for line, (name, n, params) in zip(lines, want):
        g = br.restate("l2", rows(n, 16), **params)
        assert line.split()[:3] == [name, f"n={n}", f"hash={graph_hash(g)}"], line


# ---- the file readers and the comparison helper ----------------------------------------------------------------------
def write_regular(path, g, M):
    """Engine::save's regular file (SaveRegularIndexBin, hnsw.cc:808-840), from a restatement"""
    lv, l0 = g.levels(), g.links0()
    with open(path, "wb") as f:
        f.write(struct.pack("<IIiIQQQ", 0, g.n, g.maxlevel, g.enterpoint, M, g.maxM, g.maxM0))
        for i in range(g.n):
            f.write(struct.pack("<I", lv[i]))
            for l in range(lv[i] + 1):
                L = l0[i] if l == 0 else g.links_up(i, l)
                f.write(struct.pack("<I", L[0]))
                f.write(np.ascontiguousarray(L[1:1 + L[0]], np.int32).tobytes())
        f.write(b"GFXKNNv1" + b"l2sqr_sift".ljust(24, b"\0"))


def test_regular_index_reader_and_comparison_helper(tmp_path):
    X = br.make_rows("bytes", 300)
    g = br.restate("l2sqr_sift", X, M=3, maxM0=6, efConstruction=30)
    path = str(tmp_path / "regular.idx")
    write_regular(path, g, 3)
    got = refio.parse_index(path)
    assert (got["n"], got["M"], got["maxM"], got["maxM0"]) == (300, 3, 3, 6) and got["levels"].max() >= 2
    np.testing.assert_array_equal(got["links0"], g.links0())
    np.testing.assert_array_equal(got["up_off"], g.flat_upper()[0])
    np.testing.assert_array_equal(got["up_links"], g.flat_upper()[1])
    refio.assert_graph_equals_restatement(got, g)
    # two entries of one list swapped, on level 0 and above it: named with the node inserted first
    tall = int(np.nonzero((got["levels"] > 0) & (np.arange(300) > 40))[0][0])
    assert got["up_links"][got["up_off"][tall]] >= 2
    for level, node in ((0, 250), (1, tall)):
        bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in got.items()}
        for victim in (node, 299 if level == 0 else None):
            if victim is None:
                continue
            L = refio._list_of(bad, victim, level)
            L[1], L[2] = L[2], L[1]
        with pytest.raises(AssertionError) as e:
            refio.assert_graph_equals_restatement(bad, g)
        msg = str(e.value)
        assert f"node {node} (level {got['levels'][node]}) on level {level}, batch {g.batch[node, 0]}, index {g.batch[node, 1]}" \
            in msg and "restatement:" in msg, msg
    for key, val in (("enterpoint", got["enterpoint"] + 1), ("maxM0", 7)):
        with pytest.raises(AssertionError):
            refio.assert_graph_equals_restatement(dict(got, **{key: val}), g)
    # padding behind a count (the optimized file has it) must be zeros
    padded = dict(got, links0_raw=got["links0"].copy(), up_links_raw=got["up_links"].copy())
    refio.assert_graph_equals_restatement(padded, g)
    short = int(np.nonzero(got["links0"][:, 0] < 6)[0][0])
    padded["links0_raw"][short, 6] = 5
    with pytest.raises(AssertionError, match="padding"):
        refio.assert_graph_equals_restatement(padded, g)
