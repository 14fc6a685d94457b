"""-m gpu: the batched GPU HNSW builder equals its sequential restatement, list for list.

The builder is deterministic by construction, so the whole rule it implements -- batches, construction search, batch-mates,
merge, selection, request order, shrink, promotion, post-processing -- is written down as plain sequential C
(orc_hnsw_build_batched in oracle/knn_oracle.c, itself checked by tests/test_hnsw_batched_ref_cpu.py) and the graph the
kernels build is compared with it: levels, top level, entry point, maxM0 and every list of every node on every level,
entry by entry in list order, padding included.  No tolerance and no share of nodes that may differ.

The inputs are ones on which f32 sums are exact in any order (tests/batched_ref.py), so that the wave's reduction order
and the C loop's cannot differ; the equal distances such inputs have stay in, the tie rules are part of what is compared.
angulardist is not here (the device's acosf is a few ulp from the host's): it stays at recall, tests/test_gpu_hnsw_build.py.

Every case asserts, from the restatement's own counters, that it met what it is there for.  Rows per case: the smallest of
300 / 600 / 1000 / 1500 / 2500 at which it does (tests/test_hnsw_batched_ref_cpu.py holds that without a GPU).  Counters
reached (restatement, first pass):

  core-narrow      300  candidate lists > 64: 232, shrinks 211, targets with >= 2 requests 193, merged lists cut 164
  short-efc3       300  lists shorter than M kept whole: 352 (every one)        short-efc20: 15 (the first nodes)
  doubling-efc100  300  largest batch 132, mates cut to 64: 49 nodes, merged lists cut at efC: 194
  doubling-efc200  300  mates cut to 64: 68 nodes, merged lists cut: 34
  capped-cut       300  one batch of max_batch = 48, one batch ended by the cut at 250 (it would have been 240..288)
  clustered       1500  73 requests on one target in one level of one batch (1200 iid rows, then 300 around row 7)
  mates-cap-*      600  300 iid rows, then the cluster, doubling batches, lists of up to 254: mates cut to 64 for 223 (M = 100,
                        delaunay 0) / 200 (M = 64, delaunay 1) nodes, 162 / 158 requests on one target; the 64th mate is
                        selected here (with a cap of 63 the restatement gives another graph; in the other cases it does not)
  tall             300  31 upper-level slices of >= 2 nodes, 107 mates above level 0, a promotion inside a batch
  l1 / linf / negdotprod 300  shrinks 217 / 377 / 219; ties in merge / link order 31 / 23 (l1), 256 / 270 (linf)
  cosinesimil      300  ties in the merge 3395, in the link ordering 2415       l2sqr_sift: 123 and 188
  wide-m64-d0      300  a list of 128 shrunk, 32 (batch, level)s with more targets than nodes linked before
  wide-m100-d0     300  a list of 200 shrunk, 40 such (batch, level)s
  wide-m64-d2     2500  a list of 128 shrunk (7 shrinks: heuristic 2 keeps most lists far below 128), 13 such
  heuristic1       300  top-ups: 279 in select, 1691 in shrink
  post1-d0/1/2     300  second pass in reverse order with batches of up to 16; maxM0 widened from 12 to 17 / 17 / 18
"""
import functools
import time

import numpy as np
import pytest

from tests import batched_ref as br
from tests import refio
from tests.gpuutil import make_index

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement of a case, computed once (never modified) -> (graph, seconds)"""
    space, X, params, witness = br.case_rows(name)
    t = time.perf_counter()
    g = br.restate(space, X, **params)
    return g, time.perf_counter() - t


def saved_graph(idx, tmp_path, name="g.idx"):
    p = str(tmp_path / name)
    idx.save(p, save_data=False)
    return refio.parse_index(p)


def build_and_compare(name, tmp_path):
    space, X, params, witness = br.case_rows(name)
    want, cpu_s = restated(name)
    missing = {k: (want.stats[k], v) for k, v in witness.items() if want.stats[k] < v}
    assert not missing, f"the restatement does not show the witness (counter: reached, needed): {missing}"
    t = time.perf_counter()
    idx = make_index(space, "hnsw", X, gpu_build=1, **params)
    gpu_s = time.perf_counter() - t
    try:
        assert idx.graphBuilder() == 2
        got = saved_graph(idx, tmp_path)
    finally:
        idx.close()
    print(f"{name}: n={len(X)} restatement {cpu_s:.3f} s, build {gpu_s:.3f} s, witness "
          f"{ {k: want.stats[k] for k in witness} }")
    assert ("links0_raw" in got) == (space != "l2sqr_sift")      # (the optimized file carries the padding)
    refio.assert_graph_equals_restatement(got, want)


@pytest.mark.parametrize("name", list(br.CASES))
def test_built_graph_equals_the_restatement(name, tmp_path):
    build_and_compare(name, tmp_path)


@pytest.mark.parametrize("name", ["core-narrow", "wide-m64-d0", "wide-m100-d0", "wide-m64-d2"])
def test_built_graph_equals_the_restatement_with_the_one_wave_search(name, tmp_path, monkeypatch):
    """NMSLIB_HNSW_MW=0: the construction's search step runs the one-wave kernel instead of the workgroup-per-query one"""
    monkeypatch.setenv("NMSLIB_HNSW_MW", "0")
    build_and_compare(name, tmp_path)


@pytest.mark.parametrize("post", [0, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 17])
def test_tiny_graphs(n, post, tmp_path):
    X = br.make_rows("d16", 17)[:n]
    params = dict(M=6, efConstruction=100, post=post)
    idx = make_index("l2", "hnsw", X, gpu_build=1, **params)
    got = saved_graph(idx, tmp_path)
    idx.close()
    refio.assert_graph_equals_restatement(got, br.restate("l2", X, **params))


@pytest.mark.parametrize("space,kind,n0", [("l2", "d16", 137), ("cosinesimil", "unit", 200), ("l2sqr_sift", "bytes", 1)])
def test_appended_graph_equals_the_restatement_with_a_cut(space, kind, n0, tmp_path):
    """build X[:n0], add the other rows (gpu_append=1): the graph of a build of X with a batch boundary at n0 -- here the
    restatement's with cut = n0 (137 and 200 lie inside what are the batches 133..140 and 199..210 without the cut; a start
    from one row is the whole build)"""
    X = br.make_rows(kind, 300)
    params = dict(M=6, efConstruction=64, **({"skip_optimized_index": 1} if space == "l2sqr_sift" else {}))
    want = br.restate(space, X, gpu_build_cut=n0, **params)
    assert want.stats["batches_at_cut"] == (1 if n0 > 1 else 0) and want.batch[n0, 1] == 0
    idx = make_index(space, "hnsw", X[:n0], np.arange(n0, dtype=np.int32), gpu_build=1, gpu_append=1, **params)
    ids = np.arange(n0, 300, dtype=np.int32)
    if X.dtype == np.uint8:
        idx.addUInt8Batch(X[n0:], ids)
    else:
        idx.addDenseBatch(X[n0:], ids)
    idx.finalize()
    assert idx.stats()["rows_appended"] == 300 - n0 and idx.graphBuilder() == 2
    got = saved_graph(idx, tmp_path)
    idx.close()
    refio.assert_graph_equals_restatement(got, want)
