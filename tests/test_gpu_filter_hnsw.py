"""-m gpu: filtered k-NN on an HNSW index (nmslib_gpu_filter_*).

Walk route.  The yardstick is the one of tests/test_gpu_hnsw_delete.py: on the same index the batch is searched unfiltered
for k' = max(efSearch, k) results; on the host the ids that are not allowed or deleted are dropped and the lists cut to k.
The filtered batch must give those BITS (ids, distances, counts) and the unfiltered run's ndc / hops / hops_up.

Subset route.  Integer-grid rows, on which every f32 distance is exact: the oracle is numpy over the allowed live rows,
ordered by (distance, position); ids, distances and counts are equal bit for bit.  cosinesimil and angulardist are held to
the tolerances tests/test_gpu_hnsw.py uses for them."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import refio
from tests.gpuutil import close_rel, ids_match_modulo_near_ties, make_index, same_bits, sim_close

from . import filter_poison_child

pytestmark = pytest.mark.gpu

HOST = dict(M=8, efConstruction=60, indexThreadQty=1)
GPU = dict(M=8, efConstruction=60, gpu_build=1)


def ext_ids(n):
    """external ids that are no positions (a result that carries positions shows)"""
    return (5 * np.arange(n) + 7).astype(np.int32)


def run(idx, Q, k, flt=None):
    """-> (ids, dists, counts), (ndc, hops, hops_up)"""
    res = idx.knnQueryBatch(Q, k) if flt is None else idx.knnQueryBatchFiltered(flt, Q, k)
    return res, tuple(x.copy() for x in idx.read_counters(len(Q)))


def host_filtered(before, keep_ids, k):
    """the first k entries of every list of `before` whose id is in keep_ids"""
    bids, bds, bcnt = before
    nq = len(bcnt)
    ids = np.full((nq, k), -1, np.int32)
    ds = np.full((nq, k), np.inf, np.float32)
    cnt = np.zeros(nq, np.int32)
    for q in range(nq):
        ok = np.nonzero(np.isin(bids[q, :bcnt[q]], keep_ids))[0][:k]
        ids[q, :len(ok)], ds[q, :len(ok)], cnt[q] = bids[q, ok], bds[q, ok], len(ok)
    return ids, ds, cnt


# ---- walk route -------------------------------------------------------------------------------------------------------
N, D, EF, K, NQ = 20000, 16, 64, 10, 70

WALKS = {
    # name: (space, index parameters, query parameters, last_path)
    "host-built": ("l2", HOST, {}, 4),
    "gpu-built": ("l2", GPU, {}, 4),
    "cosinesimil": ("cosinesimil", GPU, {}, 4),
    "l2sqr_sift": ("l2sqr_sift", GPU, {}, 4),
    "f16": ("l2", dict(GPU, gpu_rows="f16"), {}, 5),
    "old": ("l2", GPU, dict(algoType="old"), 4),
}


@pytest.mark.parametrize("name", list(WALKS))
def test_walk_route(name):
    space, build, qparams, last_path = WALKS[name]
    if space == "l2sqr_sift":
        X, Q = refio.s_sift_like(N, 1101), refio.s_sift_like(NQ, 1102)
    else:
        X, Q = refio.s_lowrank(N, D, 1101), refio.s_lowrank(NQ, D, 1102)
    ids = ext_ids(N)
    idx = make_index(space, "hnsw", X, ids, **build)
    assert idx.graphBuilder() == (1 if build is HOST else 2)
    idx.setQueryTimeParams(efSearch=EF, **qparams)
    before, bctr = run(idx, Q, EF)
    mask = np.random.default_rng(1103).random(N) < 0.5
    flt = idx.makeFilter(mask)
    assert flt.allowed == int(mask.sum()) and flt.hbm_bytes >= N // 8
    for k in (K, 1):
        res, ctr = run(idx, Q, k, flt)
        same_bits(res, host_filtered(before, ids[mask], k))
        for nm, got, want in zip(("ndc", "hops", "hops_up"), ctr, bctr):
            np.testing.assert_array_equal(got, want, err_msg=nm)
    assert idx.stats()["last_path"] == last_path
    # tombstones and the filter together: every query's nearest allowed row goes
    dead = np.unique(res[0][:, 0])
    assert idx.deleteIds(dead) == len(dead)
    res, ctr = run(idx, Q, K, flt)
    keep = np.setdiff1d(ids[mask], dead)
    same_bits(res, host_filtered(before, keep, K))
    for nm, got, want in zip(("ndc", "hops", "hops_up"), ctr, bctr):
        np.testing.assert_array_equal(got, want, err_msg=nm)
    assert flt.allowed == len(keep)
    # an unfiltered batch is the tombstone-only batch it was
    same_bits(run(idx, Q, K)[0], host_filtered(before, np.setdiff1d(ids, dead), K))
    flt.close()
    idx.close()


def test_rows_appended_after_the_filter_are_not_allowed():
    n0, n1 = 2000, 2300
    X, Q = refio.s_lowrank(n1, D, 1104), refio.s_lowrank(NQ, D, 1105)
    ids = ext_ids(n1)
    idx = make_index("l2", "hnsw", X[:n0], ids[:n0], gpu_append=1, gpu_build_batch=256, **GPU)
    idx.setQueryTimeParams(efSearch=EF)
    mask = np.arange(n0) % 2 == 0
    flt = idx.makeFilter(mask)
    idx.addDenseBatch(X[n0:], ids[n0:])
    idx.finalize()
    assert idx.stats()["rows_appended"] == n1 - n0
    before = idx.knnQueryBatch(Q, EF)
    assert np.isin(before[0], ids[n0:]).any()                     # the walk does find new rows
    res = idx.knnQueryBatchFiltered(flt, Q, K)
    same_bits(res, host_filtered(before, ids[:n0][mask], K))
    flt.close()
    idx.close()


def test_slices_of_a_large_batch():
    """70 000 queries: both sides of the cut at 65 536, results and counters at their offsets"""
    n, nq_small, nq_big, ef = 200, 1024, 70000, 32
    X, Q = refio.s_lowrank(n, 8, 1106), refio.s_lowrank(nq_small, 8, 1107)
    ids = ext_ids(n)
    mask = np.random.default_rng(1108).random(n) < 0.5
    assert mask.sum() > ef                                        # (the walk route)
    idx = make_index("l2", "hnsw", X, ids, M=8, efConstruction=40, indexThreadQty=1)
    idx.setQueryTimeParams(efSearch=ef)
    before, bctr = run(idx, Q, ef)
    flt = idx.makeFilter(mask)
    src = np.arange(nq_big) % nq_small
    res, ctr = run(idx, np.ascontiguousarray(Q[src]), K, flt)
    assert idx.stats()["last_path"] == 4
    want = host_filtered(before, ids[mask], K)
    same_bits(res, tuple(w[src] for w in want))
    for nm, got, w in zip(("ndc", "hops", "hops_up"), ctr, bctr):
        assert got.shape == (nq_big,)
        np.testing.assert_array_equal(got, w[src], err_msg=nm)
    flt.close()
    idx.close()


@pytest.mark.parametrize("deleted", [False, True])
def test_inner_slices_of_the_walk_route(monkeypatch, deleted):
    """250 queries cut at 100 through NMSLIB_HNSW_SLICE_MAXQ (two slices and a tail of 50) answer as the uncut batch does:
    results, counts and the walk's counters at their offsets"""
    n, nq, ef = 1500, 250, 32
    X, Q = refio.s_lowrank(n, D, 1109), refio.s_lowrank(nq, D, 1110)
    ids = ext_ids(n)
    rng = np.random.default_rng(1111)
    mask = rng.random(n) < 0.5
    idx = make_index("l2", "hnsw", X, ids, M=8, efConstruction=40, indexThreadQty=1)
    idx.setQueryTimeParams(efSearch=ef)
    if deleted:
        dead = ids[rng.permutation(n)[:n // 5]]
        assert idx.deleteIds(dead) == len(dead)
    flt = idx.makeFilter(mask)
    assert flt.allowed > ef                                       # (the walk route)
    monkeypatch.delenv("NMSLIB_HNSW_SLICE_MAXQ", raising=False)
    want, wctr = run(idx, Q, K, flt)
    assert idx.stats()["last_path"] == 4
    monkeypatch.setenv("NMSLIB_HNSW_SLICE_MAXQ", "100")
    got, gctr = run(idx, Q, K, flt)
    assert idx.stats()["last_path"] == 4
    same_bits(got, want)
    for nm, g, w in zip(("ndc", "hops", "hops_up"), gctr, wctr):
        assert g.shape == (nq,)
        np.testing.assert_array_equal(g, w, err_msg=nm)
    flt.close()
    idx.close()


# ---- subset route -----------------------------------------------------------------------------------------------------
NS = 4200
MS = (0, 1, 7, 8, 9, 31, 32, 33, 64, 65, 1000, 4096)


def grid_rows(space, n, d, seed):
    rng = np.random.default_rng(seed)
    if space == "l2sqr_sift":
        return rng.integers(0, 256, (n, 128)).astype(np.uint8)
    r = 2000 if d == 1 else 8                                    # every sum below stays an integer under 2^24
    return rng.integers(-r, r + 1, (n, d)).astype(np.float32)


def exact_distances(space, X, Q):
    """[nq][n] in float64 of exact integers (cosinesimil / angulardist: the reference formula in float64)"""
    x, q = X.astype(np.float64), Q.astype(np.float64)
    diff = q[:, None, :] - x[None, :, :]
    if space in ("l2", "l2sqr_sift"):
        return (diff * diff).sum(-1)                             # (the optimized index answers squared l2)
    if space == "l1":
        return np.abs(diff).sum(-1)
    if space == "linf":
        return np.abs(diff).max(-1)
    dot = q @ x.T
    if space == "negdotprod":
        return -dot
    cos = np.clip(dot / (np.linalg.norm(q, axis=1)[:, None] * np.linalg.norm(x, axis=1)[None, :]), -1.0, 1.0)
    return 1.0 - cos if space == "cosinesimil" else np.arccos(cos)


def subset_oracle(dist, pos, ids, k):
    """dist [nq][n]; pos: the allowed live positions, ascending -> ids, dists, counts ordered by (distance, position)"""
    nq = dist.shape[0]
    oi = np.full((nq, k), -1, np.int32)
    od = np.full((nq, k), np.inf, np.float32)
    kk = min(k, len(pos))
    for q in range(nq):
        order = np.argsort(dist[q, pos], kind="stable")[:kk]
        oi[q, :kk], od[q, :kk] = ids[pos[order]], dist[q, pos[order]].astype(np.float32)
    return oi, od, np.full(nq, kk, np.int32)


def check_subset(space, got, want):
    if space in ("cosinesimil", "angulardist"):
        np.testing.assert_array_equal(got[2], want[2])
        valid = want[0] >= 0
        assert (got[0][~valid] == -1).all() and np.isposinf(got[1][~valid]).all()
        if space == "cosinesimil":
            eps, gk, wk = (lambda v: 1e-5 * v + 1e-6), got[1], want[1]
            assert close_rel(got[1][valid], want[1][valid])
        else:
            gk, wk = (np.cos(np.where(valid, x, 0).astype(np.float64)) for x in (got[1], want[1]))   # (padding: +inf)
            eps = lambda v: 4 * 2.0 ** -23                       # noqa: E731
            assert sim_close(gk[valid], wk[valid], ulps=4)
        for q in range(len(got[2])):                             # (rank by rank over the valid prefix)
            c = got[2][q]
            bad = ids_match_modulo_near_ties(got[0][q:q + 1, :c], want[0][q:q + 1, :c], wk[q:q + 1, :c], eps, gk[q:q + 1, :c])
            assert not bad, (q, bad)
    else:
        same_bits(got, want)


SUBSETS = [("l2", 1), ("l2", 8), ("l2", 127), ("l2", 128), ("l2", 300), ("l2sqr_sift", 128), ("l1", 8), ("linf", 8),
           ("negdotprod", 8), ("cosinesimil", 8), ("angulardist", 8)]


@pytest.mark.parametrize("space,d", SUBSETS)
def test_subset_route(space, d):
    X, Q = grid_rows(space, NS, d, 1110), grid_rows(space, 5, d, 1111)
    X[3000] = X[17]                                              # a planted tie: equal distances, order by position
    if space in ("cosinesimil", "angulardist"):
        X[(X == 0).all(1)] = 1                                   # (no zero-norm row)
    Q[0] = X[17]
    ids = ext_ids(NS)
    dist = exact_distances(space, X, Q)
    idx = make_index(space, "hnsw", X, ids, M=6, efConstruction=30, gpu_build=1)
    idx.setQueryTimeParams(efSearch=64)
    order = np.random.default_rng(1112).permutation(NS)
    order = np.r_[[17, 3000], order[~np.isin(order, [17, 3000])]]   # from m = 2 on the tie is inside
    for m in MS:
        pos = np.sort(order[:m])
        mask = np.zeros(NS, bool)
        mask[pos] = True
        flt = idx.makeFilter(mask, scan_rows=4096)
        assert flt.allowed == m
        for k in sorted({max(1, m // 2), max(1, m), m + 3}):      # k < m, k = m, k > m
            got, ctr = run(idx, Q, k, flt)
            assert idx.stats()["last_path"] == 7, (m, k)
            check_subset(space, got, subset_oracle(dist, pos, ids, k))
            assert (ctr[0] == m).all() and (ctr[1] == 0).all() and (ctr[2] == 0).all()
            if m >= 2 and k >= 2 and space != "negdotprod" and d > 1:
                np.testing.assert_array_equal(got[0][0, :2], ids[[17, 3000]])
        flt.close()
    # a tombstone inside the list: the rows are evaluated and left out; the list, and so ndc, stay what they were
    pos = np.sort(order[:65])
    mask = np.zeros(NS, bool)
    mask[pos] = True
    flt = idx.makeFilter(mask, scan_rows=4096)
    dead = pos[[0, 33, 64]]
    assert idx.deleteIds(ids[dead]) == 3
    got, ctr = run(idx, Q, 10, flt)
    check_subset(space, got, subset_oracle(dist, np.setdiff1d(pos, dead), ids, 10))
    assert idx.stats()["last_path"] == 7 and (ctr[0] == 65).all() and flt.allowed == 62
    got, _ = run(idx, Q, 70, flt)
    assert (got[2] == 62).all()
    flt.close()
    # a filter made now lists the live rows only
    flt = idx.makeFilter(mask, scan_rows=4096)
    got, ctr = run(idx, Q, 10, flt)
    check_subset(space, got, subset_oracle(dist, np.setdiff1d(pos, dead), ids, 10))
    assert (ctr[0] == 62).all() and flt.allowed == 62
    flt.close()
    idx.close()


def test_the_routing_rule_on_the_device():
    """scan_rows = 0: m = k' is scanned, m = k' + 1 walked; m = 4097 is walked whatever scan_rows says"""
    X, Q = grid_rows("l2", NS, 8, 1113), grid_rows("l2", 5, 8, 1114)
    ids = ext_ids(NS)
    dist = exact_distances("l2", X, Q)
    idx = make_index("l2", "hnsw", X, ids, M=6, efConstruction=30, gpu_build=1)
    idx.setQueryTimeParams(efSearch=64)
    before = idx.knnQueryBatch(Q, 64)
    order = np.random.default_rng(1115).permutation(NS)
    for m, scan_rows, path in ((64, 0, 7), (65, 0, 4), (65, 65, 7), (66, 65, 4), (4096, 4096, 7), (4097, 4096, 4)):
        pos = np.sort(order[:m])
        mask = np.zeros(NS, bool)
        mask[pos] = True
        flt = idx.makeFilter(mask, scan_rows=scan_rows)
        got = idx.knnQueryBatchFiltered(flt, Q, 10)
        assert idx.stats()["last_path"] == path, (m, scan_rows)
        if path == 7:
            same_bits(got, subset_oracle(dist, pos, ids, 10))
        else:
            same_bits(got, host_filtered(before, ids[pos], 10))
        flt.close()
    # k above efSearch moves k' with it: m = 100 at k = 100 is scanned, at k = 10 walked
    pos = np.sort(order[:100])
    mask = np.zeros(NS, bool)
    mask[pos] = True
    flt = idx.makeFilter(mask)
    same_bits(idx.knnQueryBatchFiltered(flt, Q, 100), subset_oracle(dist, pos, ids, 100))
    assert idx.stats()["last_path"] == 7
    idx.knnQueryBatchFiltered(flt, Q, 10)
    assert idx.stats()["last_path"] == 4
    flt.close()
    idx.close()


def test_subset_route_under_gpu_rows_f16_reads_the_f32_rows():
    """column 0 holds odd integers above 2048, which fp16 does not hold: the f32 rows give exact distances, the copy cannot"""
    X, Q = grid_rows("l2", NS, 8, 1116), grid_rows("l2", 5, 8, 1117)
    X[:, 0] = 3001 + 2 * np.random.default_rng(1118).integers(0, 50, NS)
    Q[:, 0] = 3050
    ids = ext_ids(NS)
    dist = exact_distances("l2", X, Q)
    idx = make_index("l2", "hnsw", X, ids, M=6, efConstruction=30, gpu_build=1, gpu_rows="f16")
    idx.setQueryTimeParams(efSearch=64)
    pos = np.sort(np.random.default_rng(1119).permutation(NS)[:50])
    mask = np.zeros(NS, bool)
    mask[pos] = True
    flt = idx.makeFilter(mask)
    got = idx.knnQueryBatchFiltered(flt, Q, 10)
    assert idx.stats()["last_path"] == 7
    same_bits(got, subset_oracle(dist, pos, ids, 10))
    flt.close()
    idx.close()


def test_subset_route_with_more_than_64_kb_of_lds():
    """l2, 12 000 dimensions (a 48 KB query) beside 4096 keys (m = 2049): 82 KB of LDS, integer sums below 2^24"""
    n, d, m = 2100, 12000, 2049
    X, Q = grid_rows("l2", n, d, 1120), grid_rows("l2", 3, d, 1121)
    ids = ext_ids(n)
    dist = np.stack([((X - q) ** 2).sum(1, dtype=np.float64) for q in Q])
    idx = make_index("l2", "hnsw", X, ids, M=4, efConstruction=10, indexThreadQty=1)
    idx.setQueryTimeParams(efSearch=64)
    pos = np.sort(np.random.default_rng(1122).permutation(n)[:m])
    mask = np.zeros(n, bool)
    mask[pos] = True
    flt = idx.makeFilter(mask, scan_rows=4096)
    got, ctr = run(idx, Q, 10, flt)
    assert idx.stats()["last_path"] == 7 and (ctr[0] == m).all()
    same_bits(got, subset_oracle(dist, pos, ids, 10))
    flt.close()
    idx.close()


def test_poisoned_workspaces_give_the_same_bits(tmp_path):
    assert "NMSLIB_GPU_POISON" not in os.environ, "this process must run without the poison fill"
    want = filter_poison_child.run_all()
    out = tmp_path / "poison.npz"
    env = dict(os.environ, NMSLIB_GPU_POISON="255")
    # (one attempt: a non-zero exit, a death by signal or the time limit fails the test)
    r = subprocess.run([sys.executable, filter_poison_child.__file__, str(out)], env=env, timeout=120,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, f"child exit {r.returncode}\n{r.stdout[-4000:]}"
    with np.load(out) as z:
        got = {name: z[name] for name in z.files}
    assert sorted(got) == sorted(want)
    differ = [name for name in sorted(want) if not np.array_equal(got[name], want[name])]
    assert not differ, differ
