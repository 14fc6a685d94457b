"""What the tests of the batch with one filter per query share (nmslib_gpu_knn_query_batch_filtered_each).

The yardstick is code that exists without the feature: per filter group, the single-filter entry over that group's queries
in the caller's order (knnQueryBatchFiltered; knnQueryBatch for the -1 group), its counters and its last_path."""
import numpy as np

from tests.gpuutil import same_bits

COUNTERS = ("ndc", "hops", "hops_up")


def each(idx, filters, fq, Q, k):
    """the new entry -> (ids, dists, counts), (ndc, hops, hops_up) or None, routes"""
    ids, ds, cnt, routes = idx.knnQueryBatchEachFiltered(filters, fq, Q, k, return_routes=True)
    assert idx.stats()["last_path"] == 9
    ctr = idx.read_counters(len(Q))
    return (ids, ds, cnt), None if ctr is None else tuple(x.copy() for x in ctr), routes


def per_group(idx, filters, fq, Q, k):
    """one single-filter call per group -> the same three, assembled in the caller's order"""
    fq = np.asarray(fq, np.int32)
    nq = len(Q)
    ids = np.full((nq, k), -2, np.int32)
    ds = np.full((nq, k), np.nan, np.float32)
    cnt = np.full(nq, -2, np.int32)
    ctr = tuple(np.full(nq, -2, np.int32) for _ in COUNTERS)
    routes = np.full(nq, -2, np.int32)
    have_ctr = True
    for g in np.unique(fq):
        sel = np.nonzero(fq == g)[0]
        Qg = np.ascontiguousarray(Q[sel])
        res = idx.knnQueryBatch(Qg, k) if g < 0 else idx.knnQueryBatchFiltered(filters[g], Qg, k)
        ids[sel], ds[sel], cnt[sel] = res
        routes[sel] = idx.stats()["last_path"]
        c = idx.read_counters(len(sel))
        if c is None:
            have_ctr = False
        else:
            for dst, src in zip(ctr, c):
                dst[sel] = src
    return (ids, ds, cnt), ctr if have_ctr else None, routes


def same_batch(got, want):
    """results, counters and routes of two runs of each / per_group"""
    same_bits(got[0], want[0])
    assert (got[1] is None) == (want[1] is None)
    if got[1] is not None:
        for nm, g, w in zip(COUNTERS, got[1], want[1]):
            np.testing.assert_array_equal(g, w, err_msg=nm)
    np.testing.assert_array_equal(got[2], want[2], err_msg="routes")


def take(answer, sel):
    """the rows `sel` of an answer of each / per_group"""
    res, ctr, routes = answer
    return tuple(x[sel] for x in res), None if ctr is None else tuple(x[sel] for x in ctr), routes[sel]


def plan_order(fq, routes):
    """the stable permutation into plan order: unfiltered, walk-route filters, subset-route filters (route 7), by filter
    index within each"""
    fq = np.asarray(fq)
    seg = np.where(fq < 0, 0, np.where(routes == 7, 2, 1))
    return np.argsort(seg * (fq.max() + 2) + fq + 1, kind="stable")
