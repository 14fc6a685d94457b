"""-m gpu: the exact scan (seq_search) through the seeded append / delete / consolidate scripts of tests/lifecycle_ref.py,
compared after every step with the CPU oracle's scan (orc.seq_search) over the model's live rows in position order --
the existing tests of these paths (tests/test_gpu_scan_delete.py) compare with a second GPU index.

After every step: k-NN, rangeQueryFill at two radii and rangeQueryBatch with those radii per query.  ids map through the
model.  l2 and l1 run on integer grid rows and l2sqr_sift on bytes: ids and the distances' bits must be the oracle's, and
the radii are distances that occur, so the inclusive edge and its ties are part of what is compared.  cosinesimil runs on
dyadic rows of any norm: distances within gpuutil.close_rel of the oracle's, ids equal outside runs of such near-ties, and
radii halfway inside the first gap that is wider than that bound.  A state without live rows is not searched (no test of
the suite says what the scan answers there); its counts are asserted."""
import numpy as np
import pytest

from tests import batched_ref as br
from tests import lifecycle_ref as lr
from tests import orc
from tests.gpuutil import close_rel, ids_match_modulo_near_ties, make_index, same_bits

pytestmark = pytest.mark.gpu

K, NQ, CAP = 10, 32, 64
RANKS = (3, 25)                           # the radii: the distances of these ranks (1-based) in the oracle's scan


def rows_of(space, n, seed):
    if space == "l2sqr_sift":
        return br.small_bytes(n, seed)
    if space == "cosinesimil":
        return br.dyadic(n, 16, seed)
    return np.random.default_rng(seed).integers(-8, 9, (n, 16)).astype(np.float32)


def eps(v):
    return 1e-5 * v + 1e-6                # close_rel's bound


def radii_from(space, dist, rank):
    """per query: the distance at `rank` itself where distances are exact; else the middle of the first gap at or behind
    it that is wider than twice the bound"""
    if space != "cosinesimil":
        return dist[:, rank - 1].astype(np.float64)
    out = np.zeros(len(dist))
    for q, d in enumerate(dist.astype(np.float64)):
        r = rank
        while d[r] - d[r - 1] <= 4 * eps(d[r]) and r + 1 < len(d):
            r += 1
        out[q] = (d[r] + d[r - 1]) / 2
    return out


def check_state(idx, m, space, Q, what):
    live, ids = m.live_rows()
    assert idx.dataQty() == m.n and idx.deletedRows() == (0 if m.n == 0 else int(m.dead.sum())), what
    if len(ids) == 0:
        return
    n = len(live)
    pos, dist, cnt = orc.seq_search(space, live, Q, n)           # every row, ascending by (distance, position)
    assert (cnt == n).all()
    exact = space != "cosinesimil"
    k = min(K, n)
    got = idx.knnQueryBatch(Q, K)
    want = (np.full((NQ, K), -1, np.int32), np.full((NQ, K), np.inf, np.float32), np.full(NQ, k, np.int32))
    want[0][:, :k], want[1][:, :k] = ids[pos[:, :k]], dist[:, :k]
    if exact:
        same_bits(got, want)
    else:
        np.testing.assert_array_equal(got[2], want[2], err_msg=what)
        assert close_rel(got[1][:, :k], want[1][:, :k]), what
        assert not ids_match_modulo_near_ties(got[0][:, :k], want[0][:, :k], want[1][:, :k], eps, got[1][:, :k]), what
    for rank in RANKS:
        if rank >= n:
            continue
        radii = radii_from(space, dist, rank)
        inside = [np.sort(pos[q, dist[q].astype(np.float64) <= radii[q]]) for q in range(NQ)]     # position order
        bids, bds, bcnt, btot = idx.rangeQueryBatch(Q, radii, CAP)
        for q in range(NQ):
            w = inside[q]
            assert btot[q] == len(w) and bcnt[q] == min(len(w), CAP), (what, rank, q)
            c = bcnt[q]
            np.testing.assert_array_equal(bids[q, :c], ids[w[:c]], err_msg=f"{what} rank {rank} query {q}")
            wd = np.array([dist[q, np.nonzero(pos[q] == p)[0][0]] for p in w[:c]], np.float32)
            if exact:
                np.testing.assert_array_equal(bds[q, :c].view(np.uint32), wd.view(np.uint32))
            else:
                assert close_rel(bds[q, :c], wd), (what, rank, q)
            assert (bids[q, c:] == -1).all() and np.isposinf(bds[q, c:]).all()
            if q % 8 == 0:                                       # the single-query entry: the same bits as the batch's row
                fids, fds = idx.rangeQueryFill(Q[q], radii[q], CAP)
                np.testing.assert_array_equal(fids, bids[q, :c])
                np.testing.assert_array_equal(fds.view(np.uint32), bds[q, :c].view(np.uint32))


@pytest.mark.parametrize("space", ["l2", "cosinesimil", "l1", "l2sqr_sift"])
@pytest.mark.parametrize("seed", lr.SEEDS)
def test_seeded_script_on_the_exact_scan(seed, space):
    X, Q = rows_of(space, lr.POOL, 21), rows_of(space, NQ, 22)
    m = lr.ScanModel(space)
    state = dict(idx=None, step=0)

    def apply(rec):
        state["step"] += 1
        what = f"step {state['step']} ({rec['op']})"
        if rec["op"] == "build":
            state["idx"] = make_index(space, "seq_search", rec["X"], rec["ids"])
        elif rec["op"] == "append":
            if X.dtype == np.uint8:
                state["idx"].addUInt8Batch(rec["X"], rec["ids"])
            else:
                state["idx"].addDenseBatch(rec["X"], rec["ids"])
        elif rec["op"] == "delete":
            assert state["idx"].deleteIds(rec["ids"]) == rec["ret"], what
        else:
            assert state["idx"].consolidate() == rec["ret"], what
        check_state(state["idx"], m, space, Q, what)

    try:
        records = lr.run_script(m, X, lr.random_script(seed), on_step=apply)
    finally:
        if state["idx"] is not None:
            state["idx"].close()
    assert sum(1 for r in records if r["op"] == "consolidate" and r["ret"][0] > 0) >= 1
