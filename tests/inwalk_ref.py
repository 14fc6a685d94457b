"""The in-walk filtered HNSW search (gpu_inwalk=1) as plain sequential Python over a parsed graph
(refio.parse_index) and the rows, with the cases the CPU and the GPU tests share.  Test infrastructure only; nothing here
needs a GPU.

The rule, with cap = max(efSearch, k), eligible(p) = allowed (and below the filter's length) and not deleted, and every
order by the pair (distance, position):

  upper levels  greedy descent: every node a stepping stone, a move only on a strictly smaller distance, among equal
                minima the first in list order.  ndc counts the entry point and every list entry, hops_up every list.
  level 0       W: the cap smallest eligible nodes found; C: the CAPC = 1024 smallest admitted nodes not yet expanded.
                The descent's node is visited, enters C, and W if eligible.  While C is not empty: pop its smallest c;
                full = |W| == cap; bound = W's largest distance if full; stop if full and d(c) > bound; hops += 1; U = the
                unvisited neighbours of c in list order, now visited; ndc += |U|; u is admitted when not full or
                d(u) < bound (full, bound as taken before the expansion); the admitted enter C, the admitted and eligible
                enter W, each keeping its smallest.  What falls off C stays visited.
  result        the first min(k, |W|) entries of W.

The inputs are the exact-arithmetic ones of tests/batched_ref.py, so the wave's reduction order and numpy's cannot differ
and distances are compared bit for bit; the heavy ties of the unit rows and the bytes stay in.
"""
import functools

import numpy as np

from . import batched_ref as br
from . import refio

CAPC = 1024
WITNESS = ("dropped_from_c", "largest_c", "pops_at_bound", "expansions_when_full", "ties_admitted")


def ext_ids(n):
    """external ids that are no positions (a result that carries positions shows)"""
    return (5 * np.arange(n) + 7).astype(np.int32)


def distance_fn(space, X, q):
    """positions -> the f32 distances the search kernels give on these (exact) inputs.  l2 is the optimized index's squared
    distance, cosinesimil its 1 - dot over unit rows and a unit query; negdotprod gives -0.0 for a zero product, as the
    device does."""
    x, qq = X.astype(np.float64), q.astype(np.float64)

    def f(pos):
        rows = x[np.asarray(pos, np.int64)]
        if space in ("l2", "l2sqr_sift"):
            d = ((rows - qq) ** 2).sum(1)
        elif space == "l1":
            d = np.abs(rows - qq).sum(1)
        elif space == "linf":
            d = np.abs(rows - qq).max(1)
        elif space == "negdotprod":
            d = -(rows @ qq)
        elif space == "cosinesimil":
            d = np.maximum(0.0, 1.0 - np.clip(rows @ qq, -1.0, 1.0))
        else:
            raise ValueError(space)
        return d.astype(np.float32)
    return f


def search_one(g, dist, k, ef, eligible):
    """one query -> positions [k] (-1 padded), distances [k] (+inf padded), count, ndc, hops, hops_up, witness counters"""
    cap = max(ef, k)
    wit = dict.fromkeys(WITNESS, 0)
    pos = np.full(k, -1, np.int32)
    ds = np.full(k, np.inf, np.float32)
    if g["n"] == 0:
        return pos, ds, 0, 0, 0, 0, wit
    cur = int(g["enterpoint"])
    curd = dist([cur])[0]
    ndc, hops, hops_up = 1, 0, 0
    for lvl in range(int(g["maxlevel"]), 0, -1):
        changed = True
        while changed:
            changed = False
            L = refio._list_of(g, cur, lvl)
            hops_up += 1
            if L[0] > 0:
                nb = L[1:1 + L[0]]
                d = dist(nb)
                ndc += int(L[0])
                j = int(np.argmin(d))                                # the first of equal minima
                if d[j] < curd:
                    cur, curd, changed = int(nb[j]), d[j], True
    visited = np.zeros(g["n"], bool)
    visited[cur] = True
    C = [(float(curd), cur)]
    W = [(float(curd), cur)] if eligible[cur] else []
    while C:
        c = C.pop(0)
        full = len(W) == cap
        bound = W[-1][0] if full else np.inf
        if full and c[0] > bound:
            break
        wit["pops_at_bound"] += int(full and c[0] == bound)
        wit["expansions_when_full"] += int(full)
        hops += 1
        L = g["links0"][c[1]]
        U = []
        for u in L[1:1 + L[0]].tolist():
            if not visited[u]:
                visited[u] = True
                U.append(u)
        ndc += len(U)
        if not U:
            continue
        adm = [(float(d), u) for d, u in zip(dist(U), U) if not full or d < bound]
        known = {x[0] for x in C}
        dd = [x[0] for x in adm]
        wit["ties_admitted"] += sum(1 for x in dd if dd.count(x) > 1 or x in known)
        C = sorted(C + adm)
        wit["dropped_from_c"] += max(0, len(C) - CAPC)
        del C[CAPC:]
        wit["largest_c"] = max(wit["largest_c"], len(C))
        W = sorted(W + [x for x in adm if eligible[x[1]]])[:cap]
    kk = min(k, len(W))
    pos[:kk] = [x[1] for x in W[:kk]]
    ds[:kk] = np.float32([x[0] for x in W[:kk]])
    return pos, ds, kk, ndc, hops, hops_up, wit


def search(space, X, Q, g, k, ef, eligible, ids=None):
    """the batch -> (ids [nq, k], distances [nq, k], counts [nq]), (ndc, hops, hops_up), witness counters (summed; largest_c:
    the largest).  eligible: bool over the graph's positions.  ids: external ids (None: positions)"""
    nq = len(Q)
    oi = np.full((nq, k), -1, np.int32)
    od = np.full((nq, k), np.inf, np.float32)
    cnt, ndc, hops, hops_up = (np.zeros(nq, np.int32) for _ in range(4))
    wit = dict.fromkeys(WITNESS, 0)
    for q in range(nq):
        p, d, cnt[q], ndc[q], hops[q], hops_up[q], w = search_one(g, distance_fn(space, X, Q[q]), k, ef, eligible)
        od[q] = d
        oi[q] = np.where(p >= 0, (ids if ids is not None else np.arange(g["n"]))[np.maximum(p, 0)], -1)
        for name in WITNESS:
            wit[name] = max(wit[name], w[name]) if name == "largest_c" else wit[name] + w[name]
    return (oi, od, cnt), (ndc, hops, hops_up), wit


# ---- the cases ---------------------------------------------------------------------------------------------------------
KINDS = {"l2": "d16", "l1": "d16", "linf": "d16", "negdotprod": "d16", "cosinesimil": "unit", "l2sqr_sift": "bytes",
         "angulardist": "d16"}
BUILD = dict(M=8, efConstruction=60)
EF, K, NQ = 32, 10, 70


def allow_mask(spec, X):
    """("share", s, seed): every row with probability 1 / s; ("near", row, m): the m rows nearest `row` (l2, then position);
    ("first", m): positions below m; None: no filter"""
    n = len(X)
    if spec is None:
        return None
    if spec[0] == "share":
        return np.random.default_rng(spec[2]).random(n) < 1.0 / spec[1]
    if spec[0] == "first":
        return np.arange(n) < spec[1]
    x = X.astype(np.float64)
    d = ((x - x[spec[1]]) ** 2).sum(1)
    mask = np.zeros(n, bool)
    mask[np.argsort(d, kind="stable")[:spec[2]]] = True
    return mask


def dead_positions(spec, n):
    """("all-but-share", s, seed): every row but one in s; None: no deleted row"""
    if spec is None:
        return np.zeros(0, np.int64)
    return np.nonzero(np.random.default_rng(spec[2]).random(n) >= 1.0 / spec[1])[0]


# name -> space, rows (batched_ref.ROWS: the smallest at which the restatement shows the witness on the host-built graph),
# index parameters, efSearch, k, filter, deleted rows, witness: counter -> lower bound (or "counts_k": every count is k)
CASES = {
    "filter-1in8": dict(space="l2", n=2500, allow=("share", 8, 21), witness=dict(counts_k=1, expansions_when_full=1)),
    "far-cluster": dict(space="l2", n=2500, nq=20, allow=("near", 7, 40), witness=dict(dropped_from_c=1, largest_c=CAPC)),
    "tombstones": dict(space="l2", n=2500, dead=("all-but-share", 8, 22), witness=dict(counts_k=1)),
    "tombstones-filter": dict(space="l2", n=2500, allow=("share", 2, 23), dead=("all-but-share", 4, 24),
                              witness=dict(counts_k=1)),
    "cosinesimil": dict(space="cosinesimil", n=1000, allow=("share", 8, 25), witness=dict(ties_admitted=1000, pops_at_bound=1)),
    "l2sqr_sift": dict(space="l2sqr_sift", n=1000, allow=("share", 8, 26), witness=dict(ties_admitted=100)),
    "l1": dict(space="l1", n=1000, allow=("share", 8, 27), witness=dict(counts_k=1)),
    "linf": dict(space="linf", n=1000, allow=("share", 8, 28), witness=dict(counts_k=1, ties_admitted=1)),
    "negdotprod": dict(space="negdotprod", n=1000, allow=("share", 8, 29), witness=dict(counts_k=1)),
    "wide-m64": dict(space="l2", n=600, build=dict(M=64, efConstruction=100, delaunay_type=0), allow=("share", 8, 30),
                     witness=dict(counts_k=1, longest_list=128)),
    "wide-m100": dict(space="l2", n=600, build=dict(M=100, efConstruction=100, delaunay_type=0), allow=("share", 8, 31),
                      witness=dict(counts_k=1, longest_list=200)),
    "k-above-ef": dict(space="l2", n=2500, k=40, allow=("share", 8, 32), witness=dict(counts_k=1)),
    "ef-k-1": dict(space="l2", n=1000, ef=1, k=1, allow=("share", 8, 33), witness=dict(counts_k=1)),
    # (tombstones: a filter of fewer rows than cap would take the subset route)
    "ef-1024-dry": dict(space="l2", n=1500, ef=1024, nq=8, dead=("all-but-share", 2, 34), witness=dict(graph_dry=1)),
}


def case(name):
    """-> space, X, Q, ids, index parameters, efSearch, k, allow mask or None, deleted positions, witness"""
    c = CASES[name]
    space, n = c["space"], c["n"]
    assert n in br.ROWS
    X = br.make_rows(KINDS[space], n)
    Q = br.make_rows(KINDS[space], c.get("nq", NQ), seed=12)
    br.check_exact_inputs(space, X)
    br.check_exact_inputs(space, np.concatenate([X[:64], Q]))
    return (space, X, Q, ext_ids(n), dict(c.get("build", BUILD)), c.get("ef", EF), c.get("k", K),
            allow_mask(c.get("allow"), X), dead_positions(c.get("dead"), n), dict(c["witness"]))


def eligible_of(n, allow, dead):
    e = np.ones(n, bool) if allow is None else np.r_[allow, np.zeros(n - len(allow), bool)]
    e = e.copy()
    e[dead] = False
    return e


def check_witness(name, g, want, wit, eligible, k, ef):
    """the restatement `want` (search's answer) and its counters `wit` show what the case is there for"""
    cnt = want[0][2]
    for counter, least in CASES[name]["witness"].items():
        if counter == "counts_k":
            assert (cnt == k).all(), (name, cnt)
        elif counter == "longest_list":
            assert g["links0"][:, 0].max() >= least, (name, int(g["links0"][:, 0].max()))
        elif counter == "graph_dry":
            # fewer eligible rows than cap: W never fills, the walk ends when C is empty and returns what it reached
            assert eligible.sum() < max(ef, k) and wit["expansions_when_full"] == 0 and (cnt == min(k, eligible.sum())).all()
        else:
            assert wit[counter] >= least, (name, counter, wit[counter], least)


@functools.lru_cache(maxsize=None)
def host_graph(name):
    """the host-built graph of a case (indexThreadQty=1: deterministic), built without a device (gpu_defer=1), saved and
    parsed -> the parsed graph"""
    import tempfile

    from .gpuutil import make_index
    space, X, Q, ids, build, ef, k, allow, dead, witness = case(name)
    idx = make_index(space, "hnsw", X, ids, indexThreadQty=1, gpu_defer=1, **build)
    with tempfile.TemporaryDirectory() as tmp:
        idx.save(tmp + "/g.idx", save_data=False)
        g = refio.parse_index(tmp + "/g.idx")
    idx.close()
    return g


@functools.lru_cache(maxsize=None)
def restated(name):
    """the restatement of a case on its host-built graph, computed once (never modified) -> search's answer"""
    space, X, Q, ids, build, ef, k, allow, dead, witness = case(name)
    return search(space, X, Q, host_graph(name), k, ef, eligible_of(len(X), allow, dead), ids)
