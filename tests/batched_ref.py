"""Inputs and cases for the exact check of the batched GPU HNSW builder against its sequential restatement
(orc.HnswGraph.build_batched).  Test infrastructure only; nothing here needs a GPU.

The wave-parallel kernels and the C loop sum in different orders, so every input is one on which f32 arithmetic is exact
whatever the order: the graphs must then be equal entry by entry, ties included.

  dyadic      coordinates k/256 in [-1, 1), D = 16 or 32: differences are multiples of 2^-8 below 2, their squares multiples
              of 2^-16 below 4, and a sum of 32 of them needs 7 + 16 = 23 bits <= 24.  Products are multiples of 2^-16 below
              1, a sum of 32 needs 5 + 16 bits.  l1 / linf: multiples of 2^-8.
  unit rows   16 of 32 coordinates +-1/4: the squared norm is exactly 1 (normalising multiplies by 1.0), dots are
              multiples of 1/16 -- 33 possible distances, so nearly every comparison is a tie
  bytes       l2sqr_sift rows with values 0..7, D = 128: integer distances below 6273, heavy ties
"""
import numpy as np

from . import orc

ROWS = (300, 600, 1000, 1500, 2500)      # a case uses the smallest of these at which the restatement shows its witness


def dyadic(n, d, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(-256, 256, (n, d)) / 256.0).astype(np.float32)


def unit_rows(n, seed):
    rng = np.random.default_rng(seed)
    X = np.zeros((n, 32), np.float32)
    for i in range(n):
        X[i, rng.permutation(32)[:16]] = rng.choice(np.float32([-0.25, 0.25]), 16)
    return X


def small_bytes(n, seed):
    return np.random.default_rng(seed).integers(0, 8, (n, 128)).astype(np.uint8)


def clustered(n, d, seed, cluster=300):
    """n - cluster iid dyadic rows, then `cluster` rows within +-2/256 of row 7 in every coordinate, contiguous"""
    X = dyadic(n - cluster, d, seed)
    rng = np.random.default_rng(seed + 1)
    c = X[7][None, :] + rng.integers(-2, 3, (cluster, d)) / 256.0
    c = np.clip(c, -1.0, 255.0 / 256.0).astype(np.float32)
    return np.concatenate([X, c])


def make_rows(kind, n, seed=11):
    if kind == "d16":
        return dyadic(n, 16, seed)
    if kind == "d32":
        return dyadic(n, 32, seed)
    if kind == "unit":
        return unit_rows(n, seed)
    if kind == "bytes":
        return small_bytes(n, seed)
    if kind == "cluster16":
        return clustered(n, 16, seed)
    raise ValueError(kind)


def check_exact_inputs(space, X):
    """the premise: f32 sums of this input equal the float64 ones in any order (checked on a sample of pairs, two orders)"""
    rng = np.random.default_rng(3)
    a, b = rng.integers(0, len(X), 256), rng.integers(0, len(X), 256)
    A, B = X[a].astype(np.float32), X[b].astype(np.float32)
    if space in ("l2", "l2sqr_sift"):
        terms = (A - B) ** 2
    elif space in ("l1", "linf"):
        terms = np.abs(A - B)
    else:
        terms = A * B
    if space == "cosinesimil":
        assert (np.float32(1) == (X.astype(np.float32) ** 2).sum(1, dtype=np.float32)).all()
    exact = terms.astype(np.float64).sum(1)
    fwd = np.zeros(len(a), np.float32)
    for j in range(terms.shape[1]):
        fwd = (fwd + terms[:, j]).astype(np.float32)
    rev = np.zeros(len(a), np.float32)
    for j in reversed(range(terms.shape[1])):
        rev = (rev + terms[:, j]).astype(np.float32)
    pair = terms.reshape(len(a), -1, 8).sum(2, dtype=np.float32).sum(1, dtype=np.float32)
    for s in (fwd, rev, pair):
        assert (s.astype(np.float64) == exact).all()


def restate(space, X, **p):
    """the restatement of make_index(space, "hnsw", X, gpu_build=1, **p): the engine's parameter names and defaults"""
    M = p.get("M", 16)
    return orc.HnswGraph.build_batched(
        space, X, M=M, efConstruction=p.get("efConstruction", 200), maxM=p.get("maxM", M), maxM0=p.get("maxM0", 2 * M),
        delaunay_type=p.get("delaunay_type", 2), post=p.get("post", 0), batch_div=p.get("gpu_build_div", 0),
        max_batch=p.get("gpu_build_batch", 0), cut=p.get("gpu_build_cut", 0))


def resume(space, X, graph, first, levels, **p):
    """the restatement of an append (gpu_append=1): `graph` (the keys of refio.parse_index / HnswGraph.arrays)
    is a finished graph over X[:first], `levels` are those of the rows X[first:]; the batch loop is entered at `first`.
    The engine's parameter names and defaults, as restate has them.  -> the orc.HnswGraph over all of X"""
    n, M = len(X), p.get("M", 16)
    maxM, maxM0 = int(graph["maxM"]), int(graph["maxM0"])
    assert graph["n"] == first and len(levels) == n - first and p.get("post", 0) == 0
    assert (maxM, maxM0) == (p.get("maxM", M), p.get("maxM0", 2 * M))
    levels = np.asarray(levels, np.int32)
    up_off = np.concatenate([graph["up_off"], np.full(n - first, -1, np.int64)])
    cur = len(graph["up_links"])
    for i in np.nonzero(levels > 0)[0]:
        up_off[first + i] = cur
        cur += int(levels[i]) * (maxM + 1)
    up_links = np.concatenate([graph["up_links"], np.zeros(cur - len(graph["up_links"]), np.int32)])
    links0 = np.concatenate([graph["links0"], np.zeros((n - first, maxM0 + 1), np.int32)])
    g = orc.HnswGraph.from_arrays(space, X, maxM, maxM0, int(graph["maxlevel"]), int(graph["enterpoint"]),
                                  np.concatenate([graph["levels"], levels]), links0, up_off, up_links)
    return g.insert_batched(first, M=M, efConstruction=p.get("efConstruction", 200), delaunay_type=p.get("delaunay_type", 2),
                            batch_div=p.get("gpu_build_div", 0), max_batch=p.get("gpu_build_batch", 0),
                            cut=p.get("gpu_build_cut", 0))


# name -> (space, rows, n, index parameters, witness: counter -> lower bound the restatement must reach)
CASES = {
    "core-narrow": ("l2", "d16", 300, dict(M=6, efConstruction=100),
                    dict(cand_lists_gt64=1, shrinks=1, targets_ge2_requests=1)),
    "short-efc3": ("l2", "d16", 300, dict(M=6, efConstruction=3), dict(short_lists_kept=299)),
    "short-efc20": ("l2", "d16", 300, dict(M=6, efConstruction=20), dict(short_lists_kept=1)),
    "doubling-efc100": ("l2", "d16", 300, dict(M=6, efConstruction=100, gpu_build_div=1),
                        dict(mates_truncated=1, merged_cut=1)),
    "doubling-efc200": ("l2", "d16", 300, dict(M=6, efConstruction=200, gpu_build_div=1),
                        dict(mates_truncated=1, merged_cut=1)),
    "capped-cut": ("l2", "d16", 300, dict(M=6, efConstruction=100, gpu_build_div=4, gpu_build_batch=48, gpu_build_cut=250),
                   dict(batches_at_cap=1, batches_at_cut=1)),
    "clustered": ("l2", "cluster16", 1500, dict(M=8, efConstruction=100, gpu_build_div=4),
                  dict(most_requests_one_target=33)),
    # (beyond the cap's witness: in these two the 64th mate is selected -- a cap of 63 in the restatement changes the graph)
    "mates-cap-m100-d0": ("l2", "cluster16", 600, dict(M=100, maxM0=254, efConstruction=200, delaunay_type=0, gpu_build_div=1),
                          dict(mates_truncated=1, most_requests_one_target=127)),
    "mates-cap-m64-d1": ("l2", "cluster16", 600, dict(M=64, maxM0=254, efConstruction=100, delaunay_type=1, gpu_build_div=1),
                         dict(mates_truncated=1, most_requests_one_target=127)),
    "tall": ("l2", "d16", 300, dict(M=3, maxM0=6, efConstruction=100),
             dict(upper_slices_ge2=1, upper_mates=1, promotions_in_batch=1)),
    "l1": ("l1", "d16", 300, dict(M=6, efConstruction=64), dict(shrinks=1)),
    "linf": ("linf", "d16", 300, dict(M=6, efConstruction=64), dict(shrinks=1)),
    "negdotprod": ("negdotprod", "d16", 300, dict(M=6, efConstruction=64), dict(shrinks=1)),
    "cosinesimil": ("cosinesimil", "unit", 300, dict(M=6, efConstruction=64), dict(ties_merge=1, ties_link=1)),
    "l2sqr_sift": ("l2sqr_sift", "bytes", 300, dict(M=6, efConstruction=64, skip_optimized_index=1),
                   dict(ties_merge=1, ties_link=1)),
    "wide-m64-d0": ("l2", "d32", 300, dict(M=64, efConstruction=100, delaunay_type=0),
                    dict(longest_list_shrunk=127, targets_gt_nodes_before=1)),
    "wide-m100-d0": ("l2", "d32", 300, dict(M=100, maxM0=200, efConstruction=100, delaunay_type=0),
                     dict(longest_list_shrunk=127, targets_gt_nodes_before=1)),
    "wide-m64-d2": ("l2", "d32", 2500, dict(M=64, efConstruction=100, delaunay_type=2),
                    dict(longest_list_shrunk=127, targets_gt_nodes_before=1)),
    "heuristic1": ("l2", "d16", 300, dict(M=16, efConstruction=100, delaunay_type=1),
                   dict(h1_topups_select=1, h1_topups_shrink=1)),
}
for _post in (1, 2):
    for _d in (0, 1, 2):
        CASES[f"post{_post}-d{_d}"] = ("l2", "d16", 300, dict(M=6, efConstruction=100, post=_post, delaunay_type=_d),
                                       dict(second_pass_largest_batch=2, **({"post1_widened": 13} if _post == 1 else {})))


def case_rows(name):
    space, kind, n, params, witness = CASES[name]
    return space, make_rows(kind, n), dict(params), witness
