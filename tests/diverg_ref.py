"""Expected distances of the divergence spaces in float64, and the error bound the GPU tests hold them to.

d(obj1, obj2) per space as the reference defines it (src/distcomp_bregman.cc, src/distcomp_js.cc, the *rq classes of
src/space/space_bregman.cc exchange the arguments), evaluated in float64 from the float32 inputs, with the reference's
rules for zeros: the Bregman spaces take log x = -1e5 for x <= 0 (include/distcomp.h:149-154), Jensen-Shannon takes
x log x = 0 below FLT_MIN (JSStandard).

The bound.  S(obj1, obj2) is the sum of the absolute values of every product and addend of the formula; a float32
evaluation in any order lies within (D + 8) * 2^-24 * S of the exact value: recursive summation at unit roundoff 2^-24,
with room for a few ulp in each logarithm and quotient.  jsmetr* are compared through their squares."""
import numpy as np

SPACES = ["kldivfast", "kldivfastrq", "kldivgenfast", "kldivgenfastrq", "kldivgenslow", "itakurasaitofast",
          "jsdivslow", "jsdivfast", "jsmetrslow", "jsmetrfast"]
FLT_MIN = float(np.finfo(np.float32).tiny)


def is_metr(space):
    return space.startswith("jsmetr")


def _breg_log(x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x > 0, np.log(np.where(x > 0, x, 1.0)), -1e5)


def _js_xlogx(x):
    return np.where(x < FLT_MIN, 0.0, x * np.log(np.where(x < FLT_MIN, 1.0, x)))


def formula(space, a, b):
    """-> (d, S) of formula(obj1 = a, obj2 = b) over the last axis; jsmetr*: d is the SQUARE of the distance."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    if space.endswith("rq"):
        a, b = b, a
    D = a.shape[-1]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if space.startswith("kldiv"):
            la, lb = _breg_log(a), _breg_log(b)
            d = (a * (la - lb)).sum(-1)
            S = (np.abs(a * la) + np.abs(a * lb)).sum(-1)
            if space.startswith("kldivgen"):
                d = d + (b - a).sum(-1)
                S = S + (np.abs(a) + np.abs(b)).sum(-1)
            return d, S
        if space == "itakurasaitofast":
            la, lb = _breg_log(a), _breg_log(b)
            d = (a / b - (la - lb)).sum(-1) - D
            return d, (np.abs(a / b) + np.abs(la) + np.abs(lb) + 1).sum(-1)
        m = 0.5 * (a + b)
        ta, tb, tm = _js_xlogx(a), _js_xlogx(b), _js_xlogx(m)
        d = np.maximum(0.5 * (ta + tb).sum(-1) - tm.sum(-1), 0.0)
        return d, (0.5 * np.abs(ta) + 0.5 * np.abs(tb) + np.abs(tm)).sum(-1)


def bound(S, D):
    return (D + 8) * 2.0 ** -24 * S


def scan(space, rows, query):
    """d(row, query) for every row (a scan's obj1 is the row, seqsearch.cc:143-150) -> (d [n], bound [n])"""
    d, S = formula(space, rows, np.asarray(query)[None, :])
    return d, bound(S, rows.shape[1])


def pair(space, a, b):
    d, S = formula(space, a, b)
    return d, bound(S, len(a))


def comparable(space, dist):
    """a float32 distance as the quantity `formula` returns (jsmetr*: its square)"""
    dist = np.asarray(dist, np.float64)
    return dist * dist if is_metr(space) else dist


def within(space, got, want_d, bnd):
    return np.abs(comparable(space, got) - want_d) <= bnd


def seq_search(space, rows, queries, k):
    """stable (distance, position) order of the helper's own distances -> positions [nq, k], d [nq, k], bound [nq, k]"""
    pos, dd, bb = [], [], []
    for q in queries:
        d, b = scan(space, rows, q)
        o = np.argsort(d, kind="stable")[:k]
        pos.append(o)
        dd.append(d[o])
        bb.append(b[o])
    return np.array(pos), np.array(dd), np.array(bb)


def near_tie_mask(d, b):
    """[nq, k] -> positions whose distance lies within the two bounds of a neighbour's in the list"""
    close = np.diff(d, axis=1) <= b[:, 1:] + b[:, :-1]
    m = np.zeros(d.shape, bool)
    m[:, 1:] |= close
    m[:, :-1] |= close
    return m


def bigk_inputs():
    """n = 6000, D = 4: one histogram at scales spread evenly over seven decades above the queries' (each row with its
    own 0.1 % perturbation), so that the sorted distances keep apart: relative gaps of about 3e-3 against a bound of
    about 1e-6.  (Random histograms of one scale crowd: 6000 distances within one S leave 4 % of them closer than
    the bound.)"""
    rng = np.random.default_rng(61)
    scale = np.exp(np.linspace(np.log(10.0), np.log(1e8), 6000))[rng.permutation(6000), None]
    h0 = np.array([0.1, 0.2, 0.3, 0.4])
    rows = (scale * h0 * (1 + 0.001 * rng.uniform(-1, 1, size=(6000, 4)))).astype(np.float32)
    qs = rng.uniform(0.2, 1.0, size=(3, 4)).astype(np.float32)
    return rows, qs
