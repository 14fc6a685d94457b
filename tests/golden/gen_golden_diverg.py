#!/usr/bin/env python3
"""Divergence-space fixture from the REAL reference's distance functions (oracle/_ref/libnmslib_ref.so).

The reference's C ABI creates an index over these spaces but cannot fill it: create_object (nmslib_c.cpp:235-243) casts
the space to VectorSpaceSimpleStorage<float>, the Bregman and Jensen-Shannon spaces derive from VectorSpace<float>
(include/space/space_bregman.h, space_js.h), so nmslib_add_data_point* answers RUNTIME.  The fixture is therefore what
seq_search WOULD answer: the compiled reference's own distance functions (KLPrecompSIMD, KLGeneralPrecompSIMD,
KLGeneralStandard, ItakuraSaitoPrecompSIMD, JSStandard, JSPrecomp, called through ctypes on objects laid out by
CreateObjFromVect: values, then PrecompLogarithms with the C library's logf), scanned with the row as obj1
(seqsearch.cc:143-150), sorted by (distance, position), range-filtered by rangequery.cc:67-82 and reported as
nmslib_c.cpp:1104-1113 does.

    make -C oracle ref && python3 tests/golden/gen_golden_diverg.py

For every space of diverg_ref.SPACES:
  * "main" set: n = 2500 rows (three row splits), D = 19 (a 16-block, a 4-block short by one, a 3-element tail),
    positive entries normalised to sum 1; five rows and two of the 33 queries carry exact zeros, except under
    itakurasaitofast and kldivgenslow, where a zero makes the reference itself return inf / NaN (x / 0, 0 * log 0).
    k = 10 and k = 100 (ids, distances, counts), range queries at two radii with capacities 4 and 1000, get_distance
    over fixed pairs including (p, p);
  * "dims" sets: n = 300, D in {1, 3, 4, 16, 128, 1000}, 9 queries, k = 10 (positive entries, not normalised: at D = 1
    a normalised row is the constant 1);
  * "dups" set: n = 200 of which 50 rows are exact copies of other rows, k = n: ties are bit-equal;
  * "tiny" set (7 rows): k = 10 > n; the object of row 0 as nmslib_get_data_point returns it.
Only the reference's outputs are stored; the inputs are regenerated from their seeds and pinned by SHA-256.

Tie order: (distance, position), NMSLIB's documented order and this library's.

Fair id comparison.  Ids are compared exactly, so no two of the reference distances a comparison reaches (the first
k + 1 of a main, dims or tiny query; all 200 of a dups query, copies of one row apart) may be closer than twice the
error bound of tests/diverg_ref.py.  Independent random rows cannot give that: 2500 distances within one S of each
other crowd whatever the seed.  The rows a query's list reaches are therefore laid on a segment from a centre next to
the query towards another point (`segments`): the distances grow along it with gaps hundreds of bounds wide, and the
remaining rows lie farther out.  What is left to chance (rows with zeros, the queries with zeros, whose distances are
led by the 1e5 of PrecompLogarithms over all rows, free rows at small D) is settled by re-seeding: `--search` counts
seeds up until the condition holds for every space on the float64 helper's distances with a tenth to spare, the seeds
it prints are recorded below, and main() asserts the condition on the reference's own distances.
"""
import ctypes as C
import functools
import hashlib
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import diverg_ref, orc  # noqa: E402

SPACES = diverg_ref.SPACES
NO_ZEROS = ("itakurasaitofast", "kldivgenslow")
RANGE_CAPS = (4, 1000)
DIMS = (1, 3, 4, 16, 128, 1000)
# the seeds `--search` found: the first, counting up from the base, at which the gap condition holds for every space
MAIN_SEED, DUPS_SEED, TINY_SEED = 20261352, 99, 5
DIMS_SEEDS = {1: 5144, 3: 4248, 4: 4246, 16: 4258, 128: 4370, 1000: 5243}
MAIN_N, MAIN_D, MAIN_NQ, MAIN_RAYS = 2500, 19, 33, 16
GOLDEN = os.path.join(HERE, "golden_diverg.npz")


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, np.float32).tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def histograms(rng, n, D):
    """positive rows that sum to 1, from flat to peaked"""
    t = np.exp(rng.uniform(np.log(0.05), np.log(3.0), size=(n, 1)))
    x = np.exp(t * rng.standard_normal((n, D)))
    return (x / x.sum(1, keepdims=True)).astype(np.float32)


def with_zeros(x, rng, count):
    x = x.copy()
    for r in range(len(x)):
        x[r, rng.choice(x.shape[1], size=count, replace=False)] = 0.0
    return x


def segments(rng, J, per, D, t0, dt, centre, end):
    """J centres c and, for each, `per` rows (1 - t) c + t u on the segment towards another point u, t = t0, t0 + dt,
    ...: every divergence of the family is convex along the segment, so from a query next to c the distances to the
    rows of its segment grow with t and keep gaps of about t dt sum((u - c)^2 / c), far above the rounding bound.
    -> (c [J, D], rows [J * per, D]) in float64"""
    c, u = centre(rng, J, D), end(rng, J, D)
    t = (t0 + dt * np.arange(per))[None, :, None]
    return c, ((1 - t) * c[:, None, :] + t * u[:, None, :]).reshape(J * per, D)


def _peaked(lo, hi):
    """histograms exp(t N(0, 1)) normalised, t uniform in [lo, hi] per row"""
    def draw(rng, n, D):
        x = np.exp(rng.uniform(lo, hi, size=(n, 1)) * rng.standard_normal((n, D)))
        return x / x.sum(1, keepdims=True)
    return draw


def _near(rng, c, rel, normalise):
    q = c * np.exp(rel * rng.standard_normal(c.shape))
    return (q / q.sum(1, keepdims=True) if normalise else q).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _main(seed):
    """sixteen segments of 110 rows from moderately peaked centres and 740 strongly peaked free histograms, which lie
    farther from every centre than its segment's first hundred rows, shuffled; query j lies next to centre j mod 16"""
    rng = np.random.default_rng(seed)
    c, seg = segments(rng, MAIN_RAYS, 110, MAIN_D, 0.05, 0.003, _peaked(1.0, 1.0), _peaked(2.0, 2.0))
    x = np.concatenate([seg, _peaked(1.5, 3.0)(rng, MAIN_N - len(seg), MAIN_D)]).astype(np.float32)
    x = x[rng.permutation(MAIN_N)]
    q = _near(rng, c[np.arange(MAIN_NQ) % MAIN_RAYS], 0.005, True)
    zr = np.array([3, 700, 1024, 1999, 2499])
    xz, qz = x.copy(), q.copy()
    xz[zr] = with_zeros(x[zr], rng, 3)
    qz[[5, 20]] = with_zeros(q[[5, 20]], rng, 2)
    return x, q, xz, qz


def main_rows(zeros, seed=None):
    return _main(MAIN_SEED if seed is None else seed)[2 if zeros else 0].copy()


def main_queries(zeros, seed=None):
    return _main(MAIN_SEED if seed is None else seed)[3 if zeros else 1].copy()


def main_pairs():
    rng = np.random.default_rng(20261017)
    return np.array([[0, 1], [5, 5], [3, 7], [7, 3], [700, 700], [12, 400], [2499, 0], [1024, 1999]]
                    + rng.integers(0, MAIN_N, size=(12, 2)).tolist(), np.int64)


def _uniform(lo, hi):
    return lambda rng, n, D: rng.uniform(lo, hi, size=(n, D))


@functools.lru_cache(maxsize=None)
def _dims(D, seed):
    """one segment of 40 rows and 260 free rows (positive entries, not normalised: at D = 1 a normalised row is the
    constant 1), shuffled; the queries lie next to the segment's centre"""
    rng = np.random.default_rng(seed)
    c, seg = segments(rng, 1, 40, D, 0.15, 0.02, _uniform(0.3, 0.7), _uniform(0.05, 1.0))
    x = np.concatenate([seg, rng.uniform(0.05, 1.0, size=(260, D))]).astype(np.float32)
    return x[rng.permutation(300)], _near(rng, np.repeat(c, 9, axis=0), 0.005, False)


def dims_rows(D, seed=None):
    return _dims(D, DIMS_SEEDS[D] if seed is None else seed)[0].copy()


def dims_queries(D, seed=None):
    return _dims(D, DIMS_SEEDS[D] if seed is None else seed)[1].copy()


def inputs_dups(seed=None):
    """150 distinct rows on one segment, so that no two of them are near-ties, and 50 exact copies"""
    rng = np.random.default_rng(DUPS_SEED if seed is None else seed)
    c, seg = segments(rng, 1, 150, 11, 0.05, 0.005, _peaked(1.0, 1.0), _peaked(2.0, 2.0))
    x = np.concatenate([seg, seg[rng.choice(150, size=50, replace=False)]]).astype(np.float32)
    return x[rng.permutation(200)], _near(rng, np.repeat(c, 6, axis=0), 0.005, True)


def inputs_tiny(seed=None):
    rng = np.random.default_rng(TINY_SEED if seed is None else seed)
    return histograms(rng, 7, 5), histograms(rng, 3, 5)


# ---- the reference's compiled distance functions over ctypes ----------------------------------------------------------
_FUNCS = {  # space -> (exported function of libnmslib_ref.so, objects carry logarithms, arguments exchanged, sqrt)
    "kldivfast": ("_ZN10similarity13KLPrecompSIMDIfEET_PKS1_S3_m", True, False, False),
    "kldivfastrq": ("_ZN10similarity13KLPrecompSIMDIfEET_PKS1_S3_m", True, True, False),
    "kldivgenfast": ("_ZN10similarity20KLGeneralPrecompSIMDIfEET_PKS1_S3_m", True, False, False),
    "kldivgenfastrq": ("_ZN10similarity20KLGeneralPrecompSIMDIfEET_PKS1_S3_m", True, True, False),
    "kldivgenslow": ("_ZN10similarity17KLGeneralStandardIfEET_PKS1_S3_m", False, False, False),
    "itakurasaitofast": ("_ZN10similarity23ItakuraSaitoPrecompSIMDIfEET_PKS1_S3_m", True, False, False),
    "jsdivslow": ("_ZN10similarity10JSStandardIfEET_PKS1_S3_m", False, False, False),
    "jsdivfast": ("_ZN10similarity9JSPrecompIfEET_PKS1_S3_m", True, False, False),
    "jsmetrslow": ("_ZN10similarity10JSStandardIfEET_PKS1_S3_m", False, False, True),
    "jsmetrfast": ("_ZN10similarity9JSPrecompIfEET_PKS1_S3_m", True, False, True),
}
_libm = C.CDLL("libm.so.6")
_libm.logf.restype = C.c_float
_libm.logf.argtypes = [C.c_float]


def precomp_logs(x):
    """PrecompLogarithms (include/distcomp.h:149-154) with the C library's logf, as the reference's build calls it"""
    flat = np.ascontiguousarray(x, np.float32).ravel()
    return np.array([_libm.logf(float(v)) if v > 0 else -1e5 for v in flat], np.float32).reshape(np.shape(x))


class RefIndex:
    """What the reference's seq_search answers over dense float rows of a divergence space, from the distance
    functions of the compiled reference (see the module docstring for why not through its C ABI)."""

    def __init__(self, L, space, rows):
        name, self.logs, self.swap, self.sqrt = _FUNCS[space]
        self.fn = getattr(L, name)
        self.fn.restype = C.c_float
        self.fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        self.rows = self.objects(rows)
        self.n, self.D = np.shape(rows)

    def objects(self, x):
        """CreateObjFromVect: the values, then (the "fast" spaces) their logarithms"""
        x = np.ascontiguousarray(x, np.float32)
        return np.ascontiguousarray(np.concatenate([x, precomp_logs(x)], axis=-1)) if self.logs else x

    def dist(self, o1, o2):
        """HiddenDistance(obj1, obj2)"""
        if self.swap:
            o1, o2 = o2, o1
        v = np.float32(self.fn(o1.ctypes.data, o2.ctypes.data, self.D))
        return np.sqrt(v) if self.sqrt else v

    def scan(self, qobj):
        """d(row, query) for every row (DistanceObjLeft, seqsearch.cc:143-150)"""
        return np.array([self.dist(self.rows[r], qobj) for r in range(self.n)], np.float32)

    def knn_all(self, queries):
        """distances to all rows in (distance, position) order"""
        qo = self.objects(queries)
        ids, ds = [], []
        for q in range(len(qo)):
            d = self.scan(qo[q])
            o = np.lexsort((np.arange(self.n), d))
            ids.append(o.astype(np.int32))
            ds.append(d[o])
        return np.array(ids), np.array(ds)

    def knn_canonical(self, queries, k):
        ids, ds = self.knn_all(queries)
        out_i = np.full((len(ids), k), -1, np.int32)
        out_d = np.full((len(ids), k), np.inf, np.float32)
        m = min(k, self.n)
        out_i[:, :m], out_d[:, :m] = ids[:, :m], ds[:, :m]
        return out_i, out_d, np.full(len(ids), m, np.int32)

    def range(self, query, radius, capacity):
        """rows with d(row, query) <= radius in insertion order, the first `capacity`, each reported with
        d(query, row) (rangequery.cc:67-82, nmslib_c.cpp:1092-1113)"""
        qo = self.objects(query)
        hit = np.nonzero(self.scan(qo) <= np.float32(radius))[0][:capacity]
        return hit.astype(np.int32), np.array([self.dist(qo, self.rows[r]) for r in hit], np.float32)

    def distance(self, a, b):
        return self.dist(self.rows[a], self.rows[b])

    def data_point(self, pos):
        return self.rows[pos].copy()

    def close(self):
        pass


def gaps_ok(space, rows, queries, ids, ds, upto, ties=False):
    """per query: every gap between consecutive REFERENCE distances among the first `upto` exceeds twice the bound
    (`ties`: or is exactly zero, between copies of one row)"""
    ok = np.ones(len(queries), bool)
    for q in range(len(queries)):
        pos = ids[q, :upto]
        _, bnd = diverg_ref.scan(space, rows[pos], queries[q])
        d = diverg_ref.comparable(space, ds[q, :upto])
        g = np.diff(d)
        far = g > 2 * np.maximum(bnd[1:], bnd[:-1])
        ok[q] = (far | ((g == 0) & (rows[pos[1:]] == rows[pos[:-1]]).all(1))).all() if ties else far.all()
    return ok


def helper_gaps_ok(spaces, rows, queries, upto, ties=False):
    """the same condition on the float64 helper's own sorted distances, with 10 % to spare: what `--search` tries
    seeds with (the reference's distances lie well within one bound of the helper's, and main() asserts on them)"""
    for s in spaces:
        for q in queries:
            d, b = diverg_ref.scan(s, rows, q)
            if not np.isfinite(d).all():
                return False
            o = np.argsort(d, kind="stable")[:upto]
            g, bb = np.diff(d[o]), np.maximum(b[o][1:], b[o][:-1])
            far = g > 2.2 * bb
            if ties:
                far |= (rows[o[1:]] == rows[o[:-1]]).all(1)
            if not far.all():
                return False
    return True


def search(base, ok):
    for seed in range(base, base + 2000):
        if ok(seed):
            return seed
    raise SystemExit(f"no seed in [{base}, {base + 2000})")


def search_seeds():
    """Re-seed every set until the gap condition holds for every space and print the constants to record above."""
    zs = [s for s in SPACES if s not in NO_ZEROS]
    print("MAIN_SEED =", search(20261017, lambda sd: helper_gaps_ok(zs, main_rows(True, sd), main_queries(True, sd), 101)
                                and helper_gaps_ok(NO_ZEROS, main_rows(False, sd), main_queries(False, sd), 101)), flush=True)
    print("DIMS_SEEDS =", {D: search(4242 + D, lambda sd: helper_gaps_ok(SPACES, dims_rows(D, sd), dims_queries(D, sd), 11))
                           for D in DIMS}, flush=True)
    print("DUPS_SEED =", search(99, lambda sd: helper_gaps_ok(SPACES, *inputs_dups(sd), 200, ties=True)), flush=True)
    print("TINY_SEED =", search(5, lambda sd: helper_gaps_ok(SPACES, *inputs_tiny(sd), 7)), flush=True)


def run_reference():
    L = C.CDLL(orc.REF_LIB)
    out = {}
    pairs = main_pairs()
    out["main_pairs"] = pairs
    out["seeds"] = np.array([MAIN_SEED, DUPS_SEED, TINY_SEED] + [DIMS_SEEDS[D] for D in DIMS], np.int64)
    for z in (False, True):
        out[f"main_rows_sha_z{int(z)}"] = sha(main_rows(z))
        out[f"main_queries_sha_z{int(z)}"] = sha(main_queries(z))
    for D in DIMS:
        out[f"dims{D}_sha"] = sha(dims_rows(D), dims_queries(D))
    dup_rows, dup_q = inputs_dups()
    tiny_rows, tiny_q = inputs_tiny()
    out["dups_sha"] = sha(dup_rows, dup_q)
    out["tiny_sha"] = sha(tiny_rows, tiny_q)
    for s in SPACES:
        rows, qs = main_rows(s not in NO_ZEROS), main_queries(s not in NO_ZEROS)
        ix = RefIndex(L, s, rows)
        ids, ds = ix.knn_all(qs)
        for k in (10, 100):
            out[f"{s}_k{k}_ids"], out[f"{s}_k{k}_dists"] = ids[:, :k].copy(), ds[:, :k].copy()
            out[f"{s}_k{k}_cnt"] = np.full(len(qs), k, np.int32)
        assert gaps_ok(s, rows, qs, ids, ds, 101).all(), (s, "main: re-seed (--search)")
        radii = np.stack([ds[:, 2], ds[:, 9]], axis=1).astype(np.float64)   # rows at the radius are in
        out[f"{s}_radii"] = radii
        for cap in RANGE_CAPS:
            rid, rd, rn = [], [], []
            for qi in range(len(qs)):
                for r in radii[qi]:
                    a, b = ix.range(qs[qi], r, cap)
                    rid.append(a)
                    rd.append(b)
                    rn.append(len(a))
            out[f"{s}_range{cap}_n"] = np.array(rn, np.int32)
            out[f"{s}_range{cap}_ids"] = np.concatenate(rid).astype(np.int32)
            out[f"{s}_range{cap}_dists"] = np.concatenate(rd).astype(np.float32)
        out[f"{s}_pair_dists"] = np.array([ix.distance(a, b) for a, b in pairs], np.float32)
        for D in DIMS:
            rows, qs = dims_rows(D), dims_queries(D)
            ix = RefIndex(L, s, rows)
            ids, ds = ix.knn_all(qs)
            out[f"{s}_dims{D}_ids"], out[f"{s}_dims{D}_dists"] = ids[:, :10].copy(), ds[:, :10].copy()
            assert gaps_ok(s, rows, qs, ids, ds, 11).all(), (s, D, "dims: re-seed (--search)")
        ix = RefIndex(L, s, dup_rows)
        ids, ds = ix.knn_all(dup_q)
        assert gaps_ok(s, dup_rows, dup_q, ids, ds, 200, ties=True).all(), (s, "dups: re-seed (--search)")
        out[f"{s}_dups_ids"], out[f"{s}_dups_dists"] = ids, ds
        ix = RefIndex(L, s, tiny_rows)
        ids, ds = ix.knn_all(tiny_q)
        assert gaps_ok(s, tiny_rows, tiny_q, ids, ds, 7).all(), (s, "tiny: re-seed (--search)")
        out[f"{s}_tiny_ids"], out[f"{s}_tiny_dists"], out[f"{s}_tiny_cnt"] = ix.knn_canonical(tiny_q, 10)  # k > n
        out[f"{s}_tiny_obj0"] = ix.data_point(0)
        print(s, "done", flush=True)
    return out


def main():
    if sys.argv[1:] == ["--search"]:
        return search_seeds()
    assert os.path.exists(orc.REF_LIB), "build oracle/_ref first: make -C oracle ref"
    out = run_reference()
    # np.savez_compressed stamps zip times: write the members with a fixed date so a rerun gives the same bytes
    with zipfile.ZipFile(GOLDEN, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(out):
            buf = io.BytesIO()
            np.save(buf, out[key], allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(2020, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(len(out), "arrays ->", GOLDEN, os.path.getsize(GOLDEN), "bytes")


if __name__ == "__main__":
    main()
