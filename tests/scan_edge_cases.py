"""The cases of tests/test_gpu_scan_plan_edges.py: one table, with the plan values each case is there for, the inputs, the
host references and the checkers.  tests/test_scan_plan_cpu.py holds every case's plan to the restatement
(tests/scan_plan_ref.py), asserts the conditions on the inputs from the references alone, and feeds the checkers corrupted
answers.

Inputs of the integer cases (bit_hamming, leven, integer-valued sparse).  Every query is a centre object with a few
changes, and the two rows on either side of every split boundary are copies of the centre: whatever k is, each query's
list holds a group of equal distances whose positions lie in different splits, so the merge has to order equal keys of
different lists by position.  External ids run against the positions (ext_ids), so an order by reported id shows."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from tests import diverg_ref, scan_plan_ref, sparse_ref

# plan: (nsplit, rows_per_split, rows of the last split, kl, P, tq) as scan_make_plan gives them for (n, nq, k, tq_asked);
# merge: the route of launch_merge_topk_ex
Case = namedtuple("Case", "name kind n nq k tq_asked plan merge opts")


def _case(kind, n, nq, k, tq_asked, plan, merge, tag="", **opts):
    return Case(f"{kind}{tag}_n{n}_q{nq}_k{k}", kind, n, nq, k, tq_asked, scan_plan_ref.Plan(*plan), merge, opts)


def ext_ids(n):
    return (n - 1 - np.arange(n)).astype(np.int32)


def seed_of(name):
    return zlib.crc32(name.encode())


def _per_case(fn):
    """cache by the case's name (and the other arguments): the CPU and the GPU tests share inputs and references"""
    memo = {}

    @functools.wraps(fn)
    def cached(case, *args):
        key = (case.name,) + args
        if key not in memo:
            memo[key] = fn(case, *args)
        return memo[key]
    return cached


# ---- the table -------------------------------------------------------------------------------------------------------
_H = functools.partial(_case, "ham")
HAM_SWEEP = [
    # one split turning into two; then the last split holds one row
    _H(1023, 1, 10, 8, (1, 1024, 1023, 10, 512, 8), "lds"),
    _H(1024, 1, 10, 8, (1, 1024, 1024, 10, 512, 8), "lds"),
    _H(1025, 1, 10, 8, (2, 1024, 1, 10, 512, 8), "lds"),
    # the last split has fewer rows than kl, in a partial second tile
    _H(1025, 9, 100, 8, (2, 1024, 1, 100, 512, 8), "lds"),
    # three splits with a one-row last split; P 512 -> 1024
    _H(2049, 8, 256, 8, (3, 1024, 1, 256, 512, 8), "lds"),
    _H(2049, 8, 257, 8, (3, 1024, 1, 257, 1024, 8), "lds"),
    # tq 8 -> 1
    _H(3000, 7, 768, 8, (3, 1024, 952, 768, 1024, 8), "lds"),
    _H(3000, 9, 769, 8, (3, 1024, 952, 769, 2048, 1), "lds"),
    # kl = rows_per_split; k around n over two splits; k > n
    _H(2100, 8, 1024, 8, (3, 1024, 52, 1024, 2048, 1), "lds"),
    _H(2100, 8, 1025, 8, (3, 1024, 52, 1024, 2048, 1), "lds"),
    _H(1300, 3, 1299, 8, (2, 1024, 276, 1024, 2048, 1), "lds"),
    _H(1300, 3, 1300, 8, (2, 1024, 276, 1024, 2048, 1), "lds"),
    _H(1300, 3, 1301, 8, (2, 1024, 276, 1024, 2048, 1), "lds"),
    _H(1025, 3, 1030, 8, (2, 1024, 1, 1024, 2048, 1), "lds"),
    # the merge bound 8192 / k: three splits of 1024 -> two of 1500
    _H(3000, 3, 2730, 8, (3, 1024, 952, 1024, 2048, 1), "lds"),
    _H(3000, 3, 2731, 8, (2, 1500, 1500, 1500, 2048, 1), "lds"),
    # the big-k rule: LDS merge -> bisection merge
    _H(5000, 3, 4096, 8, (2, 2500, 2500, 2500, 4096, 1), "lds"),
    _H(5000, 3, 4097, 8, (2, 4096, 904, 4096, 8192, 1), "bisect"),
    # one list -> two, with a one-row second list
    _H(4096, 2, 4097, 8, (1, 4096, 4096, 4096, 8192, 1), "lds"),
    _H(4097, 2, 4097, 8, (2, 4096, 1, 4096, 8192, 1), "bisect"),
    # a single list: nsplit * k = 8192 / 8193
    _H(3000, 2, 8192, 8, (1, 4096, 3000, 4096, 8192, 1), "lds"),
    _H(3000, 2, 8193, 8, (1, 4096, 3000, 4096, 8192, 1), "bisect"),
    # four and three lists in the bisection merge, with a short last list
    _H(12289, 3, 4097, 8, (4, 4096, 1, 4096, 8192, 1), "bisect"),
    _H(9000, 2, 8200, 8, (3, 4096, 808, 4096, 8192, 1), "bisect"),
]
# 2047 tiles -> 2048 tiles: two splits -> one.  32 bits; one set of rows and queries, the first case takes all but the
# last query
HAM_TILES = [
    _H(1100, 16376, 5, 8, (2, 1024, 76, 5, 512, 8), "lds", bits=32, inputs="tiles", plant=1024, gen_nq=16377),
    _H(1100, 16377, 5, 8, (1, 1100, 1100, 5, 512, 8), "lds", bits=32, inputs="tiles", plant=1024, gen_nq=16377),
]
# every row passes the running threshold of query 0: the buffer fills to exactly P before each compaction
HAM_PRESSURE = [
    _H(2049, 8, 10, 8, (3, 1024, 1, 10, 512, 8), "lds", tag="_pressure", bits=1056, pressure=True),
    _H(2049, 8, 256, 8, (3, 1024, 1, 256, 512, 8), "lds", tag="_pressure", bits=1056, pressure=True),
    _H(2049, 8, 768, 8, (3, 1024, 1, 768, 1024, 8), "lds", tag="_pressure", bits=1056, pressure=True),
]
# W = 1, 1, 2, 3, 4, 5 words (the wide loads of W % 4 == 0 against the scalar tail); W = 512: the tile's queries staged
# in LDS, W = 513: read from HBM
HAM_WIDTHS = [_H(1025, 9, 10, 8, (2, 1024, 1, 10, 512, 8), "lds", tag=f"_b{b}", bits=b)
              for b in (1, 31, 33, 96, 128, 160, 16384, 16385)]
HAM_CASES = HAM_SWEEP + HAM_TILES + HAM_PRESSURE + HAM_WIDTHS

_L = functools.partial(_case, "leven")
LEVEN_CASES = [
    _L(1025, 9, 10, 8, (2, 1024, 1, 10, 512, 8), "lds", alpha=b"acgt", qlen=10),
    _L(2049, 8, 257, 8, (3, 1024, 1, 257, 1024, 8), "lds", alpha=b"abc", qlen=8),
    _L(3000, 9, 769, 8, (3, 1024, 952, 769, 2048, 1), "lds", alpha=b"ab", qlen=7),
    _L(4097, 2, 4097, 8, (2, 4096, 1, 4096, 8192, 1), "bisect", alpha=b"abc", qlen=9),
    # rows 0-511 hold 60-90 bytes: their 256-row chunks exceed the 16 KiB row stage and are read from HBM, in split 0
    # only; every other chunk is staged
    _L(2049, 8, 257, 8, (3, 1024, 1, 257, 1024, 8), "lds", tag="_longrows", alpha=b"ab", qlen=64, long_rows=512),
]
# Multi-block queries over 1025 rows (two splits, one row in the second): 256 / 257 bytes = 4 / 5 blocks, the blocks'
# state in LDS / in HBM; 512 / 513 bytes = 8 / 9 blocks, Peq staged / read from HBM.  The C ABI gives every query of a
# batch one length, so each length is a batch of its own, of LEVEN_MW_PER_LEN queries (blockIdx.y > 0: tq = 1).  The
# 5-byte queries run the one-block kernel.
LEVEN_MW_LENGTHS = (5, 256, 257, 512, 513, 600)
LEVEN_MW_PER_LEN = 2
LEVEN_MW_CASES = [
    _L(1025, 2, 10, 8, (2, 1024, 1, 10, 512, 8), "lds", tag="_len5", qlen=5),
    _L(1025, 2, 1030, 8, (2, 1024, 1, 1024, 2048, 1), "lds", tag="_len5", qlen=5),
] + [_L(1025, 2, k, 1, plan, "lds", tag=f"_len{m}", qlen=m)
     for m in LEVEN_MW_LENGTHS[1:]
     for k, plan in ((10, (2, 1024, 1, 10, 512, 1)), (1030, (2, 1024, 1, 1024, 2048, 1)))]

_S = functools.partial(_case, "sparse")
SPARSE_SHAPES = [
    ((1025, 9, 10), (2, 1024, 1, 10, 512, 8), "lds"),
    ((2049, 8, 257), (3, 1024, 1, 257, 1024, 8), "lds"),
    ((3000, 9, 769), (3, 1024, 952, 769, 2048, 1), "lds"),
    ((5000, 3, 4097), (2, 4096, 904, 4096, 8192, 1), "bisect"),
    ((3000, 2, 8193), (1, 4096, 3000, 4096, 8192, 1), "bisect"),
]
SPARSE_CASES = [_S(*shape, 8, plan, merge, tag="_" + space.split("_")[0], space=space)
                for space in ("l1_sparse", "negdotprod_sparse") for shape, plan, merge in SPARSE_SHAPES]
# a tile whose queries hold 4096 elements together is staged in LDS, one with 4097 is read from HBM
SPARSE_STAGE_CASES = [
    _S(1025, 8, 10, 8, (2, 1024, 1, 10, 512, 8), "lds", tag=f"_stage{total}", space="l1_sparse", q_elems=total)
    for total in (4096, 4097)]
SPARSE_COSINE = _S(2049, 9, 100, 8, (3, 1024, 1, 100, 512, 8), "lds", tag="_cosine", space="cosinesimil_sparse")

DIVERG_SPACES = ("kldivfast", "itakurasaitofast", "jsmetrfast")
_D = functools.partial(_case, "diverg")
DIVERG_SHAPES = [
    # the 64-row block of the row layout: the padded rows of the last block are never offered
    _D(63, 3, 10, 16, (1, 1024, 63, 10, 512, 16), "lds", D=4),
    _D(64, 3, 10, 16, (1, 1024, 64, 10, 512, 16), "lds", D=4),
    _D(65, 3, 10, 16, (1, 1024, 65, 10, 512, 16), "lds", D=4),
    _D(1025, 17, 10, 16, (2, 1024, 1, 10, 512, 16), "lds", D=4),
    _D(3000, 15, 768, 16, (3, 1024, 952, 768, 1024, 16), "lds", D=4),
    _D(3000, 17, 769, 16, (3, 1024, 952, 769, 2048, 1), "lds", D=4),
    _D(4097, 3, 4097, 16, (2, 4096, 1, 4096, 8192, 1), "bisect", D=4),
    # the tail group: D = 5 and 7 leave one and three elements in the last group of four
    _D(1025, 17, 10, 16, (2, 1024, 1, 10, 512, 16), "lds", tag="_D5", D=5),
    _D(1025, 17, 10, 16, (2, 1024, 1, 10, 512, 16), "lds", tag="_D7", D=7),
]
# nsplit * nq * k = 2 * 4100 * 4097 > 2^25: scan_slices halves the slice to 2050 queries, no multiple of the tile of 16.
# plan: the plan of a slice
DIVERG_SLICED = _D(4097, 4100, 4097, 16, (2, 4096, 1, 4096, 8192, 1), "bisect", tag="_sliced", D=4,
                   slices=((0, 2050), (2050, 2050)))
DIVERG_SAMPLE = 40

ALL_CASES = (HAM_CASES + LEVEN_CASES + LEVEN_MW_CASES + SPARSE_CASES + SPARSE_STAGE_CASES + [SPARSE_COSINE] +
             DIVERG_SHAPES + [DIVERG_SLICED])
INTEGER_CASES = HAM_CASES + LEVEN_CASES + LEVEN_MW_CASES + SPARSE_CASES + SPARSE_STAGE_CASES
# The 5-byte queries at k = 10 share the rows of the multi-block queries, whose two boundary rows are the nearest rows of
# every LONG query (12 bytes, the only rows that long); a 5-byte query is at least 7 edits from them.  Their tie order
# across the boundary is the business of leven_n1025_q9_k10.
NO_BOUNDARY_TIE = {"leven_len5_n1025_q2_k10"}


def boundaries(case):
    """positions of the first row of every split but the first"""
    rps = case.opts.get("plant", case.plan.rows_per_split)
    return list(range(rps, case.n, rps))


# ---- answers ---------------------------------------------------------------------------------------------------------
def topk_exact(d, k):
    """d [nq][n] integers (or exact floats) -> positions [nq][k] (-1 pad), distances f32 [nq][k] (inf pad), in
    (distance, position) order"""
    nq, n = d.shape
    m = min(n, k)
    key = d.astype(np.int16) if d.dtype.kind == "i" and d.size and np.abs(d).max() < 32767 else d
    o = np.argsort(key, axis=1, kind="stable")[:, :m]
    pos = np.full((nq, k), -1, np.int32)
    dist = np.full((nq, k), np.inf, np.float32)
    pos[:, :m] = o
    dist[:, :m] = np.take_along_axis(d, o, axis=1)
    return pos, dist


def has_boundary_tie(pos, dist, rps):
    """per query: two rows of equal distance in different splits, both in the list (a group of equal distances is in
    position order, so its splits change between two neighbours)"""
    valid = pos >= 0
    split = pos // rps
    same = (dist[:, 1:] == dist[:, :-1]) & valid[:, 1:] & valid[:, :-1]
    return (same & (split[:, 1:] != split[:, :-1])).any(axis=1)


def _common(got, n, k, nq):
    ids, ds, cnt = got
    assert ids.shape == (nq, k) and ds.shape == (nq, k) and cnt.shape == (nq,), "shapes"
    m = min(n, k)
    assert (cnt == m).all(), f"counts {np.unique(cnt).tolist()}, expected {m}"
    past = np.arange(k)[None, :] >= np.asarray(cnt)[:, None]
    assert (ids[past] == -1).all(), "an id past the count"
    assert np.isposinf(ds[past]).all(), "a distance past the count is not +inf"
    return m


def check_exact(got, want, n):
    """got = (ids, dists, counts) of the engine with ext_ids(n); want = (positions, distances) of topk_exact"""
    pos, dist = want
    nq, k = pos.shape
    m = _common(got, n, k, nq)
    ext = ext_ids(n)
    np.testing.assert_array_equal(got[1][:, :m], dist[:, :m], err_msg="distances")
    np.testing.assert_array_equal(got[0][:, :m], ext[pos[:, :m]], err_msg="ids")


def check_sparse_float(got, want, n):
    """distances by close_rel at the project's 1e-5, ids equal outside groups of equal expected distances"""
    from tests.gpuutil import close_rel
    from tests.test_gpu_sparse import ids_match_within_ties
    pos, dist = want
    nq, k = pos.shape
    m = _common(got, n, k, nq)
    assert close_rel(got[1][:, :m], dist[:, :m]), "distances"
    got_pos = n - 1 - got[0][:, :m]
    assert ids_match_within_ties(got_pos, got[1][:, :m], pos[:, :m], dist[:, :m]), "ids"


def check_diverg(space, got, want, n):
    """as test_k_above_the_split_list_limit: distances within diverg_ref's bound, ids equal outside near_tie_mask"""
    pos, d, b = want                      # [nq][min(k, n)]
    nq, k = got[0].shape
    m = _common(got, n, k, nq)
    assert pos.shape == (nq, m)
    assert (np.abs(diverg_ref.comparable(space, got[1][:, :m]) - d) <= b).all(), "distances"
    ties = diverg_ref.near_tie_mask(d, b)
    assert (got[0][:, :m][~ties] == ext_ids(n)[pos][~ties]).all(), "ids"


# ---- bit_hamming -------------------------------------------------------------------------------------------------------
_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def pack_words(B):
    """B [n][bits] of 0 / 1 -> uint32 words [n][W], bit i in word i / 32 at i % 32 (the reference's Binarize)"""
    n, bits = B.shape
    W = (bits + 31) // 32
    full = np.zeros((n, W * 32), np.uint8)
    full[:, :bits] = B
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view("<u4")


def ham_distances(R, Q):
    """R [n][W], Q [nq][W] words -> [nq][n] popcounts of XOR, by a byte table"""
    out = np.empty((len(Q), len(R)), np.int32)
    for qi in range(len(Q)):
        out[qi] = _POP[np.bitwise_xor(R, Q[qi]).view(np.uint8)].sum(axis=1, dtype=np.int64)
    return out


def bits_text(B):
    """the text of bit_hamming objects, "0 1 1 0" """
    buf = np.full((B.shape[0], 2 * B.shape[1]), 32, np.uint8)
    buf[:, ::2] = B + 48
    return [r[:-1].tobytes() for r in buf]


@functools.lru_cache(maxsize=4)
def _ham_bits(name, n, nq, bits, plant_at, pressure):
    rng = np.random.default_rng(seed_of(name))
    if pressure:
        # rows 2j - 1 and 2j hold 1025 - j leading ones: for the all-zero query 0 the distance falls from pair to pair,
        # and a pair lies across every chunk and split boundary.  Queries 1.. have five ones: the last rows are their
        # nearest as well, and a key written past query 0's buffer would land in theirs
        ones = 1025 - (np.arange(n) + 1) // 2
        B = (np.arange(bits)[None, :] < ones[:, None]).astype(np.uint8)
        Q = np.zeros((nq, bits), np.uint8)
        for q in range(1, nq):
            Q[q, rng.choice(bits, size=5, replace=False)] = 1
        return B, Q
    c = rng.integers(0, 2, size=bits, dtype=np.uint8)
    B = rng.integers(0, 2, size=(n, bits), dtype=np.uint8)
    if bits < 16:
        B[:] = 1 - c          # (half of all random rows would equal the centre)
    for b in plant_at:
        B[b - 1] = c
        B[b] = c
    Q = np.tile(c, (nq, 1))
    for _ in range(min(2, bits // 16)):
        sel = rng.random(nq) < 0.7
        at = rng.integers(0, bits, size=nq)
        Q[sel, at[sel]] ^= 1
    return B, Q


def ham_inputs(case):
    """-> rows [n][bits], queries [nq][bits] of 0 / 1"""
    bits = case.opts.get("bits", 64)
    name = case.opts.get("inputs", case.name)
    B, Q = _ham_bits(name, case.n, case.opts.get("gen_nq", case.nq), bits, tuple(boundaries(case)),
                     bool(case.opts.get("pressure")))
    return B, Q[:case.nq]


@functools.lru_cache(maxsize=2)
def _ham_distances_of(name, n, gen_nq, bits, plant_at, pressure):
    B, Q = _ham_bits(name, n, gen_nq, bits, plant_at, pressure)
    return ham_distances(pack_words(B), pack_words(Q))


def ham_reference(case, k=None):
    bits = case.opts.get("bits", 64)
    d = _ham_distances_of(case.opts.get("inputs", case.name), case.n, case.opts.get("gen_nq", case.nq), bits,
                          tuple(boundaries(case)), bool(case.opts.get("pressure")))
    return topk_exact(d[:case.nq], case.k if k is None else k)


# ---- leven -------------------------------------------------------------------------------------------------------------
def leven_rows_to_query(rows, q):
    """string_ref.levenshtein(row, q) for every row at once: the same recurrence, one text symbol per step"""
    m, n = len(q), len(rows)
    qa = np.frombuffer(q, np.uint8)
    lens = np.array([len(r) for r in rows])
    T = np.zeros((n, int(lens.max())), np.uint8)
    for i, r in enumerate(rows):
        T[i, :len(r)] = np.frombuffer(r, np.uint8)
    ar = np.arange(1, m + 1)
    prev = np.tile(np.arange(m + 1, dtype=np.int64), (n, 1))
    out = np.full(n, m, np.int64)
    for j in range(T.shape[1]):
        best = np.minimum(prev[:, :-1] + (qa[None, :] != T[:, j:j + 1]), prev[:, 1:] + 1)
        run = np.minimum.accumulate(np.minimum(best - ar, j + 1), axis=1)
        prev = np.concatenate([np.full((n, 1), j + 1, np.int64), run + ar], axis=1)
        done = lens == j + 1
        out[done] = prev[done, -1]
    return out


def _rand_str(rng, lo, hi, alpha, p=None):
    return bytes(rng.choice(np.frombuffer(alpha, np.uint8), size=int(rng.integers(lo, hi + 1)), p=p))


@_per_case
def leven_inputs(case):
    """-> rows, queries (bytes)"""
    rng = np.random.default_rng(seed_of(case.name))
    alpha, m = case.opts["alpha"], case.opts["qlen"]
    rows = [_rand_str(rng, 1, 12, alpha) for _ in range(case.n)]
    for i in range(case.opts.get("long_rows", 0)):
        rows[i] = _rand_str(rng, 60, 90, alpha)
    c = _rand_str(rng, m, m, alpha)
    for b in boundaries(case):
        rows[b - 1] = rows[b] = c
    qs = []
    for _ in range(case.nq):
        q = bytearray(c)
        for at in rng.integers(0, m, size=int(rng.integers(0, 3))):
            q[at] = alpha[int(rng.integers(0, len(alpha)))]
        qs.append(bytes(q))
    return rows, qs


def _runs(rng, m, alpha, first):
    """m bytes in runs of m / 6 to m / 3 equal letters (four or five runs), neighbours different, the first run of `first`"""
    out, last = b"", None
    while len(out) < m:
        c = first if last is None else int(rng.choice([x for x in alpha if x != last]))
        out += bytes([c]) * int(rng.integers(m // 6, m // 3 + 1))
        last = c
    return out[:m]


@functools.lru_cache(maxsize=None)
def leven_mw_inputs():
    """-> rows, {length: queries}.  Rows of 1-11 bytes over abc, and two of twelve a's across the split boundary.  A long
    query is a few runs of equal letters, the first of a's: its distance to a row is its length less their longest
    common subsequence, which depends on the order of the row's letters (0-11 over the rows) and is 12 for the two
    boundary rows alone, the nearest rows of every long query."""
    rng = np.random.default_rng(seed_of("leven_mw"))
    rows = [_rand_str(rng, 1, 11, b"abc") for _ in range(1025)]
    rows[1023] = rows[1024] = b"a" * 12
    qs = {m: [_runs(rng, m, b"abc", ord("a")) if m > 64 else _rand_str(rng, m, m, b"abc")
              for _ in range(LEVEN_MW_PER_LEN)] for m in LEVEN_MW_LENGTHS}
    return rows, qs


def leven_case_inputs(case):
    if case in LEVEN_MW_CASES:
        rows, qs = leven_mw_inputs()
        return rows, qs[case.opts["qlen"]]
    return leven_inputs(case)


@functools.lru_cache(maxsize=None)
def _leven_distances(case_key):
    rows, qs = case_key
    return np.array([leven_rows_to_query(rows, q) for q in qs])


def leven_reference(case, k=None):
    rows, qs = leven_case_inputs(case)
    return topk_exact(_leven_distances((tuple(rows), tuple(qs))), case.k if k is None else k)


# ---- sparse ------------------------------------------------------------------------------------------------------------
def _sparse_row(rng, lo, hi, vocab, value):
    m = int(rng.integers(lo, hi + 1))
    ids = np.sort(rng.choice(vocab, size=m, replace=False)).astype(np.uint32)
    return ids, value(rng, m)


def _int_values(rng, m):
    return rng.integers(1, 4, size=m).astype(np.float32)


@_per_case
def sparse_inputs(case):
    """-> rows, queries as (ids, values).  Integer values 1-3: the l1 and dot-product distances are exact in float32.
    The centre holds six ids with value 3; a query is the centre with one value lowered (the staging cases add elements
    up to their counts), so the copies of the centre at the split boundaries are its nearest rows in both spaces."""
    rng = np.random.default_rng(seed_of(case.name))
    if case.opts["space"] == "cosinesimil_sparse":
        value = lambda r, m: r.uniform(0.1, 1.0, size=m).astype(np.float32)          # noqa: E731
        rows = [_sparse_row(rng, 3, 8, 60, value) for _ in range(case.n)]
        return rows, [_sparse_row(rng, 4, 8, 60, value) for _ in range(case.nq)]
    total = case.opts.get("q_elems")
    vocab = 2000 if total else 40
    rows = [_sparse_row(rng, 1, 6, vocab, _int_values) for _ in range(case.n)]
    cid = np.sort(rng.choice(vocab, size=6, replace=False)).astype(np.uint32)
    centre = (cid, np.full(6, 3, np.float32))
    for b in boundaries(case):
        rows[b - 1] = rows[b] = centre
    counts = [6] * case.nq
    if total:
        counts = [total // case.nq] * case.nq
        counts[-1] += total - sum(counts)
    qs = []
    for m in counts:
        v = centre[1].copy()
        v[int(rng.integers(0, 6))] = float(rng.integers(1, 4))
        others = rng.choice(np.setdiff1d(np.arange(vocab, dtype=np.uint32), cid), size=m - 6, replace=False)
        ids = np.concatenate([cid, others.astype(np.uint32)])
        vals = np.concatenate([v, _int_values(rng, m - 6)])
        o = np.argsort(ids)
        qs.append((ids[o], vals[o]))
    return rows, qs


@_per_case
def _sparse_full(case):
    rows, qs = sparse_inputs(case)
    return sparse_ref.seq_search(case.opts["space"], rows, qs, case.n)


def sparse_reference(case, k=None):
    """sparse_ref.seq_search in (distance, position) order, cut (or padded) to k"""
    k = case.k if k is None else k
    pos, dist = _sparse_full(case)
    m = min(k, case.n)
    p = np.full((case.nq, k), -1, np.int32)
    d = np.full((case.nq, k), np.inf, np.float32)
    p[:, :m], d[:, :m] = pos[:, :m], dist[:, :m]
    return p, d


# ---- divergences -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def diverg_rows(D):
    """diverg_ref.bigk_inputs() for D = 4; other lengths the way that helper draws its rows"""
    if D == 4:
        return diverg_ref.bigk_inputs()[0]
    rng = np.random.default_rng(61 + D)
    scale = np.exp(np.linspace(np.log(10.0), np.log(1e8), 6000))[rng.permutation(6000), None]
    h0 = np.arange(1, D + 1) / (D * (D + 1) / 2)
    return (scale * h0 * (1 + 0.001 * rng.uniform(-1, 1, size=(6000, D)))).astype(np.float32)


def diverg_inputs(case):
    """-> rows (the first n of diverg_rows), queries (drawn as bigk_inputs draws them)"""
    D = case.opts["D"]
    rng = np.random.default_rng(seed_of(case.name))
    return diverg_rows(D)[:case.n], rng.uniform(0.2, 1.0, size=(case.nq, D)).astype(np.float32)


def diverg_sample(case):
    """the queries of the sliced batch that are checked: the first and last of every slice and others up to 40"""
    edge = sorted({q for q0, m in case.opts["slices"] for q in (q0, q0 + m - 1)})
    rng = np.random.default_rng(seed_of(case.name) + 1)
    rest = rng.choice(np.setdiff1d(np.arange(case.nq), edge), size=DIVERG_SAMPLE - len(edge), replace=False)
    return np.sort(np.concatenate([edge, rest]).astype(np.int64))


@_per_case
def diverg_reference(case, space, k):
    """-> positions, float64 distances, bounds [nq][min(k, n)] (the sliced case: of its sample)"""
    rows, qs = diverg_inputs(case)
    if "slices" in case.opts:
        qs = qs[diverg_sample(case)]
    return diverg_ref.seq_search(space, rows, qs, k)


# ---- corrupted answers (tests/test_scan_plan_cpu.py: every checker rejects each) ----------------------------------------
def answer_of(pos, dist, n):
    """the engine's answer that equals a reference: (ids, dists, counts)"""
    pos = np.asarray(pos)
    nq, k = pos.shape
    ids = np.where(pos >= 0, ext_ids(n)[np.maximum(pos, 0)], -1).astype(np.int32)
    return ids, np.asarray(dist, np.float32).copy(), np.full(nq, min(n, k), np.int32)


def swap_ranks(ans, q, i, j):
    ids, ds, cnt = (a.copy() for a in ans)
    ids[q, i], ids[q, j] = ans[0][q, j], ans[0][q, i]
    return ids, ds, cnt


def drop_row(ans_k1, q, ext_id, n):
    """ans_k1: the answer at k + 1.  -> the answer at k of an engine that never offers the row reported as ext_id"""
    ids, ds, cnt = (a.copy() for a in ans_k1)
    k = ids.shape[1] - 1
    at = int(np.nonzero(ids[q] == ext_id)[0][0])
    ids[q, at:-1], ds[q, at:-1] = ans_k1[0][q, at + 1:], ans_k1[1][q, at + 1:]
    valid = np.minimum((ids[:, :k] >= 0).sum(axis=1), k).astype(np.int32)
    valid[np.arange(len(valid)) != q] = min(n, k)
    return ids[:, :k], ds[:, :k], valid


def count_off(ans, q, by):
    ids, ds, cnt = (a.copy() for a in ans)
    cnt[q] += by
    return ids, ds, cnt


def fill_padding(ans, q, n):
    """k > n: the first padding slot of query q holds a real id and distance"""
    ids, ds, cnt = (a.copy() for a in ans)
    ids[q, n], ds[q, n] = ids[q, n - 1], ds[q, n - 1]
    return ids, ds, cnt
