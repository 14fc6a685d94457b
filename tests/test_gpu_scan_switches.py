"""The dense exact scan at every switch of its plans (bf_make_plan, bf_u8_fast_plan, bf_f32_fast_plan, bf_l1_fast_plan):
the shape on either side of each threshold in n, nq, k and D goes through the host ABI; the chain taken is read from
stats(), the answer is checked against the oracle's full scan on the first and last 8 queries and, where an environment
gate can send the same batch down the other chain of the same index, against that chain bit for bit.

Thresholds (from the plans): n = 65536 for every fast path; nq = 256 (f32, l1), 512 (u8), 1024 (f32: 256 -> 512 queries
per tile), 2048 (u8: 256 -> 512); k = 128 (f32, l1), 256 (u8), 512 (selection kernels -> big-k scan), 24 (l1 list size);
D = 128 / 256 / 384 / 512 / 768 / 1024 (chunks of 128 per row: 1, 2, 3, 4, 6, 8, then no fast path; centred cosine
carries 3 more columns), 256 (l1)."""
import numpy as np
import pytest

from . import orc, refio
from .gpuutil import close_rel, expect_path, ids_match_modulo_near_ties, make_index, same_bits

pytestmark = pytest.mark.gpu

N = 65536
GATES = {1: "NMSLIB_GPU_F32_FAST", 3: "NMSLIB_GPU_U8_FAST", 6: "NMSLIB_GPU_L1_FAST"}


def _ends(nq):
    return np.r_[0:min(8, nq), max(nq - 8, 8):nq]


def check_oracle(space, X, Q, k, got):
    """The first and last 8 queries against the oracle's scan: the suite's bars."""
    ids, ds, cnt = got
    assert (cnt == min(k, len(X))).all()
    sel = _ends(len(Q))
    if space == "l2sqr_sift":
        opos, odist, _ = orc.seq_search(space, X, Q[sel], k)
        np.testing.assert_array_equal(ds[sel], odist)
        np.testing.assert_array_equal(ids[sel], opos)
        return
    opos, odist, _ = orc.seq_search(space, X, Q[sel], k + 22)
    rec = refio.recall_nmslib(ids[sel], opos, odist, k)
    assert rec >= 0.999, rec
    rtol, atol = (1e-4, 1e-5) if space == "angulardist" else (1e-5, 1e-6)
    assert close_rel(ds[sel], odist[:, :k], rtol=rtol, atol=atol)


def run_case(idx, space, X, Q, k, path, monkeypatch, gate=None, **stats):
    """One batch: the chain, the oracle, and (fast paths) the adaptive chain of the same index bit for bit."""
    got = idx.knnQueryBatch(Q, k)
    expect_path(idx, path, **stats)
    check_oracle(space, X, Q, k, got)
    gate = gate or GATES.get(path)
    if gate and path in GATES:
        monkeypatch.setenv(gate, "0")
        other = idx.knnQueryBatch(Q, k)
        expect_path(idx, 2 if space == "l2sqr_sift" else 0)
        monkeypatch.delenv(gate)
        same_bits(got, other)
    return got


class _Cache:
    """Rows and indexes made when first asked for and shared by the module's cases."""

    def __init__(self):
        self.rows, self.idx = {}, {}

    def data(self, key, make):
        if key not in self.rows:
            self.rows[key] = make()
        return self.rows[key]

    def index(self, key, space, make):
        if key not in self.idx:
            X = make()
            self.idx[key] = (make_index(space, "seq_search", X), X)
        return self.idx[key]

    def drop(self, key):
        if key in self.idx:
            self.idx.pop(key)[0].close()

    def close(self):
        for i, _ in self.idx.values():
            i.close()
        self.idx.clear()


@pytest.fixture(scope="module")
def cache():
    c = _Cache()
    yield c
    c.close()


def _rows32(c):
    return c.data("x32", lambda: refio.s_lowrank(N, 32, 501))


def _rows_u8(c):
    return c.data("u8", lambda: refio.s_sift_like(N, 503))


def _rows128(c):
    return c.data("x128", lambda: refio.s_lowrank(N, 128, 505))


def _wide(c):
    """65536 x 1025 rows and 256 queries; the cases of D take the leading columns"""
    return c.data("wide", lambda: (refio.s_lowrank(N, 1025, 507), refio.s_lowrank(256, 1025, 508)))


def _index32(c, space):
    return c.index(("n32", space), space, lambda: _rows32(c))


def _index_u8(c):
    return c.index("nu8", "l2sqr_sift", lambda: _rows_u8(c))


Q32 = lambda nq: refio.s_lowrank(nq, 32, 502)       # noqa: E731
QU8 = lambda nq: refio.s_sift_like(nq, 504)         # noqa: E731


# ---- n ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N - 1, N])
@pytest.mark.parametrize("space,nq,fast", [("l2", 256, 1), ("l2sqr_sift", 512, 3), ("l1", 256, 6)])
def test_rows_threshold(cache, monkeypatch, space, nq, fast, n):
    u8 = space == "l2sqr_sift"
    rows = _rows_u8(cache) if u8 else _rows32(cache)
    Q = QU8(nq) if u8 else Q32(nq)
    if n == N:
        idx, X = _index_u8(cache) if u8 else _index32(cache, space)
        run_case(idx, space, X, Q, 10, fast, monkeypatch)
    else:
        X = rows[:n]
        idx = make_index(space, "seq_search", X)
        run_case(idx, space, X, Q, 10, 2 if u8 else 0, monkeypatch)
        idx.close()


# ---- nq -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space,nq,path,tiles", [
    ("l2", 255, 0, None), ("l2", 256, 1, 1),
    ("l1", 255, 0, None), ("l1", 256, 6, 2),
    ("l2sqr_sift", 511, 2, None), ("l2sqr_sift", 512, 3, 2),
    ("l2sqr_sift", 2047, 3, 8), ("l2sqr_sift", 2048, 3, 4)])
def test_batch_threshold(cache, monkeypatch, space, nq, path, tiles):
    u8 = space == "l2sqr_sift"
    idx, X = _index_u8(cache) if u8 else _index32(cache, space)
    more = {} if tiles is None else {"fast_tiles": tiles}
    run_case(idx, space, X, QU8(nq) if u8 else Q32(nq), 10, path, monkeypatch, **more)


@pytest.mark.parametrize("nq,tiles", [(1023, 4), (1024, 2)])
def test_batch_threshold_f32_tile_size(cache, monkeypatch, nq, tiles):
    """D = 128 (one chunk): 256 queries per workgroup below 1024 queries, 512 from there on."""
    idx, X = cache.index("x128", "l2", lambda: _rows128(cache))
    run_case(idx, "l2", X, refio.s_lowrank(nq, 128, 506), 10, 1, monkeypatch, fast_tiles=tiles)


# ---- k ------------------------------------------------------------------------------------------------------------
K_CASES = [("l2", 256, 128, 1), ("l2", 256, 129, 0), ("l2", 256, 256, 0), ("l2", 256, 512, 0), ("l2", 256, 513, 5),
           ("l2sqr_sift", 512, 256, 3), ("l2sqr_sift", 512, 257, 2), ("l2sqr_sift", 512, 512, 2), ("l2sqr_sift", 512, 513, 5),
           ("l1", 256, 24, 6), ("l1", 256, 25, 6), ("l1", 256, 128, 6)]


@pytest.fixture(scope="module")
def k512(cache):
    """the k = 512 answers of the l2 and the u8 index, which the k = 513 cases are compared with"""
    out = {}
    for space in ("l2", "l2sqr_sift"):
        u8 = space == "l2sqr_sift"
        idx, X = _index_u8(cache) if u8 else _index32(cache, space)
        out[space] = idx.knnQueryBatch(QU8(512) if u8 else Q32(256), 512)
    return out


@pytest.mark.parametrize("space,nq,k,path", K_CASES)
def test_k_threshold(cache, monkeypatch, k512, space, nq, k, path):
    u8 = space == "l2sqr_sift"
    idx, X = _index_u8(cache) if u8 else _index32(cache, space)
    Q = QU8(nq) if u8 else Q32(nq)
    ids, ds, cnt = run_case(idx, space, X, Q, k, path, monkeypatch)
    if k == 513:
        # the big-k scan's first 512 columns hold the rows of the selection kernels' k = 512 answer
        i512, d512, _ = k512[space]
        if u8:
            np.testing.assert_array_equal(ids[:, :512], i512)
            np.testing.assert_array_equal(ds[:, :512], d512)
        else:
            bad = ids_match_modulo_near_ties(ids[:, :512], i512, d512, lambda v: 1e-5 * v + 1e-6, got_key=ds[:, :512])
            assert not bad, bad[:10]
            assert close_rel(ds[:, :512], d512)


# ---- D ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [128, 129, 256, 257, 384, 385, 512, 513, 768, 769, 1024, 1025])
def test_dimension_threshold_l2(cache, monkeypatch, D):
    """128 columns per chunk: 1, 2, 3, 4, 6, 8 chunks; one chunk scans 256 queries per workgroup (1 tile), more chunks 128
    (2 tiles); 1025 columns have no fast path."""
    XW, QW = _wide(cache)
    X, Q = np.ascontiguousarray(XW[:, :D]), np.ascontiguousarray(QW[:, :D])
    idx = make_index("l2", "seq_search", X)
    if D > 1024:
        run_case(idx, "l2", X, Q, 10, 0, monkeypatch)
    else:
        run_case(idx, "l2", X, Q, 10, 1, monkeypatch, fast_tiles=1 if D <= 128 else 2)
    idx.close()


@pytest.mark.parametrize("D", [125, 126, 1021, 1022])
def test_dimension_threshold_centred_cosine(cache, monkeypatch, D):
    """rows with a +1.5 offset are scanned as centred rows of D + 3 columns: 128 | 129 and 1024 | 1025"""
    XW, QW = _wide(cache)
    X = (XW[:, :D] + np.float32(1.5)).astype(np.float32)
    Q = (QW[:, :D] + np.float32(1.5)).astype(np.float32)
    idx = make_index("cosinesimil", "seq_search", X)
    if D + 3 > 1024:
        run_case(idx, "cosinesimil", X, Q, 10, 0, monkeypatch)
    else:
        run_case(idx, "cosinesimil", X, Q, 10, 1, monkeypatch, gate="NMSLIB_GPU_COSC_FAST",
                 fast_tiles=1 if D + 3 <= 128 else 2)
    idx.close()


@pytest.mark.parametrize("D", [256, 257])
def test_dimension_threshold_l1(cache, monkeypatch, D):
    XW, QW = _wide(cache)
    X, Q = np.ascontiguousarray(XW[:, :D]), np.ascontiguousarray(QW[:, :D])
    idx = make_index("l1", "seq_search", X)
    run_case(idx, "l1", X, Q, 10, 6 if D <= 256 else 0, monkeypatch)
    idx.close()


def test_dimension_limit_negdotprod(cache, monkeypatch):
    XW, QW = _wide(cache)
    X, Q = np.ascontiguousarray(XW[:, :1024]), np.ascontiguousarray(QW[:, :1024])
    idx = make_index("negdotprod", "seq_search", X)
    run_case(idx, "negdotprod", X, Q, 10, 1, monkeypatch, fast_tiles=2)
    idx.close()


# ---- the adaptive kernel where it is the only chain ------------------------------------------------------------------
@pytest.fixture(scope="module")
def rows37():
    return refio.s_lowrank(70001, 37, 511), refio.s_lowrank(300, 37, 512)


@pytest.mark.parametrize("k", [10, 200])
@pytest.mark.parametrize("space", ["linf", "l1"])
def test_no_fast_path_at_size(cache, monkeypatch, rows37, space, k):
    """linf has no fast path, l1 with its gate closed neither: the direct selection kernel at a fast path's sizes"""
    X, Q = rows37
    idx, _ = cache.index(("x37", space), space, lambda: X)
    if space == "l1":
        monkeypatch.setenv("NMSLIB_GPU_L1_FAST", "0")
    got = run_case(idx, space, X, Q, k, 0, monkeypatch)
    if space == "l1" and k <= 128:
        monkeypatch.delenv("NMSLIB_GPU_L1_FAST")
        fast = idx.knnQueryBatch(Q, k)
        expect_path(idx, 6)
        same_bits(fast, got)


# ---- big-k at size ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["l2", "l2sqr_sift"])
def test_big_k_at_size(monkeypatch, space):
    """k = 700 over 70001 rows; 30 identical rows: among equal distances the position decides"""
    u8 = space == "l2sqr_sift"
    n, nq, k = 70001, 40, 700
    X = refio.s_sift_like(n, 521) if u8 else refio.s_lowrank(n, 32, 521)
    Q = refio.s_sift_like(nq, 522) if u8 else refio.s_lowrank(nq, 32, 522)
    X[40000:40030] = X[17]
    Q[3] = X[17]
    idx = make_index(space, "seq_search", X)
    ids, ds, cnt = run_case(idx, space, X, Q, k, 5, monkeypatch)
    assert ids[3, :31].tolist() == [17] + list(range(40000, 40030)) and (ds[3, :31] == 0).all()
    assert ds[3, 31] > 0
    idx.close()
