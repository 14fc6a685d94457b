"""nmslib_gpu_knn_query_batch_device on every chain of the engine: foreign streams, no counts pointer, element-aligned
pointers, the edges, batches in flight behind each other, and work of one index on two streams.

The reference answer of every check is the host ABI's nmslib_knn_query_batch on the same index; every comparison is bit
for bit on ids, distances (as uint32) and counts."""
import numpy as np
import pytest

import nmslib_zig_amd as nz

from . import refio
from .gpuutil import CNT_SENTINEL, ID_SENTINEL, enqueue_knn, expect_path, knn_on_stream, make_index, same_bits

pytestmark = pytest.mark.gpu


def _centred(n, seed):
    return (refio.s_lowrank(n, 32, seed) + np.float32(1.5)).astype(np.float32)


# chain -> (space, method, rows, queries, k, last_path, index parameters)
CHAINS = {
    "adaptive_f32": ("l2", "seq_search", lambda: refio.s_lowrank(3000, 24, 401), lambda: refio.s_lowrank(70, 24, 402), 10, 0, {}),
    "direct_linf": ("linf", "seq_search", lambda: refio.s_lowrank(3000, 24, 401), lambda: refio.s_lowrank(70, 24, 402), 10, 0, {}),
    "fast_f32": ("l2", "seq_search", lambda: refio.s_lowrank(65536, 32, 403), lambda: refio.s_lowrank(256, 32, 404), 10, 1, {}),
    "fast_cosc": ("cosinesimil", "seq_search", lambda: _centred(65536, 405), lambda: _centred(256, 406), 10, 1, {}),
    "adaptive_u8": ("l2sqr_sift", "seq_search", lambda: refio.s_sift_like(3000, 407), lambda: refio.s_sift_like(70, 408), 10, 2, {}),
    "fast_u8": ("l2sqr_sift", "seq_search", lambda: refio.s_sift_like(65536, 409), lambda: refio.s_sift_like(512, 410), 10, 3, {}),
    "bigk": ("l2", "seq_search", lambda: refio.s_lowrank(2000, 32, 411), lambda: refio.s_lowrank(24, 32, 412), 513, 5, {}),
    "fast_l1": ("l1", "seq_search", lambda: refio.s_lowrank(65536, 32, 413), lambda: refio.s_lowrank(256, 32, 414), 10, 6, {}),
    "hnsw_f32": ("l2", "hnsw", lambda: refio.s_lowrank(3000, 24, 415), lambda: refio.s_lowrank(70, 24, 416), 10, 4,
                 dict(M=8, efConstruction=100, indexThreadQty=1)),
    "hnsw_u8": ("l2sqr_sift", "hnsw", lambda: refio.s_sift_like(3000, 417), lambda: refio.s_sift_like(70, 418), 10, 4,
                dict(M=8, efConstruction=100, indexThreadQty=1)),
}


class _Chains:
    """The indexes of CHAINS, built when first asked for, with the host ABI's answer to their batch."""

    def __init__(self):
        self.made = {}

    def get(self, name):
        if name not in self.made:
            space, method, rows, queries, k, path, params = CHAINS[name]
            idx = make_index(space, method, rows(), **params)
            Q = queries()
            want = idx.knnQueryBatch(Q, k)
            expect_path(idx, path)
            assert (want[2] == k).all()
            self.made[name] = (idx, Q, k, path, want)
        return self.made[name]

    def close(self):
        for v in self.made.values():
            v[0].close()


@pytest.fixture(scope="module")
def chains():
    c = _Chains()
    yield c
    c.close()


@pytest.mark.parametrize("counts", [True, False], ids=["counts", "no_counts"])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_foreign_stream(chains, chain, counts):
    """A fresh side stream, which does not synchronise with the null stream or with the engine's own: the caller waits for
    that stream alone and reads the host ABI's answer.  Without a counts pointer nothing else is asked of the caller."""
    idx, Q, k, path, want = chains.get(chain)
    ids, ds, cnt = knn_on_stream(idx, Q, k, counts=counts)
    expect_path(idx, path)
    same_bits((ids, ds, cnt if counts else want[2]), want)
    if not counts:
        assert (cnt == CNT_SENTINEL).all()


@pytest.mark.parametrize("counts", [True, False], ids=["counts", "no_counts"])
@pytest.mark.parametrize("space,method", [("l2", "seq_search"), ("linf", "seq_search"), ("l2sqr_sift", "seq_search"),
                                          ("l2", "hnsw"), ("l2sqr_sift", "hnsw")])
def test_foreign_stream_unused_tail(space, method, counts):
    """k > n on five rows: the entries behind the five neighbours are -1 / +inf."""
    u8 = space == "l2sqr_sift"
    X = refio.s_sift_like(5, 421) if u8 else refio.s_gauss(5, 16, 421)
    idx = make_index(space, method, X, **(dict(M=8, efConstruction=100, indexThreadQty=1) if method == "hnsw" else {}))
    want = idx.knnQueryBatch(X[:3], 8)
    assert want[2].tolist() == [5, 5, 5]
    ids, ds, cnt = knn_on_stream(idx, X[:3], 8, counts=counts)
    assert (ids[:, 5:] == -1).all() and np.isposinf(ds[:, 5:]).all()
    same_bits((ids, ds, cnt if counts else want[2]), want)
    idx.close()


# What the stream-order test puts in front of the batch: MATMUL_REPS products of two MATMUL_N x MATMUL_N f32 matrices.
# Measured once with HIP events on an MI355X: the block takes 14.3 ms; one batch of CHAINS takes 0.05 .. 0.89 ms (the
# slowest: fast_l1 0.87 .. 0.89 ms, bigk 0.61 .. 0.72 ms, hnsw_u8 0.61 ms), so the block is 16 times the slowest batch.
MATMUL_N, MATMUL_REPS = 8192, 2


@pytest.mark.parametrize("chain", list(CHAINS))
def test_stream_order_only(chains, chain):
    """The query buffer holds NaN until a copy that sits on the side stream behind a long matmul, and holds NaN again
    right behind the call; the outputs get their sentinels on that stream too.  A kernel that the library puts on any
    other stream reads NaN queries, or has its output overwritten by the sentinel fill: the answer would differ.

    The matmul block in front runs for 16 times the slowest batch (see MATMUL_N)."""
    import torch
    idx, Q, k, path, want = chains.get(chain)
    a = torch.ones((MATMUL_N, MATMUL_N), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def before(qbuf):
        qbuf.fill_(float("nan") if qbuf.dtype == torch.float32 else 255)
        torch.cuda.synchronize()
        for _ in range(MATMUL_REPS):
            torch.matmul(a, a)

    def after(qbuf):
        qbuf.fill_(float("nan") if qbuf.dtype == torch.float32 else 255)

    got = knn_on_stream(idx, Q, k, before=before, after=after)
    same_bits(got, want)


@pytest.mark.parametrize("q_off,out_off", [(1, 0), (2, 0), (3, 0), (0, 1), (3, 1)])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_element_aligned_pointers(chains, chain, q_off, out_off):
    """Queries 1, 2, 3 elements past a 256-byte boundary (uint8 queries: bytes, the odd-address branch of the uint8 fast
    path's preparation kernel; the HNSW search reads the caller's buffer directly), outputs one element past theirs: the
    aligned call's answer, and nothing written around the outputs."""
    idx, Q, k, path, want = chains.get(chain)
    got = knn_on_stream(idx, Q, k, q_off=q_off, out_off=out_off)
    expect_path(idx, path)
    same_bits(got, want)


def test_edges_through_the_device_entry(chains):
    idx, Q, k, path, want = chains.get("adaptive_f32")
    # no queries: success, nothing written (the helper looks at the sentinels around the empty outputs)
    ids, ds, cnt = knn_on_stream(idx, Q[:0], k)
    assert ids.shape == (0, k) and cnt.size == 0
    # a wrong elem_count: QUERY_EXECUTION_FAILED
    with pytest.raises(nz.NmslibError) as e:
        knn_on_stream(idx, np.zeros((4, Q.shape[1] + 1), np.float32), k)
    assert e.value.code == 9
    # ... and the index still answers
    same_bits(knn_on_stream(idx, Q, k), want)
    # an index without rows
    for space in ("l2", "l2sqr_sift"):
        u8 = space == "l2sqr_sift"
        empty = nz.Index(space, "seq_search", data_type="DenseUInt8Vector" if u8 else "DenseVector",
                         dist_type="Int" if u8 else "Float")
        empty.buildIndex()
        q = np.zeros((3, 128), np.uint8 if u8 else np.float32)
        for counts in (True, False):
            ids, ds, cnt = knn_on_stream(empty, q, 4, counts=counts)
            assert (ids == -1).all() and np.isposinf(ds).all()
            assert (cnt == (0 if counts else CNT_SENTINEL)).all()
        empty.close()


def test_no_queries_leaves_the_sentinels(chains):
    """query_count == 0 with non-empty output buffers: success, and the buffers keep what the caller put there."""
    import torch
    idx = chains.get("fast_f32")[0]
    out = torch.full((64,), ID_SENTINEL, dtype=torch.int32, device="cuda")
    d = torch.full((64,), float("nan"), dtype=torch.float32, device="cuda")
    c = torch.full((8,), CNT_SENTINEL, dtype=torch.int32, device="cuda")
    q = torch.zeros((32,), dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    idx.knn_device(q.data_ptr(), 0, 32, 8, out.data_ptr(), d.data_ptr(), c.data_ptr(), s.cuda_stream)
    s.synchronize()
    assert (out.cpu().numpy() == ID_SENTINEL).all() and np.isnan(d.cpu().numpy()).all() and (c.cpu().numpy() == CNT_SENTINEL).all()


@pytest.mark.parametrize("counts", [True, False], ids=["counts", "no_counts"])
@pytest.mark.parametrize("chain", ["fast_f32", "fast_u8"])
def test_second_slice_writes_at_its_offset(chains, chain, counts):
    """32768 + 40 queries: the second slice's ids, distances and counts land behind the first slice's."""
    idx, Q0, _, path, _ = chains.get(chain)
    nq, k = 32768 + 40, 5
    Q = refio.s_sift_like(nq, 431) if chain == "fast_u8" else refio.s_lowrank(nq, 32, 431)
    want = idx.knnQueryBatch(Q, k)
    ids, ds, cnt = knn_on_stream(idx, Q, k, counts=counts)
    same_bits((ids, ds, cnt if counts else want[2]), want)
    if not counts:
        assert (cnt == CNT_SENTINEL).all()
    # the 40 queries of the second slice, alone: the same plan, the same bits
    tail = idx.knnQueryBatch(Q[32768:], k)
    same_bits((ids[32768:], ds[32768:], want[2][32768:]), tail)
    # ... and the head of the first slice in a batch of its own through the fast path
    head = idx.knnQueryBatch(Q[:1024], k)
    expect_path(idx, path)
    same_bits((ids[:1024], ds[:1024], want[2][:1024]), head)


def test_batches_back_to_back_on_one_stream(chains):
    """Three batches of different chains and sizes enqueued on one stream with no host synchronisation between them share
    the index's workspaces in stream order: each answer is the one computed alone."""
    import torch
    idx = chains.get("fast_f32")[0]
    QA, QB, QC = refio.s_lowrank(1024, 32, 441), refio.s_lowrank(64, 32, 442), refio.s_lowrank(256, 32, 443)
    batches = ((QA, 10, 1), (QB, 10, 0), (QC, 37, 1))
    want = []
    for Q, k, path in batches:         # also the warm-up pass: every workspace has its size
        want.append(idx.knnQueryBatch(Q, k))
        expect_path(idx, path)
    s = torch.cuda.Stream()
    for Q, k, _ in batches:
        knn_on_stream(idx, Q, k, stream=s)
    calls = [enqueue_knn(idx, Q, k, s) for Q, k, _ in batches]
    s.synchronize()
    for call, w in zip(calls, want):
        same_bits(call.result(), w)


@pytest.fixture(scope="module")
def two_stream_index():
    X = refio.s_lowrank(70001, 128, 451)
    QL, QS = refio.s_lowrank(32768, 128, 452), refio.s_lowrank(64, 128, 453)
    idx = make_index("l2", "seq_search", X)
    want_l = idx.knnQueryBatch(QL, 10)
    expect_path(idx, 1)
    want_s = idx.knnQueryBatch(QS, 10)
    expect_path(idx, 0)
    yield idx, QL, QS, want_l, want_s
    idx.close()


@pytest.mark.parametrize("second", ["host_abi", "device_on_another_stream"])
def test_one_index_on_two_streams(two_stream_index, second):
    """Batches of one index are executed in the order of the calls, whatever streams they are given.  A large device
    batch on a side stream and, with no host synchronisation in between, a small batch through the host ABI (the
    engine's own stream) or on a second side stream: both use the index's workspaces, so the second has to wait for the
    first.  A screen, like test_fast_paths_are_deterministic: 20 rounds, every answer of every round is the reference."""
    import torch
    idx, QL, QS, want_l, want_s = two_stream_index
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for _ in range(20):
        big = enqueue_knn(idx, QL, 10, s1)
        if second == "host_abi":
            small = idx.knnQueryBatch(QS, 10)
        else:
            call = enqueue_knn(idx, QS, 10, s2)
            s2.synchronize()
            small = call.result()
        s1.synchronize()
        same_bits(small, want_s)
        same_bits(big.result(), want_l)
