"""Helpers for the -m gpu tests: every query goes through the C ABI of libnmslib_c.so."""
import ctypes as C

import numpy as np

import nmslib_zig_amd as nz

FLOAT_SPACES = ("l2", "l1", "linf", "cosinesimil", "angulardist", "negdotprod")


def make_index(space, method, base, ids=None, **index_params):
    u8 = space == "l2sqr_sift"
    idx = nz.Index(space, method, data_type="DenseUInt8Vector" if u8 else "DenseVector",
                   dist_type="Int" if u8 else "Float")
    if u8:
        idx.addUInt8Batch(base, ids)
    else:
        idx.addDenseBatch(base, ids)
    idx.buildIndex(**index_params)
    return idx


def close_rel(a, b, rtol=1e-5, atol=1e-6):
    """north_star's float bar: distances within 1e-5 relative of the reference formula."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= rtol * np.abs(b) + atol))


def ids_match_modulo_ties(got_ids, got_d, want_ids, want_d):
    """ids identical except inside equal-distance groups."""
    for q in range(got_ids.shape[0]):
        for dv in np.unique(want_d[q]):
            m = want_d[q] == dv
            if set(got_ids[q][m].tolist()) != set(want_ids[q][m].tolist()):
                if m.sum() == 1 or not np.isclose(got_d[q][m], dv).all():
                    return False
                # a tie group cut by rank k may legitimately hold other members
                if not (want_d[q][-1] == dv):
                    return False
    return True


ULP1 = 2.0 ** -23   # spacing of float32 at 1.0


def sim_close(sim_got, sim_want, ulps=4):
    """Similarities (a dot product of unit vectors, |s| <= 1) within `ulps` float32 steps of each other: the quantity
    the reference computes accurately; 1 - s and acos(s) amplify its last bits when s is near 1."""
    a, b = np.asarray(sim_got, np.float64), np.asarray(sim_want, np.float64)
    return bool(np.all(np.abs(a - b) <= ulps * ULP1))


def ids_match_modulo_near_ties(got_ids, want_ids, want_key, eps, got_key=None):
    """ids identical at every rank whose reference key is separated from both neighbours by more than eps (callable of
    the key -> absolute resolution); inside a run of keys closer than that the SET must agree, except for a run
    that reaches rank k (it may continue past the cut).  Returns the list of offending (query, rank)."""
    bad = []
    for q in range(want_ids.shape[0]):
        key = np.asarray(want_key[q], np.float64)
        k = len(key)
        start = 0
        for i in range(1, k + 1):
            if i < k and abs(key[i] - key[i - 1]) <= eps(max(abs(key[i]), abs(key[i - 1]))):
                continue
            run = slice(start, i)
            if i - start == 1:
                if got_ids[q][start] != want_ids[q][start]:
                    # (the last rank may be a near-tie with the reference's unseen rank k+1: same key, other row)
                    last_tie = (i == k and got_key is not None and
                                abs(float(got_key[q][start]) - key[start]) <= eps(abs(key[start])))
                    if not last_tie:
                        bad.append((q, start))
            elif i < k and set(got_ids[q][run].tolist()) != set(want_ids[q][run].tolist()):
                bad.append((q, start))
            start = i
    return bad


# ---- the device-resident entry (include/nmslib_gpu.h) on a stream of the caller's choice ----------------------------
ID_SENTINEL = 0x5A5A5A5A     # what the output buffers hold before a call: ids, counts, and NaN distances
CNT_SENTINEL = -7
_GUARD = 64                  # sentinel elements kept behind every output (and the `off` elements in front of it)


def _offset_buffer(n, dtype, off):
    """-> (raw, view): `view` holds n elements and starts `off` ELEMENTS past the 256-byte-aligned start of `raw`, which
    goes on for _GUARD elements behind the view."""
    import torch
    raw = torch.empty(off + n + _GUARD, dtype=dtype, device="cuda")
    assert raw.data_ptr() % 256 == 0, "the allocator returned a block off a 256-byte boundary"
    return raw, raw[off:off + n]


class DeviceCall:
    """One batch enqueued by enqueue_knn: the buffers stay alive here; result() reads them after the stream was waited for."""

    def __init__(self, nq, k, qraw, ids, ds, cnt, off):
        self.nq, self.k, self.qraw, self.ids, self.ds, self.cnt, self.off = nq, k, qraw, ids, ds, cnt, off

    def result(self):
        """-> ids [nq, k] int32, dists [nq, k] float32, counts [nq] int32; the elements around the outputs still hold
        their sentinels (a kernel that writes outside what it was given fails here)."""
        out = []
        for raw, sentinel in ((self.ids, ID_SENTINEL), (self.ds, None), (self.cnt, CNT_SENTINEL)):
            h = raw.cpu().numpy()
            n = len(h) - self.off - _GUARD
            guard = np.r_[h[:self.off], h[self.off + n:]]
            if sentinel is None:
                assert np.isnan(guard).all(), "distances were written outside the output buffer"
            else:
                assert (guard == sentinel).all(), "ids / counts were written outside the output buffer"
            out.append(h[self.off:self.off + n])
        return out[0].reshape(self.nq, self.k), out[1].reshape(self.nq, self.k), out[2]


def enqueue_knn(idx, Q, k, stream, counts=True, q_off=0, out_off=0, before=None, after=None):
    """What knn_on_stream enqueues, without waiting for `stream`.  The queries are staged in HBM first (on torch's
    current stream, waited for), so that everything put on `stream` is device work in stream order: before(qbuf), the
    copy of the queries into qbuf, the sentinel fills, the call, after(qbuf)."""
    import torch
    Q = np.ascontiguousarray(Q)
    nq, qdim = Q.shape
    tdt = torch.uint8 if Q.dtype == np.uint8 else torch.float32
    staged = torch.from_numpy(Q).cuda().reshape(-1)
    torch.cuda.current_stream().synchronize()
    qraw, qbuf = _offset_buffer(nq * qdim, tdt, q_off)
    ids_raw, ids = _offset_buffer(nq * k, torch.int32, out_off)
    ds_raw, ds = _offset_buffer(nq * k, torch.float32, out_off)
    cnt_raw, cnt = _offset_buffer(nq, torch.int32, out_off)
    with torch.cuda.stream(stream):
        if before is not None:
            before(qbuf)
        qbuf.copy_(staged)
        ids_raw.fill_(ID_SENTINEL)
        ds_raw.fill_(float("nan"))
        cnt_raw.fill_(CNT_SENTINEL)
        # (addresses from the allocations: an empty view has no data pointer)
        at = lambda raw, off: raw.data_ptr() + off * raw.element_size()   # noqa: E731
        idx.knn_device(at(qraw, q_off), nq, qdim, k, at(ids_raw, out_off), at(ds_raw, out_off),
                       at(cnt_raw, out_off) if counts else None, stream.cuda_stream)
        if after is not None:
            after(qbuf)
    return DeviceCall(nq, k, (qraw, staged), ids_raw, ds_raw, cnt_raw, out_off)


def knn_on_stream(idx, Q, k, stream=None, counts=True, q_off=0, out_off=0, before=None, after=None):
    """One batch through nmslib_gpu_knn_query_batch_device on `stream` (None: a fresh torch.cuda.Stream(), which does
    not synchronise with the null stream).  The queries lie q_off ELEMENTS past a 256-byte-aligned allocation, ids /
    distances / counts out_off elements past theirs; before the call they are filled, on the stream, with ID_SENTINEL /
    NaN / CNT_SENTINEL.  counts=False passes d_counts = NULL (the counts come back as sentinels).  before(qbuf) /
    after(qbuf) run on the stream ahead of the upload and right behind the call.  The stream is waited for.
    -> ids, dists, counts (numpy)"""
    import torch
    if stream is None:
        stream = torch.cuda.Stream()
    call = enqueue_knn(idx, Q, k, stream, counts, q_off, out_off, before, after)
    stream.synchronize()
    return call.result()


def range_fill_guarded(idx, query, radius, capacity, declared=None):
    """One nmslib_range_query_fill whose id and distance buffers go on for _GUARD sentinel elements (ID_SENTINEL / NaN, as
    DeviceCall.result has them) behind their `capacity` elements: a write past the end fails here.  `declared` is what
    Result.capacity says when it is not the buffers' real size.  -> (ids, dists), the `size` elements the call reports"""
    q, qsz, ne = idx._query(query)
    ids = np.full(capacity + _GUARD, ID_SENTINEL, np.int32)
    ds = np.full(capacity + _GUARD, np.nan, np.float32)
    r = nz.Result(ids.ctypes.data_as(C.POINTER(C.c_int32)), ds.ctypes.data_as(C.POINTER(C.c_float)), 0,
                  capacity if declared is None else declared)
    nz._check(nz.lib().nmslib_range_query_fill(idx.h, q.ctypes.data, qsz, float(radius), C.byref(r), ne), idx.alloc)
    assert r.size <= capacity, f"size {r.size} beyond the buffer's {capacity} elements"
    assert (ids[capacity:] == ID_SENTINEL).all(), "ids were written outside the output buffer"
    assert np.isnan(ds[capacity:]).all(), "distances were written outside the output buffer"
    return ids[:r.size].copy(), ds[:r.size].copy()


def expect_path(idx, code, **more):
    """The chain the last batch took (nmslib_gpu_stats_t.last_path), and any other statistic given by name."""
    st = idx.stats()
    assert st["last_path"] == code, f"last_path {st['last_path']}, expected {code}: {st}"
    for name, want in more.items():
        assert st[name] == want, f"{name} {st[name]}, expected {want}: {st}"
    return st


def same_bits(got, want):
    """ids, distances (as uint32) and counts of two answers are identical."""
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(np.ascontiguousarray(got[1]).view(np.uint32), np.ascontiguousarray(want[1]).view(np.uint32))
    np.testing.assert_array_equal(got[2], want[2])
