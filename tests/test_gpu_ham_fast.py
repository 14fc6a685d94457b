"""-m gpu: the bit_hamming matrix-core scan (last_path 17) against popcount of XOR in numpy, in
(distance, position) order.  Integer arithmetic: ids, distances and counts are equal, and equal to the bytes the
XOR-popcount kernel returns for the same batch under NMSLIB_GPU_HAM_FAST=0.

n = 65 536 + 77 rows and 257 queries: the smallest admitted shape, with a partial last row block, a last split that is
not full and a last query tile of one query.  External ids run against the positions."""
import functools
import os

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import scan_edge_cases as sec

pytestmark = pytest.mark.gpu

N, NQ = 65536 + 77, 257
TILE = 64            # queries of a workgroup (ham_fast_plan.hpp: 32 * kQueryGroups)
BOUNDARY = 9216      # a first row of a split for every k below (rows_per_split is 1024 or 1152)


def rows_per_split(n, nq, k):
    """ham_fast_plan.hpp restated"""
    ntiles = -(-nq // TILE)
    want = min(max(-(-4096 // ntiles), -(-n // 65536)), 8192 // k)
    return -(-max(-(-n // want), 1024) // 128) * 128


def batch(idx, text, k, fast):
    os.environ["NMSLIB_GPU_HAM_FAST"] = "1" if fast else "0"
    try:
        got = idx.knnQueryBatch(text, k)
        return got, idx.stats()["last_path"]
    finally:
        del os.environ["NMSLIB_GPU_HAM_FAST"]


def check(got, d, queries, n, k):
    """rows `queries` of the batch against the distances d [len(queries)][n]"""
    ids, ds, cnt = got
    ext, pos = sec.ext_ids(n), np.arange(n)
    assert (cnt == min(k, n)).all()
    for row, q in zip(d, queries):
        o = np.lexsort((pos, row))[:k]
        np.testing.assert_array_equal(ds[q], row[o].astype(np.float32), err_msg=f"distances of query {q}")
        np.testing.assert_array_equal(ids[q], ext[o], err_msg=f"ids of query {q}")


def make(bits, n, nq, plant=()):
    rng = np.random.default_rng(bits * 1000003 + n)
    B, Q = rng.integers(0, 2, (n, bits), np.uint8), rng.integers(0, 2, (nq, bits), np.uint8)
    for j, at in enumerate(plant):   # copies of queries 0.. : position 0, the last position, both sides of a boundary
        B[at] = Q[min(j, 2)]
    idx = nz.Index("bit_hamming", "seq_search", data_type="ObjectAsString", dist_type="Int")
    idx.addStringBatch(sec.bits_text(B), ids=sec.ext_ids(n))
    idx.buildIndex()
    return idx, sec.pack_words(B), sec.pack_words(Q), sec.bits_text(Q)


@functools.lru_cache(maxsize=1)
def shared(bits):
    """one index and one reference per width: every query of the first and the last tile, every eighth in between"""
    idx, R, Qw, text = make(bits, N, NQ, plant=(0, N - 1, BOUNDARY - 1, BOUNDARY))
    last = (NQ - 1) // TILE * TILE
    queries = sorted(set(range(TILE)) | set(range(last, NQ)) | set(range(TILE, last, 8)))
    return idx, text, queries, sec.ham_distances(R, Qw[queries])


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("bits", [40, 256, 1000, 1024])
def test_matrix_core_scan_equals_xor_popcount(bits, k):
    """W = 2 with a tail, 16-byte loads, a tail in the last of 32 words, a full word count.  At 40 bits 65 613 rows share
    41 distances: almost every rank is a tie decided by position"""
    idx, text, queries, d = shared(bits)
    assert BOUNDARY % rows_per_split(N, NQ, k) == 0
    got, path = batch(idx, text, k, True)
    assert path == 17
    check(got, d, queries, N, k)
    off, path = batch(idx, text, k, False)
    assert path == 0
    for a, b in zip(got, off):
        assert a.tobytes() == b.tobytes(), "the two scans differ"


@pytest.mark.parametrize("n,nq,k,bits,path", [(65536, 255, 10, 40, 0), (65535, 256, 10, 40, 0), (65536, 256, 129, 40, 0),
                                              (65536, 256, 10, 1025, 0), (65536, 256, 10, 40, 17)])
def test_gate_edges(n, nq, k, bits, path):
    idx, R, Qw, text = make(bits, n, nq)
    got, took = batch(idx, text, k, True)
    idx.close()
    assert took == path
    queries = list(range(0, nq, 8)) + [nq - 1]
    check(got, sec.ham_distances(R, Qw[queries]), queries, n, k)
