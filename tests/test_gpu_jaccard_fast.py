"""-m gpu: the bit_jaccard matrix-core scan (last_path 18) against numpy (tests/jaccard_ref.py) in
(distance, position) order: ids, distances and counts are equal, and equal to the bytes the scan kernel returns for the same
batch under NMSLIB_GPU_JAC_FAST=0.

n = 65 536 + 77 rows and 257 queries: the smallest admitted shape, with a partial last row block, a last split that is not
full and a last query tile of one query.  Rows 1 and n - 2 and query ZERO are empty; copies of queries stand at position 0,
at the last position and on both sides of a split boundary."""
import functools
import os

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import jaccard_ref
from tests import scan_edge_cases as sec

pytestmark = pytest.mark.gpu

N, NQ, ZERO = 65536 + 77, 257, 5
TILE = 64            # queries of a workgroup
BOUNDARY = 9216      # a first row of a split for every k below (rows_per_split is 1024: ham_fast_plan.hpp's rule)


def batch(idx, text, k, fast):
    os.environ["NMSLIB_GPU_JAC_FAST"] = "1" if fast else "0"
    try:
        got = idx.knnQueryBatch(text, k)
        return got, idx.stats()["last_path"]
    finally:
        del os.environ["NMSLIB_GPU_JAC_FAST"]


def make(bits, n, nq, plant=()):
    rng = np.random.default_rng(bits * 1000003 + n)
    B, Q = jaccard_ref.mixed_bits(rng, n, bits), jaccard_ref.mixed_bits(rng, nq, bits)
    B[1] = B[n - 2] = Q[ZERO] = 0
    for j, at in enumerate(plant):
        B[at] = Q[min(j, 2)]
    idx = nz.Index("bit_jaccard", "seq_search", data_type="ObjectAsString", dist_type="Float")
    idx.addStringBatch(sec.bits_text(B), ids=sec.ext_ids(n))
    idx.buildIndex()
    return idx, sec.pack_words(B), sec.pack_words(Q), sec.bits_text(Q)


@functools.lru_cache(maxsize=1)
def shared(bits):
    """one index and one reference per width: every query of the first and the last tile, every eighth in between"""
    idx, R, Qw, text = make(bits, N, NQ, plant=(0, N - 1, BOUNDARY - 1, BOUNDARY))
    last = (NQ - 1) // TILE * TILE
    queries = sorted(set(range(TILE)) | set(range(last, NQ)) | set(range(TILE, last, 8)))
    return idx, text, queries, jaccard_ref.distances(R, Qw[queries])


@pytest.mark.parametrize("bits,k", [(b, k) for b in (40, 256, 1000, 2048) for k in (1, 10, 16)] + [(2048, 32)])
def test_matrix_core_scan_equals_numpy_and_the_scan(bits, k):
    """W = 2 with a tail, 16-byte loads, a tail in the last of 32 words, the widest code; k up to the gate of each width
    (jac_fast_plan.hpp: 16 below 1024 bits, 32 from there on; cut from 64 by the measurement of DESIGN.md 6).  At 40 bits
    almost every rank is a tie, between equal pairs of counts and between different ones of one value (1/2, 2/4)"""
    idx, text, queries, d = shared(bits)
    got, path = batch(idx, text, k, True)
    assert path == 18
    jaccard_ref.check(got, d, queries, N, k)
    off, path = batch(idx, text, k, False)
    assert path == 0
    for a, b in zip(got, off):
        assert a.tobytes() == b.tobytes(), "the two scans differ"


@pytest.mark.parametrize("n,nq,k,bits,path", [(65536, 255, 10, 40, 0), (65535, 256, 10, 40, 0), (65536, 256, 17, 40, 0),
                                              (65536, 256, 17, 1023, 0), (65536, 256, 32, 1024, 18),
                                              (65536, 256, 33, 1024, 0), (65536, 256, 10, 2049, 0),
                                              (65536, 256, 10, 40, 18)])
def test_gate_edges(n, nq, k, bits, path):
    idx, R, Qw, text = make(bits, n, nq)
    got, took = batch(idx, text, k, True)
    idx.close()
    assert took == path
    queries = list(range(0, nq, 8)) + [nq - 1]
    jaccard_ref.check(got, jaccard_ref.distances(R, Qw[queries]), queries, n, k)
