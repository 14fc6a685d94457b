"""-m gpu: bit_jaccard on the exact scan (last_path 0), range search and get_distance against numpy (tests/jaccard_ref.py).
Both sides are correctly rounded f32: ids, distances and counts are equal.

n = 2 * 4096 + 300 rows and 9 queries: three splits, two query tiles, the second holding one query.  Rows 0 and n - 1 are
empty, row COPY is query 0, query ZERO is empty: its answer is the two empty rows at distance 0, then distance 1 for every
other row, ranked by position alone."""
import functools

import numpy as np
import pytest

import nmslib_zig_amd as nz
from tests import jaccard_ref
from tests import scan_edge_cases as sec

pytestmark = pytest.mark.gpu

N, NQ, COPY, ZERO = 2 * 4096 + 300, 9, 5000, 3


@functools.lru_cache(maxsize=None)
def shared(bits):
    rng = np.random.default_rng(bits)
    B, Q = jaccard_ref.mixed_bits(rng, N, bits), jaccard_ref.mixed_bits(rng, NQ, bits)
    B[0] = B[N - 1] = Q[ZERO] = 0
    B[COPY] = Q[0]
    idx = nz.Index("bit_jaccard", "seq_search", data_type="ObjectAsString", dist_type="Float")
    idx.addStringBatch(sec.bits_text(B), ids=sec.ext_ids(N))
    idx.buildIndex()
    R = sec.pack_words(B)
    return idx, R, sec.bits_text(B), sec.bits_text(Q), jaccard_ref.distances(R, sec.pack_words(Q))


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("bits", [40, 129, 1024])
def test_scan_equals_numpy(bits, k):
    """one word and a tail, W % 4 != 0, 16-byte loads"""
    idx, _, _, qtext, d = shared(bits)
    got = idx.knnQueryBatch(qtext, k)
    assert idx.stats()["last_path"] == 0
    jaccard_ref.check(got, d, range(NQ), N, k)
    ext = sec.ext_ids(N)
    assert got[1][0, 0] == 0          # (row COPY, or an equal row before it)
    want = [ext[0], ext[N - 1]] + ext[1:9].tolist()
    assert got[0][ZERO].tolist() == want[:k] and got[1][ZERO].tolist() == ([0.0, 0.0] + [1.0] * 8)[:k]


@pytest.mark.parametrize("bits", [40, 129, 1024])
def test_range_at_a_returned_distance(bits):
    """the radius is one of the query's own distances: rows AT it are returned, in insertion order"""
    idx, _, _, qtext, d = shared(bits)
    for q in (0, ZERO, NQ - 1):
        radius = np.sort(d[q])[9]
        ids, ds = idx.rangeQueryFill(qtext[q], float(radius), N)
        inside = np.nonzero(d[q] <= radius)[0]
        assert len(inside) >= 10
        np.testing.assert_array_equal(ids, sec.ext_ids(N)[inside])
        np.testing.assert_array_equal(ds, d[q][inside])


@pytest.mark.parametrize("bits", [40, 129, 1024])
def test_get_distance_equals_the_scan_value(bits):
    """rows as queries: get_distance(a, b) is the distance the scan returns for b, bit for bit, and the range kernel's.
    Row 0 is empty: its list holds the other empty row (distance 0) and non-empty ones (distance 1)"""
    idx, R, rtext, _, _ = shared(bits)
    rows = [0, 1, COPY, 4097]
    ids, ds, _ = idx.knnQueryBatch([rtext[a] for a in rows], 10)
    for a, id_row, d_row in zip(rows, ids, ds):
        _, every = idx.rangeQueryFill(rtext[a], 1.0, N)      # every row is within 1: the distances in insertion order
        for b, d in zip((N - 1 - id_row).tolist(), d_row):   # ext_ids run against the positions
            want = jaccard_ref.distances(R[b:b + 1], R[a:a + 1])[0, 0]
            got = np.float32(idx.getDistance(a, b))
            assert got.tobytes() == d.tobytes() == every[b].tobytes() == want.tobytes(), (a, b, got, d, every[b], want)
    assert (N - 1 - ids[0, :3]).tolist() == [0, N - 1, 1] and ds[0, :3].tolist() == [0.0, 0.0, 1.0]


def test_big_k_runs_the_one_query_tile():
    """k = 769: the scan's plan drops to one query per workgroup (jac_knn_kernel<1>), lists of 769 keys"""
    idx, _, _, qtext, d = shared(129)
    got = idx.knnQueryBatch(qtext, 769)
    assert idx.stats()["last_path"] == 0
    jaccard_ref.check(got, d, range(NQ), N, 769)
