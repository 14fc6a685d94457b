"""bit_jaccard in numpy for tests/test_gpu_jaccard*.py: inputs of mixed densities, the distance from byte-table popcounts
in f32 arithmetic (one division, one subtraction; 0 for two empty codes), and the (distance, position) order."""
import numpy as np

from tests import scan_edge_cases as sec

_POP = np.array([bin(i).count("1") for i in range(256)], np.uint8)


def mixed_bits(rng, n, bits):
    """n codes whose densities are drawn per row from {0.02, 0.1, 0.5}, none of them empty"""
    dens = rng.choice(np.array([0.02, 0.1, 0.5], np.float32), size=n)
    B = (rng.random((n, bits), np.float32) < dens[:, None]).astype(np.uint8)
    B[np.arange(n), rng.integers(0, bits, n)] = 1
    return B


def distances(R, Q):
    """R [n][W], Q [nq][W] packed words -> f32 [nq][n]"""
    out = np.empty((len(Q), len(R)), np.float32)
    for qi in range(len(Q)):
        num = _POP[np.bitwise_and(R, Q[qi]).view(np.uint8)].sum(axis=1, dtype=np.int64)
        den = _POP[np.bitwise_or(R, Q[qi]).view(np.uint8)].sum(axis=1, dtype=np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            d = np.float32(1) - num.astype(np.float32) / den.astype(np.float32)
        out[qi] = np.where(den == 0, np.float32(0), d)
    return out


def check(got, d, queries, n, k):
    """rows `queries` of a k-NN batch over rows with ids ext_ids(n) against the distances d [len(queries)][n]"""
    ids, ds, cnt = got
    ext, pos = sec.ext_ids(n), np.arange(n)
    assert (cnt == min(k, n)).all()
    for row, q in zip(d, queries):
        o = np.lexsort((pos, row))[:k]
        np.testing.assert_array_equal(ds[q], row[o], err_msg=f"distances of query {q}")
        np.testing.assert_array_equal(ids[q], ext[o], err_msg=f"ids of query {q}")
