"""The CPU oracle against the real reference on larger/randomised versions of the golden checks.  The reference's
outputs are stored in tests/golden/golden_v5.npz (gen_golden_v5.py); the inputs are regenerated from their seeds."""
import os

import numpy as np
import pytest

from tests import orc
from tests.golden.gen_golden_v5 import HNSW_CASES, inputs_hnsw, inputs_u8, sha

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_v5.npz")


@pytest.fixture(scope="module")
def g5():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def pinned(g5, tag, X, Y):
    assert np.array_equal(sha(X), g5[f"{tag}_base_sha"]), f"regenerated base rows of {tag} differ from the fixture's"
    assert np.array_equal(sha(Y), g5[f"{tag}_queries_sha"]), f"regenerated queries of {tag} differ from the fixture's"
    return X, Y


@pytest.mark.parametrize("space,D", HNSW_CASES)
def test_build_and_search_match_reference(g5, space, D):
    tag = f"{space}_{D}"
    X, Y = pinned(g5, tag, *inputs_hnsw(D))
    rid, rd = g5[f"{tag}_ids"], g5[f"{tag}_dists"]
    g = orc.HnswGraph.build(space, X, 12, 80)
    np.testing.assert_array_equal(g.links0(), g5[f"{tag}_links0"])
    off, up = g.flat_upper()
    np.testing.assert_array_equal(off, g5[f"{tag}_up_off"])
    np.testing.assert_array_equal(up, g5[f"{tag}_up_links"])
    pos, dist, _, _, _ = g.search(Y, 10, 64)
    np.testing.assert_array_equal(pos, rid)
    assert np.all(np.abs(dist - rd) <= 1e-5 * np.abs(rd) + 1e-6)


def test_u8_seq_and_hnsw_match_reference(g5):
    X, Y = pinned(g5, "u8", *inputs_u8())
    pos, dist, _ = orc.seq_search("l2sqr_sift", X, Y, 50)
    np.testing.assert_array_equal(dist, g5["u8_seq_dists"])
    np.testing.assert_array_equal(pos, g5["u8_seq_ids"])
    g = orc.HnswGraph.build("l2sqr_sift", X, 8, 60)
    pos, dist, _, ndc, _ = g.search(Y, 50, 80, optimized=False)
    np.testing.assert_array_equal(dist, g5["u8_hnsw_dists"])
    np.testing.assert_array_equal(ndc, g5["u8_hnsw_ndc"])
