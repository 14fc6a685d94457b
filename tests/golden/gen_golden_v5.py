#!/usr/bin/env python3
"""Fifth fixture file from the REAL reference (oracle/_ref): the cases of tests/test_oracle_vs_reference.py.

    make -C oracle ref && python3 tests/golden/gen_golden_v5.py

  * HNSW (M=12, efConstruction=80, single thread, efSearch=64) over S-lowrank rows for six (space, D): the flattened
    graph of the reference's saved index (level-0 lists, upper-list offsets and links) and its k=10 results;
  * l2sqr_sift over S-sift-like rows: seq_search at k=50 (ids, distances) and HNSW (M=8, efConstruction=60,
    efSearch=80) at k=50 (distances, distance computations per query).
Only the reference's outputs are stored; the inputs are regenerated from their seeds and pinned by SHA-256.
"""
import hashlib
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import refio  # noqa: E402

HNSW_CASES = [("l2", 128), ("l2", 50), ("cosinesimil", 96), ("negdotprod", 64), ("l1", 40), ("linf", 40)]


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8).copy()


def inputs_hnsw(D):
    return refio.s_lowrank(1500, D, 1), refio.s_lowrank(24, D, 2)


def inputs_u8():
    return refio.s_sift_like(3000, 7), refio.s_sift_like(16, 8)


def main():
    assert refio.HAVE_REF, "build oracle/_ref first: make -C oracle ref"
    out = {}
    tmp = tempfile.mkdtemp()
    for space, D in HNSW_CASES:
        tag = f"{space}_{D}"
        X, Y = inputs_hnsw(D)
        out[f"{tag}_base_sha"], out[f"{tag}_queries_sha"] = sha(X), sha(Y)
        path = os.path.join(tmp, tag)
        ids, d, _, _, _ = refio.run_ref_driver(space, "hnsw", X, Y, 10, "M=12,efConstruction=80,indexThreadQty=1",
                                               "efSearch=64", save=path)
        P = refio.parse_optimized_index(path)
        for key in ("links0", "up_off", "up_links"):
            out[f"{tag}_{key}"] = P[key]
        out[f"{tag}_ids"], out[f"{tag}_dists"] = ids, d
    X, Y = inputs_u8()
    out["u8_base_sha"], out["u8_queries_sha"] = sha(X), sha(Y)
    ids, d, _, _, _ = refio.run_ref_driver("l2sqr_sift", "seq_search", X, Y, 50)
    out["u8_seq_ids"], out["u8_seq_dists"] = ids, d
    _, d, _, ndc, _ = refio.run_ref_driver("l2sqr_sift", "hnsw", X, Y, 50, "M=8,efConstruction=60,indexThreadQty=1",
                                           "efSearch=80")
    out["u8_hnsw_dists"], out["u8_hnsw_ndc"] = d, ndc
    np.savez_compressed(os.path.join(HERE, "golden_v5.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
