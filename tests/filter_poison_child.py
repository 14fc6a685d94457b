"""Filtered HNSW batches written to an .npz: `python tests/filter_poison_child.py OUT.npz`.

tests/test_gpu_filter_hnsw.py starts this script with NMSLIB_GPU_POISON set (read once per process) and compares what it
wrote with the same work done in its own process: the compaction's masks, prefixes and list, the subset scan's keys and the
walk route's workspaces must never be read where nothing wrote them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run_all():
    """-> {name: array}: 3000 x 16 integer-grid l2 rows, 5 queries; subset-route filters of 0, 1, 33, 65 and 1000 rows at
    k = 10 (one of them after a delete inside its list), and a walk-route filter of half the rows."""
    from tests.gpuutil import make_index
    rng = np.random.default_rng(1301)
    X = rng.integers(-8, 9, (3000, 16)).astype(np.float32)
    Q = rng.integers(-8, 9, (5, 16)).astype(np.float32)
    idx = make_index("l2", "hnsw", X, M=8, efConstruction=40, gpu_build=1)
    idx.setQueryTimeParams(efSearch=64)
    out = {}

    def keep(tag, ids, ds, cnt):
        out[tag + "/ids"], out[tag + "/dists"], out[tag + "/counts"] = ids, np.ascontiguousarray(ds).view(np.uint32), cnt

    order = rng.permutation(3000)
    for m in (0, 1, 33, 65, 1000):
        mask = np.zeros(3000, bool)
        mask[order[:m]] = True
        flt = idx.makeFilter(mask, scan_rows=4096)
        keep(f"subset{m}", *idx.knnQueryBatchFiltered(flt, Q, 10))
        assert idx.stats()["last_path"] == 7
        if m == 65:
            assert idx.deleteIds(order[:3].astype(np.int32)) == 3
            keep("subset65_deleted", *idx.knnQueryBatchFiltered(flt, Q, 10))
        flt.close()
    mask = np.zeros(3000, bool)
    mask[order[:1500]] = True
    flt = idx.makeFilter(mask)
    keep("walk", *idx.knnQueryBatchFiltered(flt, Q, 10))
    assert idx.stats()["last_path"] == 4
    flt.close()
    idx.close()
    return out


def main():
    np.savez(sys.argv[1], **run_all())


if __name__ == "__main__":
    main()
