"""One chain over an HNSW index with deleted rows, written to an .npz: `python tests/delete_poison_child.py OUT.npz`.

tests/test_gpu_hnsw_delete.py starts this script with NMSLIB_GPU_POISON set (read once per process) and compares what it
wrote with the same work done in its own process: the filter's workspaces (the walk's max(ef, k) results and counts) and
the tombstone bitset must never be read where nothing wrote them."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run_all():
    """-> {name: array}: 3000 x 16 l2 rows, 30 % deleted in two calls, 70 queries at k = 10 on the LDS kernels (efSearch 4,
    40, 200), the HBM-array kernel and SearchOld (efSearch 1100), the fp16 walk, and after 300 rows more."""
    from tests import refio
    from tests.gpuutil import make_index
    X, Q = refio.s_lowrank(3300, 16, 901), refio.s_lowrank(70, 16, 902)
    dead = np.random.default_rng(903).permutation(3000)[:900].astype(np.int32)
    idx = make_index("l2", "hnsw", X[:3000], M=8, efConstruction=60, gpu_build=1, gpu_append=1)
    out = {}

    def keep(tag, ids, ds, cnt):
        out[tag + "/ids"], out[tag + "/dists"], out[tag + "/counts"] = ids, np.ascontiguousarray(ds).view(np.uint32), cnt

    assert idx.deleteIds(dead[:500]) == 500
    idx.setQueryTimeParams(efSearch=40)
    keep("first", *idx.knnQueryBatch(Q, 10))
    assert idx.deleteIds(dead[400:]) == 400
    for ef, algo in ((4, "hybrid"), (40, "hybrid"), (200, "hybrid"), (40, "old"), (1100, "v1merge"), (1100, "hybrid")):
        idx.setQueryTimeParams(efSearch=ef, algoType=algo)
        keep(f"ef{ef}_{algo}", *idx.knnQueryBatch(Q, 10))
    idx.setQueryTimeParams(efSearch=40, gpu_rows="f16")
    keep("f16", *idx.knnQueryBatch(Q, 10))
    idx.setQueryTimeParams(efSearch=40, gpu_rows="f32")
    idx.addDenseBatch(X[3000:], np.arange(3000, 3300, dtype=np.int32))
    keep("appended", *idx.knnQueryBatch(Q, 10))
    assert idx.stats()["rows_appended"] == 300 and idx.deletedRows() == 900
    idx.close()
    return out


def main():
    np.savez(sys.argv[1], **run_all())


if __name__ == "__main__":
    main()
