"""One chain over an HNSW index that is consolidated, written to an .npz: `python tests/consolidate_poison_child.py OUT.npz`.

tests/test_gpu_hnsw_consolidate.py starts this script with NMSLIB_GPU_POISON set (read once per process) and compares
what it wrote with the same work done in its own process: the worklist, the pool and the buffers the compaction fills must
never be read where nothing wrote them."""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run_all():
    """-> {name: array}: 3000 x 16 l2 rows on a GPU-built graph with an fp16 copy, 30 % deleted and consolidated, the saved
    files' bytes, 70 queries at k = 10 (efSearch 4, 40, 200, SearchOld, the fp16 walk), then 10 % more deleted, consolidated,
    300 rows appended, and the files and a batch again."""
    from tests import refio
    from tests.gpuutil import make_index
    X, Q = refio.s_lowrank(3300, 16, 911), refio.s_lowrank(70, 16, 912)
    perm = np.random.default_rng(913).permutation(3000).astype(np.int32)
    idx = make_index("l2", "hnsw", X[:3000], M=8, efConstruction=60, gpu_build=1, gpu_append=1, gpu_rows="f16")
    out = {}

    def keep(tag, ids, ds, cnt):
        out[tag + "/ids"], out[tag + "/dists"], out[tag + "/counts"] = ids, np.ascontiguousarray(ds).view(np.uint32), cnt

    def files(tag):
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "c.idx")
            idx.save(path, save_data=True)
            out[tag + "/idx"] = np.fromfile(path, np.uint8)
            out[tag + "/dat"] = np.fromfile(path + ".dat", np.uint8)

    assert idx.deleteIds(perm[:900]) == 900
    out["first/counts"] = np.array(idx.consolidate(), np.int64)
    files("first")
    for ef, params in ((4, {}), (40, {}), (200, {}), (40, dict(algoType="old")), (40, dict(gpu_rows="f16"))):
        idx.setQueryTimeParams(efSearch=ef, **params)
        keep(f"ef{ef}_{'_'.join(params.values())}", *idx.knnQueryBatch(Q, 10))
    idx.setQueryTimeParams(efSearch=40, gpu_rows="f32")
    assert idx.deleteIds(perm[900:1200]) == 300
    out["second/counts"] = np.array(idx.consolidate(), np.int64)
    idx.addDenseBatch(X[3000:], np.arange(3000, 3300, dtype=np.int32))
    keep("appended", *idx.knnQueryBatch(Q, 10))
    assert idx.stats()["rows_appended"] == 300 and idx.deletedRows() == 0 and idx.dataQty() == 2100
    files("second")
    idx.close()
    return out


def main():
    np.savez(sys.argv[1], **run_all())


if __name__ == "__main__":
    main()
