"""One batch through every chain of the engine, written to an .npz: `python tests/poison_child.py OUT.npz`.

tests/test_gpu_poison.py starts this script with NMSLIB_GPU_POISON set (the variable is read once per process, so only a
fresh process can turn it on) and compares what it wrote with the same work done in the test's own process: a workspace
word that a kernel reads before any kernel wrote it shows up as a difference."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def run_all():
    """-> {name: array}: per chain of test_gpu_device_entry.CHAINS the host ABI's answer and the device entry's on a side
    stream without a counts pointer; a dense range query per element type; HNSW batches on the LDS visited table
    (default efSearch), on the per-query bitset in HBM (efSearch=800) and through SearchOld (efSearch=1200)."""
    from tests.gpuutil import knn_on_stream, make_index
    from tests.test_gpu_device_entry import CHAINS
    out = {}

    def keep(tag, ids, ds, cnt=None):
        out[tag + "/ids"] = ids
        out[tag + "/dists"] = np.ascontiguousarray(ds).view(np.uint32)
        if cnt is not None:
            out[tag + "/counts"] = cnt

    for name, (space, method, rows, queries, k, path, params) in CHAINS.items():
        idx = make_index(space, method, rows(), **params)
        Q = queries()
        ids, ds, cnt = idx.knnQueryBatch(Q, k)
        out[name + "/path"] = np.array([idx.stats()["last_path"]])
        keep(name + "/host", ids, ds, cnt)
        dids, dds, _ = knn_on_stream(idx, Q, k, counts=False)
        keep(name + "/device", dids, dds)
        if name in ("adaptive_f32", "adaptive_u8"):
            radius = float(ds[0, k - 1]) * 1.0001 + 1.0
            keep(name + "/range", *idx.rangeQueryFill(Q[0], radius, 64))
        if method == "hnsw":
            for ef in (800, 1200):
                idx.setQueryTimeParams(efSearch=ef)
                keep(f"{name}/ef{ef}", *idx.knnQueryBatch(Q, k))
        idx.close()
    return out


def main():
    np.savez(sys.argv[1], **run_all())


if __name__ == "__main__":
    main()
