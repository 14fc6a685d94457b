#!/usr/bin/env python3
"""Time an add after the build of a GPU-built HNSW index with and without gpu_append=1 (not part of bench.py).

Workload: l2, 1M x 128 (s_lowrank of nmslib_zig_amd/datasets.py), M=16, efConstruction=200.  Two legs over the same rows,
in this order: `rebuild` (gpu_append=0, what every add cost before) and `append` (gpu_append=1).  Each leg builds the first
rows - add rows, adds the last `--add` rows and times the finalize that follows (wall clock around nmslib_gpu_finalize, plus
the engine's own upload_seconds / build_seconds and rows_uploaded / rows_appended).  recall@10 at efSearch=128 of both
results is taken against the library's own exact scan over all rows: the rebuild leg's graph is a fresh full build.  The run
is one fresh child process under a time limit; after a failure nothing more is started on the device.

    python3 tools/hnsw_append_time.py [--rows 1000000] [--add 10000] [--out profiles/hnsw_append_parent_vs_new.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPACE, DIM, M, EF_CONSTRUCTION, EF_SEARCH, K, NQ = "l2", 128, 16, 200, 128, 10, 1024


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child(nrows, nadd):
    import numpy as np

    import nmslib_zig_amd as nz
    from nmslib_zig_amd.datasets import recall_nmslib, s_lowrank
    X, Q = s_lowrank(nrows, DIM, 42), s_lowrank(NQ, DIM, 43)
    n0 = nrows - nadd
    bf = nz.Index(SPACE, "seq_search")
    bf.addDenseBatch(X)
    bf.buildIndex()
    gt_i, gt_d, _ = bf.knnQueryBatch(Q, 32)
    bf.close()
    log("exact scan done")
    legs = []
    for name, gpu_append in (("rebuild", 0), ("append", 1)):
        idx = nz.Index(SPACE, "hnsw")
        idx.addDenseBatch(X[:n0])
        idx.buildIndex(M=M, efConstruction=EF_CONSTRUCTION, gpu_build=1, gpu_append=gpu_append)
        first = idx.stats()
        idx.addDenseBatch(X[n0:], np.arange(n0, nrows, dtype=np.int32))
        t0 = time.perf_counter()
        idx.finalize()
        wall = time.perf_counter() - t0
        st = idx.stats()
        idx.setQueryTimeParams(efSearch=EF_SEARCH)
        ids, _, _ = idx.knnQueryBatch(Q, K)
        legs.append({"leg": name, "gpu_append": gpu_append, "first_build_seconds": first["build_seconds"],
                     "first_upload_seconds": first["upload_seconds"], "finalize_wall_seconds": wall,
                     "finalize_upload_seconds": st["upload_seconds"], "finalize_build_seconds": st["build_seconds"],
                     "rows_uploaded": int(st["rows_uploaded"]), "rows_appended": int(st["rows_appended"]),
                     "hbm_bytes": int(st["hbm_bytes"]), "graph_builder": idx.graphBuilder(),
                     "recall_at_10": float(recall_nmslib(ids, gt_i, gt_d ** 2, K))})
        log(f"{name}: first build {first['build_seconds']:.2f} s; finalize after the add {wall:.3f} s, "
            f"{st['rows_uploaded']} rows uploaded, recall {legs[-1]['recall_at_10']:.4f}")
        idx.close()
    return {"shape": f"{nrows} x {DIM} {SPACE}", "rows_before": n0, "rows_added": nadd, "M": M,
            "efConstruction": EF_CONSTRUCTION, "efSearch": EF_SEARCH, "k": K, "queries": NQ, "legs": legs,
            "append_over_rebuild_wall": legs[1]["finalize_wall_seconds"] / legs[0]["finalize_wall_seconds"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--add", type=int, default=10_000)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.rows, a.add)))
        return
    out = {"tool": "tools/hnsw_append_time.py", "date": time.strftime("%Y-%m-%d"),
           "method": "finalize_wall_seconds: perf_counter around nmslib_gpu_finalize after the add (it returns when the index "
                     "is resident); finalize_upload_seconds / finalize_build_seconds: the engine's own clocks; the rebuild leg "
                     "(gpu_append=0) is the behaviour before gpu_append existed, and its graph is a fresh full build"}
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows), "--add", str(a.add)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
    if r.returncode != 0:      # nothing more is started on the device after a failure
        raise SystemExit(f"child failed ({r.returncode})")
    out["run"] = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(out["run"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
