#!/usr/bin/env python3
"""Time nmslib_gpu_consolidate against the only alternative an index with deleted rows had before it: a rebuild over the
live rows (not part of bench.py).

Workload: l2, 1M x 128 (s_lowrank of nmslib_zig_amd/datasets.py), a graph built on the GPU with M=16, efSearch 128, k 10,
batches of 1024 queries through nmslib_gpu_knn_query_batch_device.  Per share (1 %, 10 %, 30 % of the rows deleted at
random), on a graph built anew over all rows:
  (a) the tombstone search on the index with the rows marked: kernel_ms, recall@10;
  (b) consolidate(): its seconds by wall clock and split into worklist, repair and compaction (the engine reports them under
      NMSLIB_GPU_CONSOLIDATE_TRACE, waiting for each part), the lists repaired, the repair kernel's algorithmic bytes (one row
      per distance it evaluated) and the HBM rate that makes; hbm_bytes before and after; then kernel_ms and recall@10;
  (c) the rebuild in the same process: nmslib_reset_index, the live rows added, nmslib_create_index -- its seconds by wall
      clock -- then kernel_ms and recall@10 on it.
recall@10 is taken against the library's own exact scan over the live rows.  The child is a fresh process under its own
time limit; after a failure nothing more is started on the device.

    python3 tools/hnsw_consolidate_time.py [--rows 1000000] [--reps 30] [--out profiles/hnsw_consolidate_vs_rebuild.json]
"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPACE, DIM, M, EF_CONSTRUCTION, EF_SEARCH, K, NQ = "l2", 128, 16, 200, 128, 10, 1024
SHARES = (0.01, 0.10, 0.30)
TRACE = re.compile(r"consolidate: worklist ([0-9.]+) s, repair ([0-9.]+) s, compaction ([0-9.]+) s, (\d+) lists, (\d+) distances")


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child(nrows, reps, warmup, trace_path):
    sys.path.insert(0, ROOT)
    import torch

    import nmslib_zig_amd as nz
    from nmslib_zig_amd.datasets import recall_nmslib, s_lowrank
    X, Q = s_lowrank(nrows, DIM, 42), s_lowrank(NQ, DIM, 43)
    order = np.random.default_rng(44).permutation(nrows)
    dq = torch.from_numpy(Q).cuda()
    d_ids = torch.empty((NQ, K), dtype=torch.int32, device="cuda")
    d_ds = torch.empty((NQ, K), dtype=torch.float32, device="cuda")
    d_cnt = torch.empty((NQ,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    build = dict(M=M, efConstruction=EF_CONSTRUCTION, gpu_build=1)

    def exact(live):
        bf = nz.Index(SPACE, "seq_search")
        bf.addDenseBatch(X[live], live.astype(np.int32))
        bf.buildIndex()
        gi, gd, _ = bf.knnQueryBatch(Q, 32)
        bf.close()
        return gi, gd ** 2

    def leg(idx, truth):
        def batch():
            idx.knn_device(dq.data_ptr(), NQ, DIM, K, d_ids.data_ptr(), d_ds.data_ptr(), d_cnt.data_ptr(), stream)
        idx.setQueryTimeParams(efSearch=EF_SEARCH)
        for _ in range(warmup):
            batch()
        torch.cuda.synchronize()
        idx.kernel_timing(enable=True)
        for _ in range(reps):
            batch()
        torch.cuda.synchronize()
        kms, kn = idx.kernel_timing(enable=False, collect=True)
        ids, cnt = d_ids.cpu().numpy(), d_cnt.cpu().numpy()
        st = idx.stats()
        return {"kernel_ms": kms / max(kn, 1), "last_path": int(st["last_path"]), "hbm_bytes": int(st["hbm_bytes"]),
                "count_min": int(cnt.min()), "recall_at_10": float(recall_nmslib(ids, truth[0], truth[1], K))}

    shares = []
    for share in SHARES:
        dead = order[:int(nrows * share)]
        live = np.sort(order[int(nrows * share):])
        truth = exact(live)
        idx = nz.Index(SPACE, "hnsw")
        idx.addDenseBatch(X, np.arange(nrows, dtype=np.int32))
        idx.buildIndex(**build)
        full_build_seconds = idx.stats()["build_seconds"]
        assert idx.deleteIds(dead.astype(np.int32)) == len(dead)
        rec = {"share": share, "deleted": int(len(dead)), "full_build_seconds": full_build_seconds,
               "tombstone_search": leg(idx, truth)}
        t0 = time.perf_counter()
        removed, repaired = idx.consolidate()
        seconds = time.perf_counter() - t0
        assert removed == len(dead) and idx.dataQty() == len(live)
        sys.stderr.flush()
        m = TRACE.findall(open(trace_path).read())[-1]           # (this process's stderr: the engine's last trace line)
        wl, rp, cp, lists, dists = float(m[0]), float(m[1]), float(m[2]), int(m[3]), int(m[4])
        row_bytes = DIM * 4
        rec["consolidate"] = {"seconds": seconds, "worklist_seconds": wl, "repair_seconds": rp, "compaction_seconds": cp,
                              "lists_repaired": int(repaired), "repair_distances": dists,
                              "repair_algorithmic_bytes": dists * row_bytes,
                              "repair_hbm_GBps": dists * row_bytes / rp / 1e9 if rp > 0 else None}
        assert lists == repaired
        rec["consolidated"] = leg(idx, truth)
        t0 = time.perf_counter()
        idx.reset()
        idx.addDenseBatch(X[live], live.astype(np.int32))
        idx.buildIndex(**build)
        rec["rebuild"] = {"seconds": time.perf_counter() - t0, "build_seconds": idx.stats()["build_seconds"],
                          "upload_seconds": idx.stats()["upload_seconds"]}
        rec["rebuilt"] = leg(idx, truth)
        idx.close()
        log(json.dumps(rec))
        shares.append(rec)
    return {"shape": f"{nrows} x {DIM} {SPACE}", "M": M, "efConstruction": EF_CONSTRUCTION, "efSearch": EF_SEARCH, "k": K,
            "batch": NQ, "reps": reps, "warmup": warmup, "shares": shares}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help="(internal) the file the engine's trace goes to")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.rows, a.reps, a.warmup, a.child)))
        return
    trace_path = (a.out or os.path.join(ROOT, "hnsw_consolidate_time")) + ".trace"
    cmd = [sys.executable, os.path.abspath(__file__), "--child", trace_path, "--rows", str(a.rows), "--reps", str(a.reps),
           "--warmup", str(a.warmup)]
    # the engine's trace goes to the child's stderr: into a file the child reads back after each consolidate
    with open(trace_path, "w") as err:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=err, text=True, timeout=a.timeout,
                           env=dict(os.environ, NMSLIB_GPU_CONSOLIDATE_TRACE="1"))
    if r.returncode != 0:      # nothing more is started on the device after a failure
        sys.stderr.write(open(trace_path).read()[-4000:])
        raise SystemExit(f"child failed ({r.returncode})")
    os.remove(trace_path)
    out = {"tool": "tools/hnsw_consolidate_time.py", "date": time.strftime("%Y-%m-%d"),
           "method": "seconds: wall clock around the call (consolidate returns when the device is done; the rebuild is "
                     "nmslib_reset_index + add + nmslib_create_index); worklist / repair / compaction: the engine's own clock "
                     "with a wait behind each part; kernel_ms: nmslib_gpu_kernel_timing, mean over the timed batches; "
                     "recall_at_10 against the exact scan over the live rows; repair_hbm_GBps: one row per distance the "
                     "repair kernel evaluated, over its seconds",
           "run": json.loads(r.stdout.strip().splitlines()[-1])}
    out["consolidate_over_rebuild_seconds"] = {f"{s['share']:.0%}": s["consolidate"]["seconds"] / s["rebuild"]["seconds"]
                                               for s in out["run"]["shares"]}
    print(json.dumps({k: v for k, v in out.items() if k != "run"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
