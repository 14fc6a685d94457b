#!/usr/bin/env python3
"""Time the HNSW search with the walk on the f32 rows, on the fp16 copy and on the 8-bit copy (gpu_rows=f32 | f16 | i8,
DESIGN.md 4.4, 4.4a) over one and the same graph (not part of bench.py).  Modelled on tools/hnsw_f16_time.py, whose shapes,
timers and child process it uses.

Legs, in this order: f32, f16, i8, f32 -- the f32 leg twice, so that the run-to-run spread of one leg is known before two
legs are compared.  Per leg: kernel and batch times, the mean ndc, recall@10 against the library's own exact scan over the
same rows, and the HBM the index holds (the copies are made at their first batch, so the differences are their sizes).

    python3 tools/hnsw_i8_time.py [--shapes 128,768] [--rows 1000000] [--reps 30] [--out profiles/hnsw_i8_vs_f32.json]
    python3 tools/hnsw_f16_time.py --f32-only --tag parent --lib <parent's libnmslib_c.so> --out parent.json
    python3 tools/hnsw_i8_time.py --merge parent.json ...                          # record that run beside this one
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.hnsw_f16_time import EF_CONSTRUCTION, EF_SEARCH, K, M, SHAPES, log  # noqa: E402

LEGS = ("f32", "f16", "i8", "f32")


def child(shape, nrows, reps, warmup):
    import torch

    import nmslib_zig_amd as nz
    from nmslib_zig_amd.datasets import recall_nmslib, s_lowrank
    cfg = SHAPES[shape]
    space, dim, nq = cfg["space"], cfg["dim"], cfg["batch"]
    X, Q = s_lowrank(nrows, dim, 42), s_lowrank(nq, dim, 43)
    bf = nz.Index(space, "seq_search")
    bf.addDenseBatch(X)
    bf.buildIndex()
    gt_i, gt_d, _ = bf.knnQueryBatch(Q[:1024], 32)
    bf.close()
    gt_key = gt_d ** 2 if space == "l2" else gt_d
    idx = nz.Index(space, "hnsw")
    idx.addDenseBatch(X)
    idx.buildIndex(M=M, efConstruction=EF_CONSTRUCTION, gpu_build=1)
    st = idx.stats()
    log(f"{shape}: graph built in {st['build_seconds']:.1f} s ({st['hbm_bytes'] >> 20} MiB in HBM)")
    dq = torch.from_numpy(Q).cuda()
    d_ids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    d_ds = torch.empty((nq, K), dtype=torch.float32, device="cuda")
    d_cnt = torch.empty((nq,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def batch():
        idx.knn_device(dq.data_ptr(), nq, dim, K, d_ids.data_ptr(), d_ds.data_ptr(), d_cnt.data_ptr(), stream)

    legs = []
    for rows in LEGS:
        idx.setQueryTimeParams(efSearch=EF_SEARCH, gpu_rows=rows)
        for _ in range(warmup):
            batch()
        torch.cuda.synchronize()
        hbm = idx.stats()["hbm_bytes"]
        idx.kernel_timing(enable=True)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            batch()
            b.record()
        torch.cuda.synchronize()
        kms, kn = idx.kernel_timing(enable=False, collect=True)
        whole = np.array([a.elapsed_time(b) for a, b in ev])
        ndc = idx.read_counters(nq)[0].astype(np.int64)
        legs.append({"gpu_rows": rows, "last_path": int(idx.stats()["last_path"]), "hbm_bytes": int(hbm),
                     "kernel_ms_mean": kms / max(kn, 1), "kernel_intervals": int(kn),
                     "batch_ms_median": float(np.median(whole)), "batch_ms_min": float(whole.min()),
                     "batch_ms_max": float(whole.max()), "ndc_mean": float(ndc.mean()),
                     "recall_at_10": float(recall_nmslib(d_ids.cpu().numpy()[:1024], gt_i, gt_key, K))})
        log(f"{shape} {rows}: kernel {legs[-1]['kernel_ms_mean']:.4f} ms, batch {legs[-1]['batch_ms_median']:.4f} ms, "
            f"ndc {legs[-1]['ndc_mean']:.0f}, recall {legs[-1]['recall_at_10']:.4f}")
    idx.close()
    by = {}
    for g in legs:
        by.setdefault(g["gpu_rows"], []).append(g)
    f32 = [g["kernel_ms_mean"] for g in by["f32"]]
    return {"shape": f"{nrows} x {dim} {space}", "M": M, "efConstruction": EF_CONSTRUCTION, "efSearch": EF_SEARCH, "k": K,
            "batch": nq, "reps": reps, "warmup": warmup, "build_seconds": st["build_seconds"], "legs": legs,
            "f32_kernel_ms_spread": max(f32) - min(f32),
            "f16_copy_bytes": by["f16"][0]["hbm_bytes"] - by["f32"][0]["hbm_bytes"],
            "i8_copy_bytes": by["i8"][0]["hbm_bytes"] - by["f16"][0]["hbm_bytes"],
            "i8_kernel_ms_minus_f16": by["i8"][0]["kernel_ms_mean"] - by["f16"][0]["kernel_ms_mean"],
            "i8_kernel_ms_minus_fastest_f32": by["i8"][0]["kernel_ms_mean"] - min(f32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128,768")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--merge", default=None, help="JSON of tools/hnsw_f16_time.py --f32-only on the parent commit's library")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.rows, a.reps, a.warmup)))
        return
    out = {"tool": "tools/hnsw_i8_time.py", "date": time.strftime("%Y-%m-%d"),
           "method": "kernel_ms: nmslib_gpu_kernel_timing (HIP events inside the engine: the walk; f16 and i8: walk + overflow "
                     "launch + re-rank), mean over the timed batches; batch_ms: HIP events around "
                     "nmslib_gpu_knn_query_batch_device on the caller's stream; legs in the order run",
           "runs": []}
    if a.merge:
        with open(a.merge) as f:
            out["parent_f32"] = json.load(f)
    for shape in a.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--rows", str(a.rows), "--reps", str(a.reps),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if r.returncode != 0:      # nothing more is started on the device after a failure
            raise SystemExit(f"shape {shape}: child failed ({r.returncode})")
        out["runs"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(out["runs"][-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
