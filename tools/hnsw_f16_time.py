#!/usr/bin/env python3
"""Time the HNSW search with the walk on the f32 rows against the walk on the fp16 copy (gpu_rows=f16),
over one and the same graph (not part of bench.py).

Shapes (generators of nmslib_zig_amd/datasets.py):
    128  1M x 128 l2,            M=16, efSearch 128, batch 1024
    768  1M x 768 cosinesimil,   M=16, efSearch 128, batch 8192
One index per shape, built on the GPU; the query-time parameter gpu_rows switches the traversal.  Legs, in this order:
f32, f16, f32, f32 -- the f32 leg three times, so that the run-to-run spread of one leg is known before two legs are
compared.  Per leg: `--warmup` batches, then `--reps` batches through nmslib_gpu_knn_query_batch_device, each timed twice:
nmslib_gpu_kernel_timing (HIP events inside the engine: the walk; in f16 mode walk + overflow launch + re-rank) and HIP
events around the whole call on the caller's stream.  recall@10 of both traversals is taken against the library's own exact
scan over the same rows.  Every shape runs in a fresh child process under its own time limit; after a failure nothing more
is started on the device.

    python3 tools/hnsw_f16_time.py [--shapes 128,768] [--rows 1000000] [--reps 30] [--out profiles/hnsw_f16_vs_f32.json]
    python3 tools/hnsw_f16_time.py --f32-only --tag parent --lib <parent's libnmslib_c.so> --out parent.json
    python3 tools/hnsw_f16_time.py --merge parent.json ...                        # record that run beside this one
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

SHAPES = {
    "128": dict(space="l2", dim=128, batch=1024),
    "768": dict(space="cosinesimil", dim=768, batch=8192),
}
M, EF_CONSTRUCTION, EF_SEARCH, K = 16, 200, 128, 10


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child(shape, nrows, reps, warmup, f32_only, lib):
    import torch

    import nmslib_zig_amd as nz
    if lib:
        nz.LIB_PATH = os.path.abspath(lib)   # another build of the library (the parent commit's)
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
    log(f"{shape}: exact scan done")
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
    for rows in (("f32",) if f32_only else ("f32", "f16", "f32", "f32")):
        if f32_only:
            idx.setQueryTimeParams(efSearch=EF_SEARCH)
        else:
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
        ids = d_ids.cpu().numpy()
        ndc = idx.read_counters(nq)[0].astype(np.int64)
        legs.append({"gpu_rows": rows, "last_path": int(idx.stats()["last_path"]), "hbm_bytes": int(hbm),
                     "kernel_ms_mean": kms / max(kn, 1), "kernel_intervals": int(kn),
                     "batch_ms_median": float(np.median(whole)), "batch_ms_min": float(whole.min()),
                     "batch_ms_max": float(whole.max()), "queries_per_s": nq / (float(np.median(whole)) * 1e-3),
                     "ndc_mean": float(ndc.mean()),
                     "recall_at_10": float(recall_nmslib(ids[:1024], gt_i, gt_key, K))})
        log(f"{shape} {rows}: kernel {legs[-1]['kernel_ms_mean']:.4f} ms, batch {legs[-1]['batch_ms_median']:.4f} ms, "
            f"recall {legs[-1]['recall_at_10']:.4f}")
    idx.close()
    rec = {"shape": f"{nrows} x {dim} {space}", "M": M, "efConstruction": EF_CONSTRUCTION, "efSearch": EF_SEARCH, "k": K,
           "batch": nq, "reps": reps, "warmup": warmup, "build_seconds": st["build_seconds"], "legs": legs}
    f32 = [g["kernel_ms_mean"] for g in legs if g["gpu_rows"] == "f32"]
    rec["f32_kernel_ms_spread"] = max(f32) - min(f32)
    f16 = [g["kernel_ms_mean"] for g in legs if g["gpu_rows"] == "f16"]
    if f16:
        rec["f16_kernel_ms_gain_over_slowest_f32"] = max(f32) - f16[0]
        rec["f16_kernel_ms_gain_over_fastest_f32"] = min(f32) - f16[0]
        rec["f16_faster_by_more_than_the_spread"] = bool(min(f32) - f16[0] > rec["f32_kernel_ms_spread"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128,768")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--f32-only", action="store_true", help="one f32 leg, no gpu_rows parameter (runs on older commits)")
    ap.add_argument("--lib", default=None, help="path of another build of libnmslib_c.so to measure instead")
    ap.add_argument("--tag", default="new")
    ap.add_argument("--merge", default=None, help="JSON written by another run (e.g. the parent commit's), recorded beside this one")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.rows, a.reps, a.warmup, a.f32_only, a.lib)))
        return
    out = {"tool": "tools/hnsw_f16_time.py", "tag": a.tag, "date": time.strftime("%Y-%m-%d"),
           "method": "kernel_ms: nmslib_gpu_kernel_timing (HIP events inside the engine), mean over the timed batches; batch_ms: "
                     "HIP events around nmslib_gpu_knn_query_batch_device on the caller's stream; legs in the order run",
           "runs": []}
    if a.merge:
        with open(a.merge) as f:
            out["other"] = json.load(f)
    for shape in a.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", shape, "--rows", str(a.rows), "--reps", str(a.reps),
               "--warmup", str(a.warmup)] + (["--f32-only"] if a.f32_only else []) + (["--lib", a.lib] if a.lib else [])
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
