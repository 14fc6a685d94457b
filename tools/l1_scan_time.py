#!/usr/bin/env python3
"""Time the exact l1 scan at the large-batch shape (not part of bench.py).

Workload: 1M x 128 float rows, one batch of 1024 queries, k = 10, on Gaussian rows (gauss128) and on low-rank rows
(lowrank128).  Legs, each in a fresh child process under its own time limit: the l1 fast path (last_path 6), the same
library with NMSLIB_GPU_L1_FAST=0 (the adaptive VALU kernel), and -- with --parent-lib -- another build of the library
(the parent commit's) measured in the same session.  The figure is the median HIP-event time of `--reps` warm batches
through nmslib_gpu_knn_query_batch_device (device buffers, the caller's stream).

The first leg also counts, for 8 queries in numpy f64, the rows inside the error band of the filter
(s * SAD <= d_k - X_q + E_q): what the scan's lists must hold for the proof to succeed.

    python3 tools/l1_scan_time.py [--parent-lib <libnmslib_c.so>] [--out profiles/l1_fast_parent_vs_new.json]
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

K = 10


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def band_rows(X, Q, dk):
    """rows with s * SAD <= d_k - X_q + E_q per query, by the formulas of csrc/l1_quant.hpp"""
    lo, hi = X.min(0).astype(np.float64), X.max(0).astype(np.float64)
    s = (hi - lo).max() / 255.0
    xb = np.rint((X.astype(np.float64) - lo) / s)
    rmax = np.abs(X - (lo + s * xb)).max(0)
    xb = xb.astype(np.int16)
    out = []
    for q, d in zip(Q.astype(np.float64), dk):
        qc = np.clip(q, lo, hi)
        qb = np.rint((qc - lo) / s)
        excess = np.abs(q - qc).sum()
        bound = (np.abs(qc - (lo + s * qb)) + rmax).sum()
        sad = np.abs(xb - qb.astype(np.int16)).sum(1, dtype=np.int64)
        out.append(int((s * sad <= float(d) - excess + bound).sum()))
    return out


def child(data, nrows, dim, nq, reps, lib, count_band):
    import torch

    import nmslib_zig_amd as nz
    if lib:
        nz.LIB_PATH = os.path.abspath(lib)   # another build of the library (the parent commit's)
    from nmslib_zig_amd.datasets import s_gauss, s_lowrank
    gen = s_gauss if data.startswith("gauss") else s_lowrank
    X, Q = gen(nrows, dim, 42), gen(nq, dim, 43)
    idx = nz.Index("l1", "seq_search")
    idx.addDenseBatch(X)
    idx.buildIndex()
    hbm = int(idx.stats()["hbm_bytes"])
    log(f"{data}: index built and uploaded ({hbm >> 20} MiB in HBM)")
    dq = torch.from_numpy(Q).cuda()
    d_ids = torch.empty((nq, K), dtype=torch.int32, device="cuda")
    d_ds = torch.empty((nq, K), dtype=torch.float32, device="cuda")
    d_cnt = torch.empty((nq,), dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def batch():
        idx.knn_device(dq.data_ptr(), nq, dim, K, d_ids.data_ptr(), d_ds.data_ptr(), d_cnt.data_ptr(), stream)

    for _ in range(3):
        batch()                                             # warm-up: code objects, workspaces, clocks
    torch.cuda.synchronize()
    idx.kernel_timing(enable=True)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        batch()
        b.record()
    torch.cuda.synchronize()
    kms, kn = idx.kernel_timing(enable=False, collect=True)
    whole = np.array([a.elapsed_time(b) for a, b in ev])
    st = idx.stats()
    rec = {"data": data, "rows": nrows, "dim": dim, "batch": nq, "k": K, "reps": reps, "hbm_bytes": hbm,
           "l1_fast_env": os.environ.get("NMSLIB_GPU_L1_FAST"), "lib": "other build" if lib else "this build",
           "last_path": int(st["last_path"]), "fast_tiles": int(st["fast_tiles"]),
           "fast_tiles_fallback": int(st["fast_tiles_fallback"]),
           "batch_ms_median": float(np.median(whole)), "batch_ms_min": float(whole.min()), "batch_ms_max": float(whole.max()),
           "scan_ms_mean": kms / max(kn, 1), "ids_checksum": int(d_ids.cpu().numpy().astype(np.int64).sum()),
           "dists_checksum": int(d_ds.cpu().numpy().view(np.uint32).astype(np.int64).sum())}
    idx.close()
    if count_band:
        counts = band_rows(X, Q[:8], d_ds.cpu().numpy()[:8, K - 1])
        rec["band_rows_per_query"] = {"queries": 8, "median": float(np.median(counts)), "max": int(max(counts))}
    log(f"{data}: path {rec['last_path']}, batch {rec['batch_ms_median']:.3f} ms, fallback tiles {rec['fast_tiles_fallback']}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", default="gauss128,lowrank128")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--parent-lib", default=None, help="libnmslib_c.so of the parent commit, measured beside this build")
    ap.add_argument("--sad-rate", default=None, help="text of the tools/probe/sad_probe.hip run of the same session, recorded as is")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--count-band", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.rows, a.dim, a.batch, a.reps, a.lib, a.count_band)))
        return
    out = {"tool": "tools/l1_scan_time.py", "date": time.strftime("%Y-%m-%d"),
           "method": "batch_ms: HIP events around nmslib_gpu_knn_query_batch_device on the caller's stream, median of the warm "
                     "batches; scan_ms: nmslib_gpu_kernel_timing (HIP events around the selection / scan launch); legs in the "
                     "order run, one process each",
           "legs": []}
    if a.sad_rate:
        with open(a.sad_rate) as f:
            out["sad_probe"] = f.read().splitlines()
    legs = [("new", None, None), ("new_l1_fast_off", None, "0")]
    if a.parent_lib:
        legs.append(("parent", a.parent_lib, None))
    for data in a.data.split(","):
        for tag, lib, env in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", data, "--rows", str(a.rows), "--dim", str(a.dim),
                   "--batch", str(a.batch), "--reps", str(a.reps)] + (["--lib", lib] if lib else []) + \
                  (["--count-band"] if tag == "new" else [])
            e = dict(os.environ)
            e.pop("NMSLIB_GPU_L1_FAST", None)
            if env is not None:
                e["NMSLIB_GPU_L1_FAST"] = env
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout, env=e)
            if r.returncode != 0:      # nothing more is started on the device after a failure
                raise SystemExit(f"{data} {tag}: child failed ({r.returncode})")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            rec["leg"] = tag
            out["legs"].append(rec)
            print(json.dumps(rec), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
    by = {(g["data"], g["leg"]): g for g in out["legs"]}
    out["gate"] = {}
    for data in a.data.split(","):
        if (data, "parent") in by:
            new, par = by[(data, "new")], by[(data, "parent")]
            out["gate"][data] = {"new_ms": new["batch_ms_median"], "parent_ms": par["batch_ms_median"],
                                 "ratio": new["batch_ms_median"] / par["batch_ms_median"],
                                 "at_most_half": bool(new["batch_ms_median"] <= 0.5 * par["batch_ms_median"]),
                                 "same_answers": new["ids_checksum"] == par["ids_checksum"] and
                                 new["dists_checksum"] == par["dists_checksum"]}
    print(json.dumps(out["gate"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
