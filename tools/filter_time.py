#!/usr/bin/env python3
"""Time filtered k-NN (nmslib_gpu_filter_*; not part of bench.py).

Workload: l2, 1M x 128 (s_lowrank of nmslib_zig_amd/datasets.py), k 10, batches of 1024 queries through the device entries.
Two index kinds, each in a child process of its own: hnsw (one graph built on the GPU with M=16, efSearch 128) and
brute_force.  Legs, in the order run: unfiltered; random filters that allow 50 %, 10 %, 1 %, 0.1 % and 0.01 % of the rows;
then the unfiltered leg twice more -- the spread of the three unfiltered legs is known before one of them is compared with
the parent commit's.  Per leg: `--warmup` batches, then `--reps` batches, each timed twice: nmslib_gpu_kernel_timing (HIP
events inside the engine around the dominant launches) and HIP events around the whole call on the caller's stream.  Per
filter: the seconds nmslib_gpu_filter_create took, the device bytes the filter holds, the rows it allows, and the path the
batch took (hnsw: 4 = walk route, 7 = subset route; a subset between efSearch and 4096 rows is run a second time
with scan_rows = 4096, which puts it on the subset route).  recall@10 of a leg is taken against an exact scan over an index
built from the allowed rows alone.

With --parent-root (a checkout of the parent commit whose library is built) one more child per kind imports that package
and runs the unfiltered leg alone, in the same call.  Every child is a fresh process under its own time limit; after a
failure nothing more is started on the device.

    python3 tools/filter_time.py [--rows 1000000] [--reps 30] [--parent-root DIR] [--out profiles/filter_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPACE, DIM, M, EF_CONSTRUCTION, EF_SEARCH, K, NQ = "l2", 128, 16, 200, 128, 10, 1024
SHARES = (0.5, 0.1, 0.01, 0.001, 0.0001)
KINDS = ("hnsw", "brute_force")
SCAN_ROWS = 4096


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child(kind, nrows, reps, warmup, parent_root):
    sys.path.insert(0, os.path.abspath(parent_root) if parent_root else ROOT)
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
    out_ptrs = (d_ids.data_ptr(), d_ds.data_ptr(), d_cnt.data_ptr(), stream)

    def exact(allowed):
        bf = nz.Index(SPACE, "seq_search")
        bf.addDenseBatch(X[allowed], allowed.astype(np.int32))
        bf.buildIndex()
        gi, gd, _ = bf.knnQueryBatch(Q, 32)
        bf.close()
        return gi, gd ** 2

    def leg(idx, name, truth, flt, extra):
        def batch():
            if flt is None:
                idx.knn_device(dq.data_ptr(), NQ, DIM, K, *out_ptrs)
            else:
                idx.knn_device_filtered(flt, dq.data_ptr(), NQ, DIM, K, *out_ptrs)
        for _ in range(warmup):
            batch()
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
        ids, cnt = d_ids.cpu().numpy(), d_cnt.cpu().numpy()
        st = idx.stats()
        rec = {"leg": name, "last_path": int(st["last_path"]), "kernel_ms": kms / max(reps, 1), "kernel_intervals": int(kn),
               "batch_ms": float(np.median(whole)),
               "batch_ms_min": float(whole.min()), "batch_ms_max": float(whole.max()), "count_mean": float(cnt.mean()),
               "count_min": int(cnt.min()), "recall_at_10": float(recall_nmslib(ids, truth[0], truth[1], K))}
        rec.update(extra)
        log(f"{kind} {name}: kernel {rec['kernel_ms']:.4f} ms, batch {rec['batch_ms']:.4f} ms, count "
            f"{rec['count_mean']:.2f}, recall {rec['recall_at_10']:.4f}, path {rec['last_path']} {extra}")
        return rec

    all_ids = np.arange(nrows, dtype=np.int32)
    truth_all = exact(np.arange(nrows))
    log("exact scan over all rows done")
    idx = nz.Index(SPACE, kind)
    idx.addDenseBatch(X, all_ids)
    if kind == "hnsw":
        idx.buildIndex(M=M, efConstruction=EF_CONSTRUCTION, gpu_build=1)
        idx.setQueryTimeParams(efSearch=EF_SEARCH)
    else:
        idx.buildIndex()
    idx.finalize()
    build_seconds = idx.stats()["build_seconds"]
    legs = [leg(idx, "unfiltered", truth_all, None, {"allowed_share": 1.0})]
    if not parent_root:
        for share in SHARES:
            allowed = np.sort(order[:max(1, int(round(nrows * share)))])
            mask = np.zeros(nrows, bool)
            mask[allowed] = True
            t0 = time.perf_counter()
            flt = idx.makeFilter(mask)
            create_seconds = time.perf_counter() - t0
            extra = {"allowed_share": share, "allowed_rows": int(flt.allowed), "filter_create_seconds": create_seconds,
                     "filter_hbm_bytes": int(flt.hbm_bytes)}
            truth = exact(allowed)
            legs.append(leg(idx, f"{share:.2%} allowed", truth, flt, extra))
            flt.close()
            if kind == "hnsw" and EF_SEARCH < len(allowed) <= SCAN_ROWS:
                # the same subset with the caller's bound raised to the kernel's capacity: the subset route
                flt = idx.makeFilter(mask, scan_rows=SCAN_ROWS)
                legs.append(leg(idx, f"{share:.2%} allowed, scan_rows={SCAN_ROWS}", truth, flt,
                                dict(extra, scan_rows=SCAN_ROWS, filter_hbm_bytes=int(flt.hbm_bytes))))
                flt.close()
        for i in (2, 3):
            legs.append(leg(idx, f"unfiltered ({i})", truth_all, None, {"allowed_share": 1.0}))
    idx.close()
    return {"kind": kind, "shape": f"{nrows} x {DIM} {SPACE}", "M": M, "efConstruction": EF_CONSTRUCTION, "efSearch": EF_SEARCH,
            "k": K, "batch": NQ, "reps": reps, "warmup": warmup, "build_seconds": build_seconds, "legs": legs}


def run_child(a, kind, parent_root):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--rows", str(a.rows), "--reps", str(a.reps),
           "--warmup", str(a.warmup)] + (["--parent-root", parent_root] if parent_root else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
    if r.returncode != 0:      # nothing more is started on the device after a failure
        raise SystemExit(f"child failed ({r.returncode})")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, choices=KINDS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.rows, a.reps, a.warmup, a.parent_root)))
        return
    out = {"tool": "tools/filter_time.py", "date": time.strftime("%Y-%m-%d"),
           "method": "kernel_ms: nmslib_gpu_kernel_timing (HIP events inside the engine), summed over the timed batches and "
                     "divided by their number; batch_ms: median of HIP events around the device entry on the "
                     "caller's stream; recall_at_10 against an exact scan over an index of the allowed rows alone; legs in the "
                     "order run",
           "runs": {}, "summary": {}}
    for kind in KINDS:
        run = out["runs"][kind] = run_child(a, kind, None)
        unf = [g["batch_ms"] for g in run["legs"] if g["allowed_share"] == 1.0]
        s = out["summary"][kind] = {"unfiltered_batch_ms": unf, "unfiltered_batch_ms_spread": max(unf) - min(unf)}
        if a.parent_root:
            par = out["runs"][kind + " (parent)"] = run_child(a, kind, a.parent_root)
            p = par["legs"][0]["batch_ms"]
            s["parent_batch_ms"] = p
            s["parent_within_the_spread"] = bool(min(unf) - s["unfiltered_batch_ms_spread"] <= p <=
                                                 max(unf) + s["unfiltered_batch_ms_spread"])
    print(json.dumps(out["summary"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
