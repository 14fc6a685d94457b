#!/usr/bin/env python3
"""Time a batch with one filter per query against a loop of single-filter batches (not part of bench.py).

Workload: l2, 1M x 128 (s_lowrank of nmslib_zig_amd/datasets.py), k 10, batches of 1024 queries through the device entries.
T disjoint, equal-sized tenants (row p belongs to tenant perm[p] % T), T in 1, 8, 64, 512; query q belongs to tenant q % T.
Two ways to answer the batch, in the same process and run:
  each: one nmslib_gpu_knn_query_batch_filtered_each_device call over the 1024 queries in the caller's (interleaved) order;
  loop: what there was before it -- the caller sorts the queries by tenant once (not timed) and makes one
        nmslib_gpu_knn_query_batch_filtered_device call per tenant over that tenant's slice.
Three index kinds, each in a child process of its own: hnsw (built on the GPU with M=16, efSearch 128; the two stages),
hnsw with gpu_inwalk=1, and brute_force.  The in-walk kind stops at T = 64: its walk grows with 1 / share of eligible rows
(DESIGN.md 6 "in-walk filtering"), at T = 512 a tenant holds 0.2 % of the rows and one pass of the loop takes tens of seconds.
Per leg: `--warmup` batches, then `--reps` batches, each between two HIP events on the caller's stream (the interval holds
the host's enqueue time as well: that is what a loop of small calls is made of); the median, the smallest and the largest
are kept.  The two ways are checked to return the same ids before they are timed.
Every child is a fresh process under its own time limit; after a failure nothing more is started on the device.

    python3 tools/filter_each_time.py [--rows 1000000] [--reps 20] [--out profiles/filter_each_vs_loop.json]
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
TENANTS = {"hnsw": (1, 8, 64, 512), "hnsw_inwalk": (1, 8, 64), "brute_force": (1, 8, 64, 512)}
KINDS = tuple(TENANTS)


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child(kind, nrows, reps, warmup):
    sys.path.insert(0, ROOT)
    import torch

    import nmslib_zig_amd as nz
    from nmslib_zig_amd.datasets import s_lowrank
    X, Q = s_lowrank(nrows, DIM, 42), s_lowrank(NQ, DIM, 43)
    perm = np.random.default_rng(44).permutation(nrows)
    idx = nz.Index(SPACE, "brute_force" if kind == "brute_force" else "hnsw")
    idx.addDenseBatch(X, np.arange(nrows, dtype=np.int32))
    if kind == "brute_force":
        idx.buildIndex()
    else:
        idx.buildIndex(M=M, efConstruction=EF_CONSTRUCTION, gpu_build=1)
        idx.setQueryTimeParams(efSearch=EF_SEARCH, gpu_inwalk=1 if kind == "hnsw_inwalk" else 0)
    idx.finalize()
    stream = torch.cuda.current_stream().cuda_stream

    def buffers():
        return (torch.empty((NQ, K), dtype=torch.int32, device="cuda"), torch.empty((NQ, K), dtype=torch.float32, device="cuda"),
                torch.empty((NQ,), dtype=torch.int32, device="cuda"))

    def timed(batch):
        for _ in range(warmup):
            batch()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            batch()
            b.record()
        torch.cuda.synchronize()
        ms = np.array([a.elapsed_time(b) for a, b in ev])
        return {"ms": float(np.median(ms)), "ms_min": float(ms.min()), "ms_max": float(ms.max())}

    legs = []
    for T in TENANTS[kind]:
        tenant_of_row = perm % T
        t0 = time.perf_counter()
        filters = [idx.makeFilter(tenant_of_row == t) for t in range(T)]
        create_seconds = time.perf_counter() - t0
        fq = (np.arange(NQ) % T).astype(np.int32)
        order = np.argsort(fq, kind="stable")
        bounds = np.searchsorted(fq[order], np.arange(T + 1))
        dq = torch.from_numpy(Q).cuda()
        dq_sorted = torch.from_numpy(np.ascontiguousarray(Q[order])).cuda()
        e_ids, e_ds, e_cnt = buffers()
        l_ids, l_ds, l_cnt = buffers()
        routes = np.zeros(NQ, np.int32)

        def each():
            idx.knn_device_each_filtered(filters, fq, dq.data_ptr(), NQ, DIM, K, e_ids.data_ptr(), e_ds.data_ptr(),
                                         e_cnt.data_ptr(), stream, routes=routes)

        def loop():
            for t in range(T):
                a, b = int(bounds[t]), int(bounds[t + 1])
                idx.knn_device_filtered(filters[t], dq_sorted.data_ptr() + a * DIM * 4, b - a, DIM, K,
                                        l_ids.data_ptr() + a * K * 4, l_ds.data_ptr() + a * K * 4, l_cnt.data_ptr() + a * 4,
                                        stream)

        each()
        loop()
        torch.cuda.synchronize()
        same = bool((e_ids.cpu().numpy()[order] == l_ids.cpu().numpy()).all() and
                    (e_cnt.cpu().numpy()[order] == l_cnt.cpu().numpy()).all())
        rec = {"tenants": T, "rows_per_tenant": int((tenant_of_row == 0).sum()), "queries_per_tenant": NQ // T,
               "filters_create_seconds": create_seconds, "same_ids_and_counts": same,
               "routes": sorted(int(v) for v in np.unique(routes)), "count_mean": float(e_cnt.float().mean().item()),
               "each": timed(each), "loop": timed(loop)}
        # the batch sorted by tenant is in plan order: what the permutation costs
        fq_sorted = np.ascontiguousarray(fq[order])

        def each_sorted():
            idx.knn_device_each_filtered(filters, fq_sorted, dq_sorted.data_ptr(), NQ, DIM, K, e_ids.data_ptr(),
                                         e_ds.data_ptr(), e_cnt.data_ptr(), stream)

        rec["each_in_plan_order"] = timed(each_sorted)
        rec["loop_over_each"] = rec["loop"]["ms"] / rec["each"]["ms"]
        legs.append(rec)
        log(f"{kind} T={T}: each {rec['each']['ms']:.4f} ms (in plan order {rec['each_in_plan_order']['ms']:.4f}), loop "
            f"{rec['loop']['ms']:.4f} ms, routes {rec['routes']}, same {same}, filters made in {create_seconds:.2f} s")
        if not same:
            raise SystemExit("the two ways disagree")
        for f in filters:
            f.close()
    idx.close()
    return {"kind": kind, "shape": f"{nrows} x {DIM} {SPACE}", "M": M, "efConstruction": EF_CONSTRUCTION, "efSearch": EF_SEARCH,
            "k": K, "batch": NQ, "reps": reps, "warmup": warmup, "legs": legs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kinds", default=",".join(KINDS), help="the index kinds to run, comma-separated")
    ap.add_argument("--child", default=None, choices=KINDS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.rows, a.reps, a.warmup)))
        return
    out = {"tool": "tools/filter_each_time.py", "date": time.strftime("%Y-%m-%d"),
           "method": "ms: median of HIP events around the whole way of answering the batch (one call, or one call per tenant) "
                     "on the caller's stream, host enqueue time included; legs in the order run",
           "runs": {}}
    for kind in a.kinds.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--rows", str(a.rows), "--reps", str(a.reps),
               "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if r.returncode != 0:      # nothing more is started on the device after a failure
            raise SystemExit(f"child failed ({r.returncode})")
        out["runs"][kind] = json.loads(r.stdout.strip().splitlines()[-1])
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps({k: [(g["tenants"], g["each"]["ms"], g["loop"]["ms"]) for g in v["legs"]] for k, v in out["runs"].items()}))


if __name__ == "__main__":
    main()
