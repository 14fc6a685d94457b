#!/usr/bin/env python3
"""Time the HNSW search on an index with deleted rows (nmslib_gpu_delete_ids; not part of bench.py).

Workload: l2, 1M x 128 (s_lowrank of nmslib_zig_amd/datasets.py), one graph built on the GPU with M=16, efSearch 128, k 10,
batches of 1024 queries through nmslib_gpu_knn_query_batch_device.  Legs, in the order run: no tombstones; 1 %, 10 % and
30 % of the rows deleted at random (cumulative: every set holds the one before it); then nmslib_reset_index, the same
rows and the same build again for two more legs without tombstones -- the spread of the three no-tombstone legs is known
before one of them is compared with the parent commit's.  Per leg: `--warmup` batches, then `--reps` batches, each timed
twice: nmslib_gpu_kernel_timing (HIP events inside the engine: the walk; with tombstones walk + overflow launch + filter)
and HIP events around the whole call on the caller's stream.  recall@10 of a leg is taken against the library's own exact
scan over the live rows, and beside it stands the same recall of a fresh graph built over the live rows only.

With --parent-root (a checkout of the parent commit whose library is built) one more child imports that package and runs
the no-tombstone leg alone, in the same call.  Every child is a fresh process under its own time limit; after a failure
nothing more is started on the device.

    python3 tools/hnsw_delete_time.py [--rows 1000000] [--reps 30] [--parent-root DIR] [--out profiles/hnsw_delete_vs_parent.json]
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
SHARES = (0.01, 0.10, 0.30)


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child(nrows, reps, warmup, parent_root):
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

    def exact(live):
        bf = nz.Index(SPACE, "seq_search")
        bf.addDenseBatch(X[live], live.astype(np.int32))
        bf.buildIndex()
        gi, gd, _ = bf.knnQueryBatch(Q, 32)
        bf.close()
        return gi, gd ** 2

    def graph(rows, ids):
        idx = nz.Index(SPACE, "hnsw")
        idx.addDenseBatch(rows, ids)
        idx.buildIndex(M=M, efConstruction=EF_CONSTRUCTION, gpu_build=1)
        idx.setQueryTimeParams(efSearch=EF_SEARCH)
        return idx

    def leg(idx, name, truth, extra):
        def batch():
            idx.knn_device(dq.data_ptr(), NQ, DIM, K, d_ids.data_ptr(), d_ds.data_ptr(), d_cnt.data_ptr(), stream)
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
        ndc = idx.read_counters(NQ)[0].astype(np.int64)
        st = idx.stats()
        rec = {"leg": name, "last_path": int(st["last_path"]), "hbm_bytes": int(st["hbm_bytes"]),
               "kernel_ms": kms / max(kn, 1), "kernel_intervals": int(kn), "batch_ms": float(np.median(whole)),
               "batch_ms_min": float(whole.min()), "batch_ms_max": float(whole.max()), "ndc": float(ndc.mean()),
               "count_mean": float(cnt.mean()), "count_min": int(cnt.min()),
               "recall_at_10": float(recall_nmslib(ids, truth[0], truth[1], K))}
        rec.update(extra)
        log(f"{name}: kernel {rec['kernel_ms']:.4f} ms, batch {rec['batch_ms']:.4f} ms, ndc {rec['ndc']:.0f}, "
            f"recall {rec['recall_at_10']:.4f} {extra}")
        return rec

    all_ids = np.arange(nrows, dtype=np.int32)
    truth_all = exact(np.arange(nrows))
    log("exact scan over all rows done")
    idx = graph(X, all_ids)
    build_seconds = idx.stats()["build_seconds"]
    legs = [leg(idx, "no tombstones", truth_all, {"deleted": 0})]
    if not parent_root:
        for share in SHARES:
            dead = order[:int(nrows * share)]
            live = np.sort(order[int(nrows * share):])
            t0 = time.perf_counter()
            marked = idx.deleteIds(dead.astype(np.int32))
            delete_seconds = time.perf_counter() - t0
            assert idx.deletedRows() == len(dead)
            truth = exact(live)
            fresh = graph(X[live], live.astype(np.int32))
            fresh.knn_device(dq.data_ptr(), NQ, DIM, K, d_ids.data_ptr(), d_ds.data_ptr(), d_cnt.data_ptr(), stream)
            torch.cuda.synchronize()
            fresh_recall = float(recall_nmslib(d_ids.cpu().numpy(), truth[0], truth[1], K))
            fresh.close()
            legs.append(leg(idx, f"{share:.0%} deleted", truth,
                            {"deleted": int(len(dead)), "newly_marked": int(marked), "delete_call_seconds": delete_seconds,
                             "recall_at_10_fresh_graph_over_live_rows": fresh_recall}))
        idx.reset()
        idx.addDenseBatch(X, all_ids)
        idx.buildIndex(M=M, efConstruction=EF_CONSTRUCTION, gpu_build=1)
        idx.setQueryTimeParams(efSearch=EF_SEARCH)
        assert idx.deletedRows() == 0
        for i in (2, 3):
            legs.append(leg(idx, f"no tombstones, after reset and rebuild ({i})", truth_all, {"deleted": 0}))
    idx.close()
    return {"shape": f"{nrows} x {DIM} {SPACE}", "M": M, "efConstruction": EF_CONSTRUCTION, "efSearch": EF_SEARCH, "k": K,
            "batch": NQ, "reps": reps, "warmup": warmup, "build_seconds": build_seconds, "legs": legs}


def run_child(a, parent_root):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--rows", str(a.rows), "--reps", str(a.reps), "--warmup",
           str(a.warmup)] + (["--parent-root", parent_root] if parent_root else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
    if r.returncode != 0:      # nothing more is started on the device after a failure
        raise SystemExit(f"child failed ({r.returncode})")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=540)
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit with its library built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.rows, a.reps, a.warmup, a.parent_root)))
        return
    out = {"tool": "tools/hnsw_delete_time.py", "date": time.strftime("%Y-%m-%d"),
           "method": "kernel_ms: nmslib_gpu_kernel_timing (HIP events inside the engine), mean over the timed batches; batch_ms: "
                     "median of HIP events around nmslib_gpu_knn_query_batch_device on the caller's stream; recall_at_10 "
                     "against the exact scan over the live rows; legs in the order run"}
    out["run"] = run_child(a, None)
    if a.parent_root:
        out["parent"] = run_child(a, a.parent_root)
    none = [g["kernel_ms"] for g in out["run"]["legs"] if g["deleted"] == 0]
    out["no_tombstone_kernel_ms_spread"] = max(none) - min(none)
    if a.parent_root:
        p = out["parent"]["legs"][0]["kernel_ms"]
        out["parent_kernel_ms"] = p
        out["no_tombstone_minus_parent_kernel_ms"] = [v - p for v in none]
        out["parent_within_the_spread"] = bool(min(none) - out["no_tombstone_kernel_ms_spread"] <= p <=
                                               max(none) + out["no_tombstone_kernel_ms_spread"])
    out["filter_cost_kernel_ms"] = {g["leg"]: g["kernel_ms"] - float(np.mean(none)) for g in out["run"]["legs"]
                                    if g["deleted"]}
    print(json.dumps({k: v for k, v in out.items() if k not in ("run", "parent")}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
