#!/usr/bin/env python3
"""Time the in-walk filtered HNSW search (query-time parameter gpu_inwalk=1; not part of bench.py) against
the two-stage route it replaces.

Workload, as tools/filter_time.py: l2, 1M x 128 (s_lowrank of nmslib_zig_amd/datasets.py), one graph built on the GPU with
M=16, efSearch 128, k 10, batches of 1024 queries through the device entries.  Leg groups, each in a child process of its
own:

  filter   random filters that allow 50 %, 10 %, 1 % and 0.1 % of the rows
  delete   50 %, 90 % and 99 % of the rows deleted (nested sets), no filter
  control  the unfiltered batch on an index without tombstones, three times: the path gpu_inwalk does not touch

Per share, three legs: the two stages at efSearch 128; the in-walk search at efSearch 128; the two stages at the smallest
efSearch of 256 / 512 / 1024 / 2048 whose recall reaches the in-walk's (every efSearch tried is kept; "reached": null when
none does).  Per leg: `--warmup` batches, then `--reps` batches, each timed twice: nmslib_gpu_kernel_timing (HIP events
inside the engine around the dominant launches) and HIP events around the whole call on the caller's stream; the mean count,
recall@10 against an exact scan over an index of the eligible rows alone, the mean ndc, and the path the batch took
(4 = two stages, 7 = exact scan of the subset, 8 = in-walk).

With --parent-root (a checkout of the parent commit whose library is built) one more child imports that package and runs
the control group's first leg alone, in the same call; its time must lie within the spread of the three.  Every child is a
fresh process under its own time limit; after a failure nothing more is started on the device.

    python3 tools/inwalk_time.py [--rows 1000000] [--reps 30] [--parent-root DIR] [--out profiles/inwalk_time.json]
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
FILTER_SHARES = (0.5, 0.1, 0.01, 0.001)
DELETE_SHARES = (0.5, 0.9, 0.99)
EF_LADDER = (256, 512, 1024, 2048)
GROUPS = ("filter", "delete", "control")


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child(group, nrows, reps, warmup, parent_root):
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

    def exact(rows):
        bf = nz.Index(SPACE, "seq_search")
        bf.addDenseBatch(X[rows], rows.astype(np.int32))
        bf.buildIndex()
        gi, gd, _ = bf.knnQueryBatch(Q, 32)
        bf.close()
        return gi, gd ** 2

    def leg(idx, name, truth, flt, ef, inwalk, extra):
        idx.setQueryTimeParams(efSearch=ef, **({} if parent_root else {"gpu_inwalk": inwalk}))

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
        ctr = idx.read_counters(NQ)
        rec = {"leg": name, "efSearch": ef, "gpu_inwalk": inwalk, "last_path": int(idx.stats()["last_path"]),
               "kernel_ms": kms / max(reps, 1), "kernel_intervals": int(kn), "batch_ms": float(np.median(whole)),
               "batch_ms_min": float(whole.min()), "batch_ms_max": float(whole.max()), "count_mean": float(cnt.mean()),
               "count_min": int(cnt.min()), "recall_at_10": float(recall_nmslib(ids, truth[0], truth[1], K)),
               "ndc_mean": float(ctr[0].mean()) if ctr is not None else None}
        rec.update(extra)
        log(f"{group} {name}: ef {ef} inwalk {inwalk}: kernel {rec['kernel_ms']:.4f} ms, batch {rec['batch_ms']:.4f} ms, count "
            f"{rec['count_mean']:.2f}, recall {rec['recall_at_10']:.4f}, ndc {rec['ndc_mean']}, path {rec['last_path']}")
        return rec

    def three(idx, name, truth, flt, extra):
        """two stages and in-walk at EF_SEARCH, then the two stages up the ladder until they reach the in-walk's recall"""
        legs = [leg(idx, name, truth, flt, EF_SEARCH, 0, extra), leg(idx, name, truth, flt, EF_SEARCH, 1, extra)]
        reached = None
        for ef in EF_LADDER:
            legs.append(leg(idx, name, truth, flt, ef, 0, extra))
            if legs[-1]["recall_at_10"] >= legs[1]["recall_at_10"]:
                reached = ef
                break
        for g in legs:
            g["two_stage_ef_that_reaches_inwalk_recall"] = reached
        return legs

    all_ids = np.arange(nrows, dtype=np.int32)
    idx = nz.Index(SPACE, "hnsw")
    idx.addDenseBatch(X, all_ids)
    idx.buildIndex(M=M, efConstruction=EF_CONSTRUCTION, gpu_build=1)
    idx.finalize()
    build_seconds = idx.stats()["build_seconds"]
    legs = []
    if group == "control":
        truth_all = exact(np.arange(nrows))
        for i in range(1 if parent_root else 3):
            legs.append(leg(idx, f"unfiltered ({i + 1})", truth_all, None, EF_SEARCH, 1, {"eligible_share": 1.0}))
    elif group == "filter":
        for share in FILTER_SHARES:
            allowed = np.sort(order[:max(1, int(round(nrows * share)))])
            mask = np.zeros(nrows, bool)
            mask[allowed] = True
            flt = idx.makeFilter(mask)
            legs += three(idx, f"{share:.2%} allowed", exact(allowed), flt,
                          {"eligible_share": share, "eligible_rows": int(flt.allowed)})
            flt.close()
    else:
        for share in DELETE_SHARES:
            dead = order[:int(round(nrows * share))]
            idx.deleteIds(all_ids[dead])
            assert idx.deletedRows() == len(dead)
            live = np.sort(order[len(dead):])
            legs += three(idx, f"{share:.0%} deleted", exact(live), None,
                          {"eligible_share": 1.0 - share, "eligible_rows": int(len(live))})
    idx.close()
    return {"group": group, "shape": f"{nrows} x {DIM} {SPACE}", "M": M, "efConstruction": EF_CONSTRUCTION, "k": K,
            "batch": NQ, "reps": reps, "warmup": warmup, "build_seconds": build_seconds, "legs": legs}


def run_child(a, group, parent_root):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", group, "--rows", str(a.rows), "--reps", str(a.reps),
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
    ap.add_argument("--child", default=None, choices=GROUPS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.child, a.rows, a.reps, a.warmup, a.parent_root)))
        return
    out = {"tool": "tools/inwalk_time.py", "date": time.strftime("%Y-%m-%d"),
           "method": "kernel_ms: nmslib_gpu_kernel_timing (HIP events inside the engine), summed over the timed batches and "
                     "divided by their number; batch_ms: median of HIP events around the device entry on the caller's stream; "
                     "recall_at_10 against an exact scan over an index of the eligible rows alone; ndc_mean: the walk's distance "
                     "evaluations per query; legs in the order run",
           "runs": {}, "summary": {}}
    for group in GROUPS:
        out["runs"][group] = run_child(a, group, None)
        if a.out:                  # (what is measured so far survives a later child's failure)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    unf = [g["batch_ms"] for g in out["runs"]["control"]["legs"]]
    s = out["summary"] = {"unfiltered_batch_ms": unf, "unfiltered_batch_ms_spread": max(unf) - min(unf)}
    if a.parent_root:
        par = out["runs"]["control (parent)"] = run_child(a, "control", a.parent_root)
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
