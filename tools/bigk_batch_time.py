#!/usr/bin/env python3
"""Time exact k-NN for 512 < k <= 4096 on the batched scan against the per-query sort it replaces (not part
of bench.py).

Workload: one brute_force index of 1M x 128 rows per space -- l2 on s_lowrank, l2sqr_sift on s_sift_like
(nmslib_zig_amd/datasets.py) -- k = 1000 and 4096, Q in 1, 4, 16, 64, 1024 queries from the same generator.  Two routes of
the same index in the same process: the batched kernels (last_path 12, the batch gate opened with
NMSLIB_GPU_BIGK_MIN_QUERIES=1 so that every Q takes them) and NMSLIB_GPU_BIGK_BATCH=0 (last_path 5), which is the code
this route was added to and therefore the yardstick.  A leg is one call of the device entry between two HIP events on a
stream of its own; queries and results stay in HBM.  After one warm-up call per route the routes alternate for `--legs`
legs each; the median, the smallest and the largest leg are kept.  Before the timing the two routes are checked to give
the same ids, distance bits and counts.  A route whose single call would take longer than --loop-limit-ms by its
per-query time is timed on its first 64 queries and scaled (marked "scaled").
Every space runs in a child process of its own under a time limit; after a failure nothing more is started on the device.

    python3 tools/bigk_batch_time.py [--rows 1000000] [--legs 5] [--out profiles/bigk_batch_vs_loop.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIM = 128
SPACES = ("l2", "l2sqr_sift")
QUERIES = (1, 4, 16, 64, 1024)
KS = (1000, 4096)


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child(space, nrows, legs, queries, loop_limit_ms):
    sys.path.insert(0, ROOT)
    import torch
    import nmslib_zig_amd as nz
    from nmslib_zig_amd.datasets import s_lowrank, s_sift_like
    os.environ["NMSLIB_GPU_BIGK_MIN_QUERIES"] = "1"
    u8 = space == "l2sqr_sift"
    nq_max = max(queries)
    X, Q = (s_sift_like(nrows, 42), s_sift_like(nq_max, 43)) if u8 else (s_lowrank(nrows, DIM, 42), s_lowrank(nq_max, DIM, 43))
    idx = nz.Index(space, "brute_force", data_type="DenseUInt8Vector" if u8 else "DenseVector", dist_type="Int" if u8 else "Float")
    (idx.addUInt8Batch if u8 else idx.addDenseBatch)(X, np.arange(nrows, dtype=np.int32))
    idx.buildIndex()
    idx.finalize()
    stream = torch.cuda.Stream()
    dq = torch.from_numpy(Q).cuda()
    torch.cuda.synchronize()

    def call(nq, k, batched, out):
        """-> ms between two events around one device entry"""
        os.environ["NMSLIB_GPU_BIGK_BATCH"] = "1" if batched else "0"
        ids, ds, cnt = out
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            t0.record()
            idx.knn_device(dq.data_ptr(), nq, DIM, k, ids.data_ptr(), ds.data_ptr(), cnt.data_ptr(), stream.cuda_stream)
            t1.record()
        stream.synchronize()
        return t0.elapsed_time(t1)

    def stats(ms):
        return {"ms": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}

    cases = []
    for k in KS:
        for nq in queries:
            outs = [(torch.empty(nq * k, dtype=torch.int32, device="cuda"), torch.empty(nq * k, dtype=torch.float32, device="cuda"),
                     torch.empty(nq, dtype=torch.int32, device="cuda")) for _ in range(2)]
            nq_loop = nq
            rec = {"k": k, "queries": nq}
            warm_batch = call(nq, k, True, outs[0])
            rec["last_path"] = int(idx.stats()["last_path"])
            rec["redone"] = int(idx.stats()["fast_tiles_fallback"])
            probe = call(min(nq, 4), k, False, outs[1]) / min(nq, 4)
            if probe * nq > loop_limit_ms:
                nq_loop = 64
            call(nq_loop, k, False, outs[1])
            rec["loop_path"] = int(idx.stats()["last_path"])
            same = all(bool((a[:nq_loop * (k if i < 2 else 1)].view(torch.int32) == b[:nq_loop * (k if i < 2 else 1)].view(torch.int32)).all())
                       for i, (a, b) in enumerate(zip(outs[0], outs[1])))
            rec["same_ids_bits_and_counts"] = same
            if not same or rec["last_path"] != 12 or rec["loop_path"] != 5:
                raise SystemExit(f"routes disagree or did not run: {rec}")
            t_batch, t_loop = [], []
            for _ in range(legs):
                t_batch.append(call(nq, k, True, outs[0]))
                t_loop.append(call(nq_loop, k, False, outs[1]) * (nq / nq_loop))
            rec.update(batch=stats(t_batch), loop=stats(t_loop), loop_scaled_from=nq_loop if nq_loop != nq else None,
                       first_batch_call_ms=warm_batch)
            rec["loop_over_batch"] = rec["loop"]["ms"] / rec["batch"]["ms"]
            cases.append(rec)
            log(f"{space} k={k} Q={nq}: batch {rec['batch']['ms']:.3f} ms, loop {rec['loop']['ms']:.3f} ms"
                f"{' (scaled)' if nq_loop != nq else ''}, x{rec['loop_over_batch']:.1f}, redone {rec['redone']}")
    idx.close()
    return {"space": space, "shape": f"{nrows} x {DIM}", "legs": legs, "device": torch.cuda.get_device_name(0), "cases": cases}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=280)
    ap.add_argument("--loop-limit-ms", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--spaces", default=",".join(SPACES))
    ap.add_argument("--queries", default=",".join(str(q) for q in QUERIES))
    ap.add_argument("--child", default=None, choices=SPACES)
    a = ap.parse_args()
    queries = tuple(int(q) for q in a.queries.split(","))
    if a.child:
        print(json.dumps(child(a.child, a.rows, a.legs, queries, a.loop_limit_ms)))
        return
    out = {"tool": "tools/bigk_batch_time.py", "date": time.strftime("%Y-%m-%d"),
           "method": "ms: HIP events around one call of the device entry; the routes alternate, median / smallest / largest of "
                     "the legs; one run", "runs": {}}
    for space in a.spaces.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", space, "--rows", str(a.rows), "--legs", str(a.legs),
               "--queries", a.queries, "--loop-limit-ms", str(a.loop_limit_ms)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if r.returncode != 0:      # nothing more is started on the device after a failure
            raise SystemExit(f"child failed ({r.returncode})")
        out["runs"][space] = json.loads(r.stdout.strip().splitlines()[-1])
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps({s: [(c["k"], c["queries"], round(c["batch"]["ms"], 3), round(c["loop"]["ms"], 3)) for c in v["cases"]]
                      for s, v in out["runs"].items()}))


if __name__ == "__main__":
    main()
