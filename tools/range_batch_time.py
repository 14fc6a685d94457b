#!/usr/bin/env python3
"""Time a batched range query against the loop of single range queries it replaces (not part of bench.py).

Workload: one brute_force index of 1M x 128 rows per space -- l2 and l1 on s_lowrank, l2sqr_sift on s_sift_like
(nmslib_zig_amd/datasets.py) -- and Q in 16, 256, 1024 queries from the same generator.  Every query gets its own radius
from its exact neighbours (one knnQueryBatch for k = 1001): the middle between its 10th and 11th, and between its 1000th and
1001st distance, so about 10 and about 1000 rows match.  Capacities 128 and 4096.  Two ways, in the same process:
  batch: one nmslib_gpu_range_query_batch call (host pointers in and out, copies included);
  loop : one nmslib_range_query_fill call per query into a result of the same capacity.
Both are host entries that return when the answer is in host memory, so a leg is wall-clock time around the calls.  After a
warm-up the two ways alternate for `--legs` legs each; the median, the smallest and the largest leg are kept.  Before the
timing the two ways are checked to give the same ids, distance bits and counts.
--single-only times the loop alone; with --package-root pointing at a checkout of another commit (built there) it shows
whether the single entry moved: the tool then needs nothing that commit does not have.
Every space runs in a child process of its own under a time limit; after a failure nothing more is started on the device.

    python3 tools/range_batch_time.py [--rows 1000000] [--legs 3] [--out profiles/range_batch_vs_loop.json]
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
SPACES = ("l2", "l1", "l2sqr_sift")
QUERIES = (16, 256, 1024)
MATCHES = (10, 1000)
CAPACITIES = (128, 4096)


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child(space, nrows, legs, single_only, package_root, queries):
    sys.path.insert(0, package_root)
    import nmslib_zig_amd as nz
    from nmslib_zig_amd.datasets import s_lowrank, s_sift_like
    u8 = space == "l2sqr_sift"
    nq_max = max(queries)
    X, Q = (s_sift_like(nrows, 42), s_sift_like(nq_max, 43)) if u8 else (s_lowrank(nrows, DIM, 42), s_lowrank(nq_max, DIM, 43))
    idx = nz.Index(space, "brute_force", data_type="DenseUInt8Vector" if u8 else "DenseVector", dist_type="Int" if u8 else "Float")
    (idx.addUInt8Batch if u8 else idx.addDenseBatch)(X, np.arange(nrows, dtype=np.int32))
    idx.buildIndex()
    idx.finalize()
    _, kd, _ = idx.knnQueryBatch(Q, max(MATCHES) + 1)
    radii = {m: (kd[:, m - 1].astype(np.float64) + kd[:, m].astype(np.float64)) / 2 for m in MATCHES}

    def wall(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    def stats(ms):
        return {"ms": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms))}

    out = []
    for nq in queries:
        for m in MATCHES:
            for cap in CAPACITIES:
                q, r = Q[:nq], radii[m][:nq]

                def loop():
                    return [idx.rangeQueryFill(q[i], r[i], cap) for i in range(nq)]

                def batch():
                    return idx.rangeQueryBatch(q, r, cap)

                rec = {"queries": nq, "matches_wanted": m, "capacity": cap}
                single = loop()                                        # (warms up, too)
                rec["matches_mean"] = float(np.mean([len(s[0]) for s in single]))
                if not single_only:
                    ids, ds, cnt, tot = batch()
                    same = all(cnt[i] == len(single[i][0]) and (ids[i, :cnt[i]] == single[i][0]).all() and
                               (ds[i, :cnt[i]].view(np.uint32) == single[i][1].view(np.uint32)).all() for i in range(nq))
                    rec.update(same_ids_bits_and_counts=bool(same), totals_mean=float(tot.mean()),
                               last_path=int(idx.stats()["last_path"]))
                    if not same:
                        raise SystemExit("the two ways disagree")
                t_loop, t_batch = [], []
                for _ in range(legs):
                    if not single_only:
                        t_batch.append(wall(batch)[0])
                    t_loop.append(wall(loop)[0])
                rec["loop"] = stats(t_loop)
                rec["loop_ms_per_query"] = rec["loop"]["ms"] / nq
                if not single_only:
                    rec["batch"] = stats(t_batch)
                    rec["loop_over_batch"] = rec["loop"]["ms"] / rec["batch"]["ms"]
                out.append(rec)
                log(f"{space} Q={nq} ~{m} matches cap {cap}: loop {rec['loop']['ms']:.2f} ms" +
                    ("" if single_only else f", batch {rec['batch']['ms']:.2f} ms, x{rec['loop_over_batch']:.1f}"))
    idx.close()
    return {"space": space, "shape": f"{nrows} x {DIM}", "legs": legs, "cases": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=280)
    ap.add_argument("--out", default=None)
    ap.add_argument("--spaces", default=",".join(SPACES))
    ap.add_argument("--queries", default=",".join(str(q) for q in QUERIES))
    ap.add_argument("--single-only", action="store_true", help="time the loop of single range queries alone")
    ap.add_argument("--package-root", default=ROOT, help="the checkout whose nmslib_zig_amd package (built) is timed")
    ap.add_argument("--child", default=None, choices=SPACES)
    a = ap.parse_args()
    queries = tuple(int(q) for q in a.queries.split(","))
    if a.child:
        print(json.dumps(child(a.child, a.rows, a.legs, a.single_only, os.path.abspath(a.package_root), queries)))
        return
    out = {"tool": "tools/range_batch_time.py", "date": time.strftime("%Y-%m-%d"),
           "method": "ms: wall-clock time around the host entries (they return with the answer in host memory); batch and loop "
                     "alternate, median / smallest / largest of the legs", "single_only": a.single_only, "runs": {}}
    for space in a.spaces.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", space, "--rows", str(a.rows), "--legs", str(a.legs),
               "--queries", a.queries, "--package-root", a.package_root] + (["--single-only"] if a.single_only else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if r.returncode != 0:      # nothing more is started on the device after a failure
            raise SystemExit(f"child failed ({r.returncode})")
        out["runs"][space] = json.loads(r.stdout.strip().splitlines()[-1])
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
    print(json.dumps({s: [(c["queries"], c["matches_wanted"], c["capacity"], round(c["loop"]["ms"], 2),
                           round(c.get("batch", {}).get("ms", 0), 2)) for c in v["cases"]] for s, v in out["runs"].items()}))


if __name__ == "__main__":
    main()
