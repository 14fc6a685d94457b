#!/usr/bin/env python3
"""Time the exact string scans (not part of bench.py).

Workloads, one batch = 1024 queries through nmslib_knn_query_batch (host buffers, the reference's slot layout):
  leven        : 1M rows of random lowercase strings, lengths uniform in [8, 64]; queries of 32 bytes (the C ABI's batch
                 gives every query of one call the same length); k = 10, and range search at radius 12.
  bit_hamming  : 1M rows of 256 bits and 1M rows of 1024 bits, uniform random; k = 10, and range search at radius
                 bits/2 - 3 * sqrt(bits)/2 (about 0.1 % of the rows).
Range search serves one query per call: the figure is the time of 1024 calls.

Every GPU measurement runs in a fresh child process under its own time limit.  The reference's seq_search
(oracle/_ref/libnmslib_ref.so, its C ABI, one thread) is timed on a row subsample and a few queries and extrapolated
linearly to the full workload -- labelled "subsample, extrapolated".

The bit_hamming scan reads every row once per tile of 8 queries: "row_stream_TBps" is that traffic (rows x tiles)
over the measured kernel time, and "fraction_of_hbm_peak" divides it by 8 TB/s.  Repeated reads of a row may be
served by the L2 / MALL, so the fraction is of the stream the kernel issues, not of DRAM traffic.

    python3 tools/string_scan_time.py [--rows 1000000] [--ref-rows 20000] [--ref-queries 8] [--out result.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBPS = 8.0
WORKLOADS = ("leven", "bit_hamming_256", "bit_hamming_1024")
CHUNK = 65536


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def leven_texts(seed, n, lo, hi):
    """-> [n][hi + 1] uint8 buffer of NUL-terminated strings (lowercase letters, length uniform in [lo, hi])"""
    rng = np.random.default_rng(seed)
    buf = rng.integers(97, 123, size=(n, hi + 1), dtype=np.uint8)
    lens = rng.integers(lo, hi + 1, size=n)
    buf[np.arange(hi + 1)[None, :] >= lens[:, None]] = 0
    return buf


def bit_texts(seed, n, bits):
    """-> [n][2 * bits + 1] uint8 buffer of NUL-terminated texts "b b b ..." """
    rng = np.random.default_rng(seed)
    buf = np.full((n, 2 * bits + 1), 32, np.uint8)
    buf[:, 0:2 * bits:2] = rng.integers(0, 2, size=(n, bits), dtype=np.uint8) + 48
    buf[:, -1] = 0
    return buf


def workload(name, n, seed):
    if name == "leven":
        return leven_texts(seed, n, 8, 64)
    return bit_texts(seed, n, int(name.rsplit("_", 1)[1]))


def queries(name, nq):
    if name == "leven":
        return leven_texts(99, nq, 32, 32)
    return bit_texts(99, nq, int(name.rsplit("_", 1)[1]))


def radius(name):
    if name == "leven":
        return 12.0
    bits = int(name.rsplit("_", 1)[1])
    return float(int(bits / 2 - 1.5 * bits ** 0.5))


def add_rows(L, h, name, nrows):
    """the rows, generated and added CHUNK at a time (chunk c from seed (1, c)): one
    nmslib_add_data_point_batch_string call per chunk"""
    for lo in range(0, nrows, CHUNK):
        m = min(CHUNK, nrows - lo)
        buf = workload(name, m, (1, lo // CHUNK))
        w = buf.shape[1]
        ptrs = (C.c_void_p * m)(*[buf.ctypes.data + i * w for i in range(m)])
        assert L.nmslib_add_data_point_batch_string(h, C.cast(ptrs, C.c_void_p), m, None) == 0


def child_gpu(name, nrows, reps, nq):
    import nmslib_zig_amd as nz
    Q = queries(name, nq)
    space = "leven" if name == "leven" else "bit_hamming"
    idx = nz.Index(space, "seq_search", data_type="ObjectAsString", dist_type="Int")
    add_rows(nz.lib(), idx.h, name, nrows)
    idx.buildIndex()
    qstr = [bytes(r).split(b"\0", 1)[0] for r in Q]
    t0 = time.perf_counter()
    idx.knnQueryBatch(qstr[:8], 10)                        # upload and code objects
    log(f"{name}: index uploaded, warm-up {time.perf_counter() - t0:.3f} s")
    idx.kernel_timing(enable=True)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        idx.knnQueryBatch(qstr, 10)
        wall.append(time.perf_counter() - t0)
        log(f"{name}: k-NN batch of {nq} queries {wall[-1] * 1e3:.2f} ms")
    kms, kn = idx.kernel_timing(enable=False, collect=True)
    r = radius(name)
    t0 = time.perf_counter()
    found = 0
    for q in qstr:
        found += len(idx.rangeQueryFill(q, r, 100000)[0])
    range_s = time.perf_counter() - t0
    log(f"{name}: {nq} range queries at radius {r}: {range_s * 1e3:.1f} ms, {found / nq:.1f} rows each")
    idx.close()
    rec = {"workload": name, "rows": nrows, "batch": nq, "k": 10, "reps": reps,
           "knn_batch_wall_ms_median": float(np.median(wall)) * 1e3,
           "knn_batch_gpu_ms_mean": kms / reps,
           "range_radius": r, "range_batch_wall_ms": range_s * 1e3, "range_mean_results": found / nq}
    if name != "leven":
        bits = int(name.rsplit("_", 1)[1])
        stream = nrows * (bits // 8) * ((nq + 7) // 8)
        tbps = stream / (rec["knn_batch_gpu_ms_mean"] * 1e-3) / 1e12
        rec.update({"row_stream_TBps": tbps, "fraction_of_hbm_peak": tbps / HBM_PEAK_TBPS})
    return rec


def child_ref(name, ref_rows, ref_queries, nrows, nq):
    from tests.golden import gen_golden_strings as gs
    X = workload(name, CHUNK, (1, 0))[:ref_rows]           # the first rows of the GPU workload
    Q = queries(name, ref_queries)
    L = gs.ref_lib()
    rows = [bytes(r).split(b"\0", 1)[0] for r in X]
    ix = gs.RefIndex(L, "leven" if name == "leven" else "bit_hamming", rows)
    ix.n = 10                                               # knn_all asks for ix.n results
    t0 = time.perf_counter()
    for q in Q:
        ix.knn_all(bytes(q).split(b"\0", 1)[0])
    per_query = (time.perf_counter() - t0) / ref_queries
    ix.close()
    return {"ref_rows_measured": ref_rows, "ref_queries_measured": ref_queries,
            "ref_s_per_query_measured": per_query,
            "ref_ms_per_batch_subsample_extrapolated": per_query * nrows / ref_rows * nq * 1e3,
            "ref_note": "reference: one thread, seq_search, k = 10; subsample, extrapolated linearly in rows and queries"}


def run_child(args, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True,
                       timeout=timeout)
    if r.returncode != 0:
        raise SystemExit(f"child {args} failed ({r.returncode})")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--ref-rows", type=int, default=20000)
    ap.add_argument("--ref-queries", type=int, default=8)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", choices=["gpu", "ref"], default=None)
    ap.add_argument("--workload", default=None)
    ap.add_argument("--only", default=None, help="comma-separated subset of " + ",".join(WORKLOADS))
    ap.add_argument("--no-ref", action="store_true")
    a = ap.parse_args()
    if a.child == "gpu":
        print(json.dumps(child_gpu(a.workload, a.rows, a.reps, a.batch)))
        return
    if a.child == "ref":
        print(json.dumps(child_ref(a.workload, a.ref_rows, a.ref_queries, a.rows, a.batch)))
        return
    out = []
    for name in (a.only.split(",") if a.only else WORKLOADS):
        rec = run_child(["--child", "gpu", "--workload", name, "--rows", str(a.rows), "--reps", str(a.reps),
                         "--batch", str(a.batch)], a.timeout)
        from tests import orc
        if not a.no_ref and os.path.exists(orc.REF_LIB):
            rec.update(run_child(["--child", "ref", "--workload", name, "--rows", str(a.rows), "--batch", str(a.batch),
                                  "--ref-rows", str(a.ref_rows), "--ref-queries", str(a.ref_queries)], a.timeout))
        out.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
