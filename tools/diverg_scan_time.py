#!/usr/bin/env python3
"""Time the exact scan over the divergence spaces (not part of bench.py).

Workload: 1M histograms of 128 positive entries that sum to 1, 1024 queries of the same kind, k = 10; kldivfast,
itakurasaitofast and jsdivfast, and the dense l1 scan at the same shape as a yardstick (two vector-ALU instructions per
element, like KL).  One batch = 1024 queries through nmslib_knn_query_batch (host buffers): the figure is the median
wall time of `--reps` warm batches, host packing, both PCIe copies and the merge included, beside the mean of the
HIP-event time of the scan + merge alone.

Every measurement runs in a fresh child process under its own time limit.  There is no reference figure: the
reference's C ABI cannot add a row to these spaces (tests/golden/gen_golden_diverg.py), so its seq_search cannot be
run over them.

    python3 tools/diverg_scan_time.py [--rows 1000000] [--dim 128] [--reps 20] [--out result.json]

--compare ROUNDS times the bf16 MFMA filter path of kldivfast and itakurasaitofast and the hardware-log2
filter path of jsdivfast and jsmetrfast (4.11b; --spaces picks a subset) against the exact scan in the same call: per space ROUNDS rounds, each one fresh process with NMSLIB_GPU_DIVERG_FAST=1 and then one with 0.
Every run records the path its batches took (last_path), the 16-query groups on the filter path and the share of them
the exact scan had to redo; the summary gives median and range per leg and says whether the filter wins by more than the
two legs' spread.  With --trace one more filter-path process per space runs under rocprofv3 --kernel-trace --stats (a run
of its own: tracing slows the host) and the time of a batch is split by kernel.  How full the lists must be is a CPU
question: tools/diverg_fast_sim.py.

    python3 tools/diverg_scan_time.py --compare 3 --trace --reps 10 --out profiles/diverg_fast_vs_scan.json
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPACES = ("kldivfast", "itakurasaitofast", "jsdivfast", "l1")
# the spaces --compare runs, and the last_path their filter reports: 14 = bf16 MFMA filter, 16 = hardware-log2 filter (4.11b)
FILTER_SPACES = ("kldivfast", "itakurasaitofast", "jsdivfast", "jsmetrfast")
FILTER_PATH = {"kldivfast": 14, "itakurasaitofast": 14, "jsdivfast": 16, "jsmetrfast": 16}
# diverg_js_filter_kernel's inner loop, one group of 4 elements against 16 queries: 32 v_pk_add + 64 v_log + 32 v_pk_fma + 5
JS_FILTER_VALU_PER_ELEMENT = 133 / 64
# Vector-ALU wave instructions per (row element, query) in the inner loop of diverg_knn_kernel<.., 16>, counted in its
# gfx950 code: the loop body serves one group of 4 elements against 16 queries, 64 pairs, and holds
#   kldivfast        64 v_sub + 32 v_pk_mul + 32 v_pk_add + 6 moves / address adds              = 134
#   itakurasaitofast 128 v_sub + 32 v_pk_mul + 32 v_pk_add + 6                                  = 198
#   jsdivfast        1195 (one accurate logf per pair element: v_log_f32 with its scaling, selects and fix-up)
VALU_PER_ELEMENT = {"kldivfast": 134 / 64, "itakurasaitofast": 198 / 64, "jsdivfast": 1195 / 64}
# f32 operations of the formula per pair element (a logarithm counted as one)
FLOP_PER_ELEMENT = {"kldivfast": 3, "itakurasaitofast": 4, "jsdivfast": 9}
SIMDS, CLOCK_HZ = 256 * 4, 2.4e9
# A SIMD issues one wave64 vector instruction per 4 cycles (16 lanes a cycle), packed or not.
PEAK_WAVE_INSTR_PER_S = SIMDS * CLOCK_HZ / 4
# The 157 TF packed-f32 peak is that rate with every instruction a v_pk_fma_f32: 64 lanes x 2 elements x 2 operations.
PEAK_PACKED_F32_FLOPS = PEAK_WAVE_INSTR_PER_S * 64 * 2 * 2


def histograms(seed, n, dim):
    rng = np.random.default_rng(seed)
    x = rng.gamma(0.7, size=(n, dim)).astype(np.float32) + np.float32(1e-4)
    return x / x.sum(1, keepdims=True, dtype=np.float32)


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child(space, nrows, dim, reps, nq):
    import nmslib_zig_amd as nz
    X, Q = histograms(1, nrows, dim), histograms(2, nq, dim)
    idx = nz.Index(space, "seq_search")
    idx.addDenseBatch(X)
    idx.buildIndex()
    log(f"{space}: index built and uploaded ({idx.stats()['hbm_bytes'] >> 20} MiB in HBM)")
    for _ in range(3):
        idx.knnQueryBatch(Q, 10)                           # warm-up: code objects, workspaces, clocks
    idx.kernel_timing(enable=True)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        idx.knnQueryBatch(Q, 10)
        wall.append(time.perf_counter() - t0)
    kms, kn = idx.kernel_timing(enable=False, collect=True)
    st = idx.stats()
    idx.close()
    rec = {"space": space, "rows": nrows, "dim": dim, "batch": nq, "k": 10, "reps": reps,
           "batch_wall_ms_median": float(np.median(wall)) * 1e3, "batch_wall_ms_min": float(np.min(wall)) * 1e3,
           "method": "median wall time of warm nmslib_knn_query_batch calls (host buffers in and out)"}
    if kn:
        rec["scan_gpu_ms_mean"] = kms / kn * max(1, kn // reps)
        rec["scan_gpu_method"] = "HIP events around the scan and merge launches of a batch, mean over the same batches"
    rec["last_path"] = int(st["last_path"])
    if st["last_path"] in (14, 16):      # a filter path: 16-query groups it served, and those the exact scan redid
        rec["hbm_mib"] = int(st["hbm_bytes"]) >> 20
        rec["fast_tiles"], rec["fast_tiles_fallback"] = int(st["fast_tiles"]), int(st["fast_tiles_fallback"])
        rec["fallback_share"] = rec["fast_tiles_fallback"] / max(1, rec["fast_tiles"])
        if st["last_path"] == 16 and kn:      # (an upper figure: the batch's time holds the re-rank and the proof too)
            rec["filter_valu_instr_per_element"] = JS_FILTER_VALU_PER_ELEMENT
            rec["v_log_f32_per_s_lower_bound"] = float(nrows) * dim * nq / (rec["scan_gpu_ms_mean"] * 1e-3)
    elif space in VALU_PER_ELEMENT and kn:      # (figures of the exact scan's inner loop: for runs that ran it)
        pairs_el, sec = float(nrows) * dim * nq, rec["scan_gpu_ms_mean"] * 1e-3
        rec["valu_instr_per_element"] = VALU_PER_ELEMENT[space]
        # share of the chip's vector-instruction issue slots the inner loop's instructions fill (1 = VALU-bound)
        rec["valu_issue_fraction"] = VALU_PER_ELEMENT[space] * pairs_el / 64 / sec / PEAK_WAVE_INSTR_PER_S
        # the formula's own f32 operations against the 157 TF packed-f32 peak
        rec["fraction_of_packed_f32_peak"] = FLOP_PER_ELEMENT[space] * pairs_el / sec / PEAK_PACKED_F32_FLOPS
    return rec


def run_child(a, space, fast=None, reps=None, wrap=()):
    env = dict(os.environ)
    if fast is not None:
        env["NMSLIB_GPU_DIVERG_FAST"] = str(fast)
    r = subprocess.run([*wrap, sys.executable, os.path.abspath(__file__), "--child", "--space", space, "--rows", str(a.rows),
                        "--dim", str(a.dim), "--reps", str(reps or a.reps), "--batch", str(a.batch)],
                       stdout=subprocess.PIPE, text=True, timeout=a.timeout, env=env)
    if r.returncode != 0:      # nothing more is started on the device after a failure
        raise SystemExit(f"{space}: child failed ({r.returncode})")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])   # (a tracer may print after it)


def kernel_split(a, space, outdir):
    """one filter-path process under the kernel trace -> per kernel: calls, mean and total time; 3 warm-up + 3 batches"""
    d = os.path.join(outdir, f"trace_{space}")
    run_child(a, space, fast=1, reps=3, wrap=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "t", "--"))
    found = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        raise SystemExit(f"{space}: the trace left no kernel statistics under {d}")
    rows = []
    with open(found[0]) as f:
        for r in csv.DictReader(f):
            rows.append({"kernel": r["Name"].replace("(anonymous namespace)::", "").split("(")[0].removeprefix("void "), "calls": int(r["Calls"]),
                         "mean_ms": float(r["AverageNs"]) * 1e-6, "total_ms": float(r["TotalDurationNs"]) * 1e-6})
    return {"space": space, "batches": 6, "kernels": sorted(rows, key=lambda r: -r["total_ms"])}


def compare(a):
    """the filter path against the exact scan: alternating fresh processes, then the verdict"""
    runs, doc = [], {}
    spaces = tuple(a.spaces.split(",")) if a.spaces else FILTER_SPACES
    for space in spaces:
        for rnd in range(a.compare):
            for fast in (1, 0):
                rec = run_child(a, space, fast=fast)
                rec["fast"], rec["round"] = fast, rnd
                if rec["last_path"] != (FILTER_PATH[space] if fast else 0):
                    raise SystemExit(f"{space}: NMSLIB_GPU_DIVERG_FAST={fast} ran path {rec['last_path']}")
                runs.append(rec)
                print(json.dumps(rec), flush=True)
    summary = []
    for space in spaces:
        leg = {}
        for fast in (1, 0):
            mine = [r for r in runs if r["space"] == space and r["fast"] == fast]
            g = [r["scan_gpu_ms_mean"] for r in mine]
            leg[fast] = {"gpu_ms_median": float(np.median(g)), "gpu_ms_min": min(g), "gpu_ms_max": max(g),
                         "wall_ms_median": float(np.median([r["batch_wall_ms_median"] for r in mine]))}
        on = [r for r in runs if r["space"] == space and r["fast"] == 1]
        spread = max(leg[1]["gpu_ms_max"] - leg[1]["gpu_ms_min"], leg[0]["gpu_ms_max"] - leg[0]["gpu_ms_min"])
        summary.append({"space": space, "filter": leg[1], "exact_scan": leg[0], "spread_ms": spread,
                        "filter_wins": leg[0]["gpu_ms_median"] - leg[1]["gpu_ms_median"] > spread,
                        "fast_tiles": on[0]["fast_tiles"], "fallback_share_max": max(r["fallback_share"] for r in on)})
        print(json.dumps(summary[-1]), flush=True)
    doc = {"method": "per space and round one fresh process with NMSLIB_GPU_DIVERG_FAST=1, then one with 0; GPU ms = HIP events "
                     "around a batch's kernels, mean over the run's warm batches; median and range over the rounds",
           "summary": summary, "runs": runs}
    if a.trace:
        outdir = os.path.dirname(os.path.abspath(a.out)) if a.out else os.getcwd()
        doc["kernel_split"] = [kernel_split(a, space, a.trace_dir or outdir) for space in spaces]
        for ks in doc["kernel_split"]:
            print(json.dumps(ks), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--space", default=None)
    ap.add_argument("--compare", type=int, default=0, metavar="ROUNDS")
    ap.add_argument("--spaces", default=None, help="--compare: a comma-separated subset of " + ",".join(FILTER_SPACES))
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--trace-dir", default=None)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.space, a.rows, a.dim, a.reps, a.batch)))
        return
    if a.compare:
        compare(a)
        return
    out = []
    for space in SPACES:
        out.append(run_child(a, space))
        print(json.dumps(out[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
