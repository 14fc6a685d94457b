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

SPACES = ("kldivfast", "itakurasaitofast", "jsdivfast", "l1")
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
    idx.close()
    rec = {"space": space, "rows": nrows, "dim": dim, "batch": nq, "k": 10, "reps": reps,
           "batch_wall_ms_median": float(np.median(wall)) * 1e3, "batch_wall_ms_min": float(np.min(wall)) * 1e3,
           "method": "median wall time of warm nmslib_knn_query_batch calls (host buffers in and out)"}
    if kn:
        rec["scan_gpu_ms_mean"] = kms / kn * max(1, kn // reps)
        rec["scan_gpu_method"] = "HIP events around the scan and merge launches of a batch, mean over the same batches"
    if space in VALU_PER_ELEMENT and kn:
        pairs_el, sec = float(nrows) * dim * nq, rec["scan_gpu_ms_mean"] * 1e-3
        rec["valu_instr_per_element"] = VALU_PER_ELEMENT[space]
        # share of the chip's vector-instruction issue slots the inner loop's instructions fill (1 = VALU-bound)
        rec["valu_issue_fraction"] = VALU_PER_ELEMENT[space] * pairs_el / 64 / sec / PEAK_WAVE_INSTR_PER_S
        # the formula's own f32 operations against the 157 TF packed-f32 peak
        rec["fraction_of_packed_f32_peak"] = FLOP_PER_ELEMENT[space] * pairs_el / sec / PEAK_PACKED_F32_FLOPS
    return rec


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
    a = ap.parse_args()
    if a.child:
        print(json.dumps(child(a.space, a.rows, a.dim, a.reps, a.batch)))
        return
    out = []
    for space in SPACES:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--space", space, "--rows",
                            str(a.rows), "--dim", str(a.dim), "--reps", str(a.reps), "--batch", str(a.batch)],
                           stdout=subprocess.PIPE, text=True, timeout=a.timeout)
        if r.returncode != 0:      # nothing more is started on the device after a failure
            raise SystemExit(f"{space}: child failed ({r.returncode})")
        out.append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps(out[-1]), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
