#!/usr/bin/env python3
"""Time the bit_hamming matrix-core scan (last_path 17) against the XOR-popcount scan (NMSLIB_GPU_HAM_FAST=0).

The workloads of tools/string_scan_time.py: 1M rows of 256 and of 1024 uniform random bits, one batch of 1024 queries,
k = 10.  Per width, in one process: a warm-up of both legs, then the legs alternated --reps times; a leg's figure is the
kernel time of its batch (scan + merge, HIP events around them).  The switch-off leg runs the kernels the path leaves
untouched.  Both legs' results are compared byte for byte.  "int8_peak_share" is 2 n nq bits over the kernel time
against 5 POP/s.

    python3 tools/ham_fast_time.py [--rows 1000000] [--reps 5] [--ks 10] [--out profiles/ham_fast_vs_scan.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import string_scan_time as sst   # noqa: E402

INT8_PEAK = 5e15


def leg(idx, qstr, k, fast):
    os.environ["NMSLIB_GPU_HAM_FAST"] = "1" if fast else "0"
    idx.kernel_timing(enable=True)
    got = idx.knnQueryBatch(qstr, k)
    ms, _ = idx.kernel_timing(enable=False, collect=True)
    assert idx.stats()["last_path"] == (17 if fast else 0)
    return ms, b"".join(a.tobytes() for a in got)


def measure(idx, qstr, bits, nrows, nq, k, reps):
    same = leg(idx, qstr, k, True)[1] == leg(idx, qstr, k, False)[1]   # the warm-up of both
    new, off = [], []
    for _ in range(reps):
        new.append(leg(idx, qstr, k, True)[0])
        off.append(leg(idx, qstr, k, False)[0])
    spread = lambda v: max(v) - min(v)   # noqa: E731
    med = float(np.median(new))
    return {"bits": bits, "rows": nrows, "batch": nq, "k": k, "reps": reps, "same_bytes": same,
            "new_ms": new, "off_ms": off, "new_ms_median": med, "new_spread_ms": spread(new),
            "off_ms_min": min(off), "off_ms_median": float(np.median(off)), "off_spread_ms": spread(off),
            "wins": med < min(off) - max(spread(new), spread(off)),
            "int8_peak_share": 2.0 * nrows * nq * bits / (med * 1e-3) / INT8_PEAK}


def index_of(bits, nrows, nq):
    import nmslib_zig_amd as nz
    name = f"bit_hamming_{bits}"
    idx = nz.Index("bit_hamming", "seq_search", data_type="ObjectAsString", dist_type="Int")
    sst.add_rows(nz.lib(), idx.h, name, nrows)
    idx.buildIndex()
    qstr = [bytes(r).split(b"\0", 1)[0] for r in sst.queries(name, nq)]
    return idx, qstr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bits", default="256,1024")
    ap.add_argument("--ks", default="10")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for bits in (int(b) for b in a.bits.split(",")):
        idx, qstr = index_of(bits, a.rows, a.batch)
        for k in (int(v) for v in a.ks.split(",")):
            out.append(measure(idx, qstr, bits, a.rows, a.batch, k, a.reps))
            print(json.dumps(out[-1]), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
        idx.close()


if __name__ == "__main__":
    main()
