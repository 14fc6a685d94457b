#!/usr/bin/env python3
"""Time the bit_jaccard matrix-core scan (last_path 18) against the bit_jaccard scan kernel (NMSLIB_GPU_JAC_FAST=0), with
bit_hamming's XOR-popcount scan over the same rows beside them as the yardstick for the row stream.

The rows of tools/string_scan_time.py: 1M rows of 256, 1024 and 2048 uniform random bits, one batch of 1024 queries,
k = 10, 16, 32 and 64.  Per width, in one process: a warm-up of every leg, then the legs alternated --reps times; a leg's figure
is the kernel time of its batch (scans + merges, HIP events around them).  The two bit_jaccard legs' results are compared
byte for byte.  "path" is the last_path of the switched-on leg: 18 where the plan (jac_fast_plan.hpp) serves the cell, 0 where
it does not -- the cell is then marked "served": false, both bit_jaccard legs ran the scan kernel, and "wins" and
"int8_peak_share" are null.  --force switches the path on with NMSLIB_GPU_JAC_FAST=2, which lifts the plan's k gate to the
kernel's limit (k <= 64), so that the cells the gate cuts out can be timed on path 18 as well.  "int8_peak_share" is 2 n nq bits over the kernel time against 5 POP/s.

    python3 tools/jac_fast_time.py [--rows 1000000] [--reps 5] [--ks 10,16,32,64] [--force] [--out profiles/jac_fast_vs_scan.json]
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


def leg(idx, qstr, k, env, on):
    """-> kernel ms, the result's bytes, last_path"""
    os.environ[env] = on
    idx.kernel_timing(enable=True)
    got = idx.knnQueryBatch(qstr, k)
    ms, _ = idx.kernel_timing(enable=False, collect=True)
    return ms, b"".join(a.tobytes() for a in got), idx.stats()["last_path"]


def measure(jac, ham, qstr, bits, nrows, nq, k, reps, force):
    legs = {"new": (jac, "NMSLIB_GPU_JAC_FAST", "2" if force else "1"), "off": (jac, "NMSLIB_GPU_JAC_FAST", "0"),
            "ham_xor": (ham, "NMSLIB_GPU_HAM_FAST", "0")}
    warm = {name: leg(idx, qstr, k, env, on) for name, (idx, env, on) in legs.items()}
    path = warm["new"][2]
    assert path in (0, 18) and warm["off"][2] == 0 and warm["ham_xor"][2] == 0, {n: w[2] for n, w in warm.items()}
    served = path == 18
    ms = {name: [] for name in legs}
    for _ in range(reps):
        for name, (idx, env, on) in legs.items():
            ms[name].append(leg(idx, qstr, k, env, on)[0])
    spread = lambda v: max(v) - min(v)   # noqa: E731
    med = float(np.median(ms["new"]))
    return {"bits": bits, "rows": nrows, "batch": nq, "k": k, "reps": reps, "forced": force, "path": path, "served": served,
            "same_bytes": warm["new"][1] == warm["off"][1],
            "new_ms": ms["new"], "off_ms": ms["off"], "ham_xor_ms": ms["ham_xor"],
            "new_ms_median": med, "new_spread_ms": spread(ms["new"]),
            "off_ms_min": min(ms["off"]), "off_ms_median": float(np.median(ms["off"])), "off_spread_ms": spread(ms["off"]),
            "ham_xor_ms_median": float(np.median(ms["ham_xor"])),
            "wins": med < min(ms["off"]) - max(spread(ms["new"]), spread(ms["off"])) if served else None,
            "int8_peak_share": 2.0 * nrows * nq * bits / (med * 1e-3) / INT8_PEAK if served else None}


def indexes_of(bits, nrows, nq):
    import nmslib_zig_amd as nz
    name = f"bit_hamming_{bits}"   # string_scan_time's generator: the width is the name's suffix
    out = []
    for space, dist in (("bit_jaccard", "Float"), ("bit_hamming", "Int")):
        idx = nz.Index(space, "seq_search", data_type="ObjectAsString", dist_type=dist)
        sst.add_rows(nz.lib(), idx.h, name, nrows)
        idx.buildIndex()
        out.append(idx)
    return out[0], out[1], [bytes(r).split(b"\0", 1)[0] for r in sst.queries(name, nq)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bits", default="256,1024,2048")
    ap.add_argument("--ks", default="10,16,32,64")
    ap.add_argument("--force", action="store_true", help="NMSLIB_GPU_JAC_FAST=2: time path 18 outside the plan's k gate too")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for bits in (int(b) for b in a.bits.split(",")):
        jac, ham, qstr = indexes_of(bits, a.rows, a.batch)
        for k in (int(v) for v in a.ks.split(",")):
            out.append(measure(jac, ham, qstr, bits, a.rows, a.batch, k, a.reps, a.force))
            print(json.dumps(out[-1]), flush=True)
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(out, f, indent=1)
        jac.close()
        ham.close()


if __name__ == "__main__":
    main()
