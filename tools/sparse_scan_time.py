#!/usr/bin/env python3
"""Time the exact sparse scan (not part of bench.py).

Workload: 1M rows, ids Zipf-distributed (a = 1.1) over a 2^20 vocabulary, Poisson(64) draws per row (the heavy head
repeats ids: about 49 distinct elements per row remain); 1024 queries of Poisson(32) draws; k = 10; cosinesimil_sparse and
l2_sparse; one batch = 1024 queries through nmslib_knn_query_batch (host buffers, the reference's slot layout).

Every GPU measurement runs in a fresh child process under its own time limit.  The reference's seq_search
(oracle/_ref/libnmslib_ref.so, its C ABI, one thread) is timed on a row subsample and a few queries and extrapolated
to the full workload -- the extrapolated figure is labelled as such.

    python3 tools/sparse_scan_time.py [--rows 1000000] [--ref-rows 20000] [--ref-queries 8] [--out result.json]
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

VOCAB = 1 << 20
SPACES = ("cosinesimil_sparse", "l2_sparse")


def zipf_csr(seed, n, mean_len, vocab=VOCAB, a=1.1):
    """n rows as a CSR triple: Poisson(mean_len) Zipf draws per row, kept below vocab, duplicates merged"""
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.poisson(mean_len, size=n), 1, None)
    total = int(lens.sum())
    ids = np.empty(0, np.int64)
    while len(ids) < total:
        d = rng.zipf(a, size=total) - 1
        ids = np.concatenate([ids, d[d < vocab]])
    ids = ids[:total]
    row = np.repeat(np.arange(n, dtype=np.int64), lens)
    key = np.unique(row * vocab + ids)                     # sorted by (row, id), duplicates merged
    row, ids = key // vocab, key % vocab
    indptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int64)
    vals = rng.uniform(-1, 1, size=len(ids)).astype(np.float32)
    return indptr, ids.astype(np.uint32), vals


def as_rows(csr, lo, hi):
    p, i, v = csr
    return [(i[p[r]:p[r + 1]], v[p[r]:p[r + 1]]) for r in range(lo, hi)]


def log(msg):
    print(f"[{time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def child_gpu(space, nrows, reps, nq):
    import nmslib_zig_amd as nz
    X = zipf_csr(1, nrows, 64)
    Q = zipf_csr(2, 1024, 32)
    qrows = as_rows(Q, 0, nq)
    log(f"{space}: data ready ({int(X[0][-1])} elements)")
    idx = nz.Index(space, "seq_search", data_type="SparseVector")
    idx.addSparseBatch(X)
    idx.buildIndex()
    log(f"{space}: index built and uploaded")
    t0 = time.perf_counter()
    idx.knnQueryBatch(qrows[:8], 10)                       # warm-up: code objects
    log(f"{space}: warm-up batch of 8 queries {time.perf_counter() - t0:.3f} s")
    idx.kernel_timing(enable=True)
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        idx.knnQueryBatch(qrows, 10)
        wall.append(time.perf_counter() - t0)
        log(f"{space}: batch of {nq} queries {wall[-1]:.3f} s")
    kms, kn = idx.kernel_timing(enable=False, collect=True)
    idx.close()
    return {"space": space, "rows": nrows, "nnz": int(X[0][-1]), "mean_row_len": float(X[0][-1] / nrows),
            "mean_query_len": float(Q[0][-1] / 1024), "batch": nq, "k": 10, "reps": reps,
            "batch_wall_s_median": float(np.median(wall)), "batch_gpu_s_mean": kms / 1e3 / max(kn, 1)}


def child_ref(space, nrows, ref_rows, ref_queries):
    from tests.golden import gen_golden_sparse as gs
    X = zipf_csr(1, nrows, 64)
    Q = zipf_csr(2, 1024, 32)
    L = gs.ref_lib()
    ix = gs.RefIndex(L, space, {}, as_rows(X, 0, ref_rows))
    qs = as_rows(Q, 0, ref_queries)
    t0 = time.perf_counter()
    ix.knn(qs, 10)
    per_query = (time.perf_counter() - t0) / ref_queries
    ix.close()
    per_query_full = per_query * nrows / ref_rows
    return {"space": space, "ref_rows_measured": ref_rows, "ref_queries_measured": ref_queries,
            "ref_s_per_query_measured": per_query,
            "ref_s_per_query_extrapolated": per_query_full,
            "ref_s_per_batch_extrapolated": per_query_full * 1024,
            "note": "reference: one thread, seq_search; extrapolated linearly in rows and queries"}


def run_child(args, timeout):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE, text=True,
                       timeout=timeout)                     # (the child's progress goes straight to stderr)
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
    ap.add_argument("--space", default=None)
    a = ap.parse_args()
    if a.child == "gpu":
        print(json.dumps(child_gpu(a.space, a.rows, a.reps, a.batch)))
        return
    if a.child == "ref":
        print(json.dumps(child_ref(a.space, a.rows, a.ref_rows, a.ref_queries)))
        return
    out = []
    for space in SPACES:
        rec = run_child(["--child", "gpu", "--space", space, "--rows", str(a.rows), "--reps", str(a.reps),
                         "--batch", str(a.batch)], a.timeout)
        from tests import orc
        if os.path.exists(orc.REF_LIB):
            rec.update(run_child(["--child", "ref", "--space", space, "--rows", str(a.rows), "--ref-rows",
                                  str(a.ref_rows), "--ref-queries", str(a.ref_queries)], a.timeout))
        out.append(rec)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
