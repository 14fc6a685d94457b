#!/usr/bin/env python3
"""How full must the lists of the divergence filter scan be?  A float64 simulation on the CPU.

The proof of a query holds when every split's list reaches past d_k + 2 E_q (d_k the k-th distance over all rows, E_q the
query's bound): a row inside that window can have a filter key below a row of the top k.  For every (query, split) this
counts the rows with d <= d_k + 2 E_q; the largest count must stay <= k' / 2 (dvf::kKeep / 2) for k' to be justified.
E_q restates dvf::row's maxima and dvf::query (csrc/diverg_filter.hpp) in numpy; d is the float64 inner-product form.

    python3 tools/diverg_fast_sim.py [--data bench | fixture] [--rows 1000000] [--dim 128] [--batch 1024] [--k 10]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KEEP, SPLITS, ROW_BLOCK = 32, 64, 32          # dvf::kKeep, kSplits, kRowBlock
U32, UACC, U40 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -40
FORMS = {"kldivfast": 0, "kldivfastrq": 1, "kldivgenfast": 2, "kldivgenfastrq": 3, "itakurasaitofast": 4}


def bf16_rn(v):
    """dvf::bf16_rn on finite float32: nearest even to 8 significant bits, subnormal results flushed"""
    u = v.view(np.uint32)
    r = u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))
    r = np.where((r & np.uint32(0x7F800000)) == 0, u & np.uint32(0x80000000), r)
    return (r & np.uint32(0xFFFF0000)).view(np.float32)


def norms(v):
    """Euclidean norms per row of v, of its hi and lo parts and of the split's residual, as float64, widened as dvf does"""
    hi = bf16_rn(v)
    lo = bf16_rn(v - hi)
    v64, h, l = v.astype(np.float64), hi.astype(np.float64), lo.astype(np.float64)
    w = 1.0 + U40
    return [np.sqrt((t * t).sum(1)) * w for t in (v64, h, l, v64 - h - l)]


def up32(r):
    f = r.astype(np.float32)
    return np.where(f.astype(np.float64) < r, np.nextafter(f, np.float32(np.inf)), f).astype(np.float64)


def operands(form, X, Q):
    """-> a, b (float32 operands), sign, R_row, R_abs, C_q, C_abs (float64)"""
    lX, lQ = np.log(X), np.log(Q)          # float32 logarithms, as stored
    x, q, lx, lq = (t.astype(np.float64) for t in (X, Q, lX, lQ))
    if form == 0:
        return X, lQ, -1.0, (x * lx).sum(1), np.abs(x * lx).sum(1), np.zeros(len(Q)), np.zeros(len(Q))
    if form == 1:
        return lX, Q, -1.0, np.zeros(len(X)), np.zeros(len(X)), (q * lq).sum(1), np.abs(q * lq).sum(1)
    if form == 2:
        return X, lQ, -1.0, (x * lx - x).sum(1), (np.abs(x * lx) + np.abs(x)).sum(1), q.sum(1), np.abs(q).sum(1)
    if form == 3:
        return lX, Q, -1.0, x.sum(1), np.abs(x).sum(1), (q * lq - q).sum(1), (np.abs(q * lq) + np.abs(q)).sum(1)
    D = X.shape[1]
    return X, np.float32(1) / Q, 1.0, -lx.sum(1), np.abs(lx).sum(1), lq.sum(1) - D, (np.abs(lq) + 1.0).sum(1)


def bound(a, b, Rabs, Cabs, dim):
    """dvf::query's E_q per query from the rows' largest figures"""
    m_a, m_hi, m_lo, m_res = (up32(t).max() for t in norms(a))
    r_abs = up32(Rabs * (1.0 + U40)).max()
    B, Bh, Bl, Br = norms(b)
    dpad = (dim + 15) // 16 * 16
    T = m_hi * Bh + m_hi * Bl + m_lo * Bh
    S = r_abs + Cabs + m_a * B
    e = m_lo * Bl + m_res * B + (m_a + m_res) * Br
    e += 1.001 * 3.0 * dpad * UACC * T
    e += U32 * 1.001 * (T + r_abs)
    e += (U32 + U40) * r_abs + U40 * Cabs
    e += 1.001 * (dim / 2 + 12.0) * U32 * S
    return e * (1.0 + U40) + 1e-30


def simulate(space, X, Q, k):
    """-> dict: E_q, and over all (query, split) the count of rows with d <= d_k + 2 E_q"""
    n, dim = X.shape
    a, b, sign, R, Rabs, C, Cabs = operands(FORMS[space], X, Q)
    E = bound(a, b, Rabs, Cabs, dim)
    nblocks = (n + ROW_BLOCK - 1) // ROW_BLOCK
    rows_per_split = (nblocks + SPLITS - 1) // SPLITS * ROW_BLOCK
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    dist = lambda r0, r1: sign * (b64 @ a64[r0:r1].T) + R[None, r0:r1] + C[:, None]
    best = np.full((len(Q), k), np.inf)
    for r0 in range(0, n, rows_per_split):
        d = dist(r0, min(n, r0 + rows_per_split))
        best = np.sort(np.concatenate([best, np.partition(d, min(k, d.shape[1]) - 1, axis=1)[:, :k]], axis=1), axis=1)[:, :k]
    limit = best[:, k - 1] + 2 * E
    counts = np.stack([(dist(r0, min(n, r0 + rows_per_split)) <= limit[:, None]).sum(1)
                       for r0 in range(0, n, rows_per_split)], axis=1)
    return {"space": space, "rows": n, "dim": dim, "queries": len(Q), "k": k, "splits": counts.shape[1],
            "rows_per_split": rows_per_split, "keep": KEEP, "E_q_median": float(np.median(E)), "E_q_max": float(E.max()),
            "d_k_median": float(np.median(best[:, k - 1])),
            "rows_within_2E_per_split_max": int(counts.max()),
            "rows_within_2E_per_split_p99": float(np.percentile(counts, 99)),
            "rows_within_2E_per_query_max": int(counts.sum(1).max()),
            "queries_without_proof": int((counts.max(1) >= KEEP).sum()),
            "holds": bool(counts.max() <= KEEP // 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--data", choices=("bench", "fixture"), default="bench")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--spaces", default=None)
    a = ap.parse_args()
    if a.data == "bench":      # the timing tool's histograms
        from tools.diverg_scan_time import histograms
        X, Q = histograms(1, a.rows, a.dim), histograms(2, a.batch, a.dim)
        spaces = (a.spaces or "kldivfast,itakurasaitofast").split(",")
    else:                      # the GPU test's rows and queries, at its largest k
        from tests.test_gpu_diverg_fast import data
        X, Q = data(a.dim)
        spaces = (a.spaces or ",".join(FORMS)).split(",")
    for space in spaces:
        print(json.dumps(simulate(space, X, Q, a.k)), flush=True)


if __name__ == "__main__":
    main()
