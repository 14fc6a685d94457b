// The plan of the bit_jaccard matrix-core scan (kernels/jaccard_mfma_kernels.hip; last_path 18): whether a
// batch is served and how its rows and queries are split.  Header-only, no HIP types.
//
// Served: an exact scan (brute_force / seq_search) over n >= kMinRows rows, a batch of nq >= kMinQueries queries,
// 1 <= k <= kMaxK (k <= kNarrowMaxK for codes below kWideBits), bits <= kMaxBits, and the split of ham_fast_plan.hpp (a split
// within 65 536 rows, nsplit * k <= 8192).  Everything else runs jac_knn_kernel.  The k gate is where the path was measured to
// win (DESIGN.md 6 "string scan"): it loses at k = 64 at every measured width and at k = 32 below 1024 bits.  `measure`
// (NMSLIB_GPU_JAC_FAST=2, for tools/jac_fast_time.py) lifts the k gate to the kernel's own limit kKernelMaxK, so that a cell
// outside the gate can be timed.
#pragma once
#include "ham_fast_plan.hpp"

namespace gfxknn {
namespace jacfast {

using hamfast::Plan;
constexpr int kMinRows = hamfast::kMinRows;
constexpr int kMinQueries = hamfast::kMinQueries;
constexpr int kKernelMaxK = 64;    // what the kernel can hold: lists of 2 k + 32 u64 keys, 98.8 KiB of LDS at 2048 bits
constexpr int kMaxK = 32;          // 64-bit keys: the cut of a list costs twice the bit_hamming scan's; measured to lose at 64
constexpr int kNarrowMaxK = 16;    // ... and at 32 on codes of 256 and 512 bits:
constexpr int kWideBits = 1024;    // 16 < k <= 32 is served from this width on
constexpr int kMaxBits = 2048;     // the common fingerprint width; the K loop only gets longer
constexpr int kPopRows = hamfast::kRowBlock;   // |b| of a row block's rows, handed from the loading lanes to the accumulators' lanes

// dynamic LDS of a workgroup: query words [W][tile] u32, lists [cap][tile] u64, counters [tile], |b| [kPopRows]
inline size_t lds_bytes(int W, int cap, int tile) {
    return ((size_t)W + 2 * (size_t)cap + 1) * tile * 4 + (size_t)kPopRows * 4;
}

inline Plan plan(bool exact_scan, long long n, long long nq, long long k, long long bits, bool measure = false) {
    Plan p;
    if (!exact_scan || n < kMinRows || n > 0x7FFFFFFFll || nq < kMinQueries || k < 1 || k > kKernelMaxK || bits < 1 ||
        bits > kMaxBits)
        return p;
    if (!measure && (k > kMaxK || (k > kNarrowMaxK && bits < kWideBits))) return p;
    if (!hamfast::split_rows(p, n, nq, k)) return p;
    p.W = (int)((bits + 31) / 32);
    p.lds = lds_bytes(p.W, p.cap, p.tile);   // at most 64.8 KiB in the gate (2048 bits, k = 32) of a compute unit's 160
    p.use = true;
    return p;
}

}  // namespace jacfast
}  // namespace gfxknn
