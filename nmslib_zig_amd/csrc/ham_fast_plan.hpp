// The plan of the bit_hamming matrix-core scan (kernels/ham_mfma_kernels.hip; last_path 17): whether a
// batch is served and how its rows and queries are split.  Header-only, no HIP types: tests/ham_fast_plan_check.cpp calls it.
//
// Served: an exact scan (brute_force / seq_search) over n >= kMinRows rows, a batch of nq >= kMinQueries queries,
// 1 <= k <= kMaxK, kMinBits <= bits <= kMaxBits -- and a split of the rows that keeps a split within 65 536 rows (its
// keys are (distance << 16) | row within the split) with nsplit * k <= 8192 (launch_merge_topk_ex merges in LDS).  The
// last condition refuses only n > 2^29 / k rows, more than 4 194 304 at k = 128.  Everything else runs ham_knn_kernel.
#pragma once
#include <cstddef>

namespace gfxknn {
namespace hamfast {

constexpr int kMinRows = 65536;
constexpr int kMinQueries = 256;
constexpr int kMaxK = 128;
constexpr int kMinBits = 1;        // every width up to kMaxBits is served (DESIGN.md 6 "string scan": both measured widths win at k = 10)
constexpr int kMaxBits = 1024;
constexpr int kSplitMaxRows = 65536;   // a row's place in its split is 16 bits of its key
constexpr int kSplitMinRows = 1024;    // no finer: a split's lists start empty, and every split costs nq * k keys
constexpr int kMergeKeys = 8192;       // nsplit * k the merge sorts in LDS
constexpr int kSampleRows = 16384;     // rows scanned first: their k-th distance per query bounds the scan of all rows
constexpr int kSampleSplits = 16;
constexpr int kRowBlock = 128;         // rows a wave scores at once: 4 groups of 32
constexpr int kQueryGroups = 2;       // 4 row groups x 2 query groups of 32 x 32 accumulators: 128 registers, two waves per SIMD
constexpr int kWantWaves = 4096;       // workgroups (one wave each) the grid aims at: two rounds of 2 waves on 1024 SIMDs

struct Plan {
    bool use = false;
    int W = 0;                 // uint32 words per row
    int qb = 0;                // 32-query groups per wave (kQueryGroups)
    int tile = 0;              // queries per workgroup = 32 * qb
    int ntiles = 0;
    int cap = 0;               // keys a query's list holds: 2 k + 32 (a cut leaves k; behind one look at the count the
                               // query's two lanes append up to 16 keys each)
    int nsplit = 0, rows_per_split = 0;   // rows_per_split is a multiple of kRowBlock
    int sample_rows = 0, sample_nsplit = 0;   // the sample pass: sample_nsplit <= nsplit splits of whole row blocks
    size_t lds = 0;            // dynamic LDS of a workgroup: query words [W][tile], lists [cap][tile], counters [tile]
};

// The split of n >= kMinRows rows and nq queries at 1 <= k <= kMaxK, the sample pass and the list capacity (everything but
// W and lds); false when no split keeps within both limits.  Shared with the bit_jaccard scan (jac_fast_plan.hpp).
inline bool split_rows(Plan& p, long long n, long long nq, long long k) {
    const long long min_split = (n + kSplitMaxRows - 1) / kSplitMaxRows, max_split = kMergeKeys / k;
    if (min_split > max_split) return false;
    p.cap = 2 * (int)k + 32;
    p.qb = kQueryGroups;
    p.tile = 32 * p.qb;
    p.ntiles = (int)((nq + p.tile - 1) / p.tile);
    long long want = (kWantWaves + p.ntiles - 1) / p.ntiles;
    if (want < min_split) want = min_split;
    if (want > max_split) want = max_split;
    long long rps = (n + want - 1) / want;
    if (rps < kSplitMinRows) rps = kSplitMinRows;
    rps = (rps + kRowBlock - 1) / kRowBlock * kRowBlock;   // (<= 65 536: want >= min_split, and 65 536 is a multiple)
    p.rows_per_split = (int)rps;
    p.nsplit = (int)((n + rps - 1) / rps);
    p.sample_rows = kSampleRows;   // (< kMinRows <= n; >= kMaxK rows: every query has a k-th distance there)
    p.sample_nsplit = p.nsplit < kSampleSplits ? p.nsplit : kSampleSplits;
    while (p.sample_rows % (p.sample_nsplit * kRowBlock)) --p.sample_nsplit;
    return true;
}

inline Plan plan(bool exact_scan, long long n, long long nq, long long k, long long bits) {
    Plan p;
    if (!exact_scan || n < kMinRows || n > 0x7FFFFFFFll || nq < kMinQueries || k < 1 || k > kMaxK || bits < kMinBits ||
        bits > kMaxBits)
        return p;
    if (!split_rows(p, n, nq, k)) return p;
    p.W = (int)((bits + 31) / 32);
    p.lds = ((size_t)p.W + p.cap + 1) * p.tile * 4;
    p.use = true;
    return p;
}

}  // namespace hamfast
}  // namespace gfxknn
