// Host arithmetic of the batched exact scan for 512 < k <= 4096 (brute.cpp: Engine::knn_brute): whether
// the batched kernels (last_path 12) or the per-query sort (last_path 5) answer a batch, the sample's block stride and
// rank, how the batch is cut into query slices and the workspace a slice takes.  Integer and double arithmetic only -- no
// HIP, nothing of the engine.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>

namespace gfxknn {

constexpr size_t kBigkBatchMaxK = 4096;          // the redo kernel sorts k keys in LDS
constexpr size_t kBigkBatchCap = 16384;          // keys of a query's list: 128 KB, what one workgroup sorts in LDS
constexpr size_t kBigkBatchMaxDim = 256;         // float rows: the register arrangement's bound (kRangeBatchMaxDim)
// The row gate (NMSLIB_GPU_BIGK_MIN_ROWS overrides it).  Not the fast paths' 65536: the suite's switch tests hold k = 513
// over 65 536, 70 001 and 263 173 rows to the per-query sort (last_path 5), so the gate sits above them, at 2^19.
constexpr size_t kBigkBatchMinRows = (size_t)1 << 19;
// The smallest batch (NMSLIB_GPU_BIGK_MIN_QUERIES overrides it).  Measured on 1M x 128: a single query is
// a tie or a loss against the per-query sort (0.6 .. 1.1 times), four queries win in every shape (1.7 .. 3.9 times).
constexpr size_t kBigkBatchMinQueries = 4;
constexpr size_t kBigkBatchWsBytes = (size_t)256 << 20;   // lists of one slice; NMSLIB_GPU_BIGK_WS_BYTES lowers it
constexpr size_t kBigkBatchTargetWgs = 1024;     // as the range batch: fewer row blocks are multiplied by query splits
constexpr size_t kBigkBatchQueryTile = 32;

struct BigkBatchPlan {
    bool use = false;
    size_t cap = 0;             // keys per query list
    size_t nblocks = 0;         // 64-row blocks
    size_t stride = 0;          // the sample pass walks the blocks b with b % stride == 0
    size_t rank = 0;            // the radius is the rank-th smallest sample distance (1-based)
    size_t slice_queries = 0, slices = 0;
    size_t grid_x = 0, grid_y = 0;        // the collect pass over all blocks
    size_t sample_grid_x = 0, sample_grid_y = 0;
};

// bytes of the lists one query takes
inline size_t bigk_batch_query_bytes() { return kBigkBatchCap * 8; }

// n rows of dim elements of elem bytes (4: float, 1: the 128 bytes of l2sqr_sift); min_rows, min_queries, budget: this
// call's gates
inline BigkBatchPlan bigk_batch_plan(size_t n, size_t dim, size_t elem, size_t nq, size_t k, size_t min_rows,
                                     size_t min_queries, size_t budget) {
    BigkBatchPlan p;
    const bool dim_ok = elem == 1 ? dim == 128 : dim >= 1 && dim <= kBigkBatchMaxDim;
    if (!dim_ok || k > kBigkBatchMaxK || n < 2 * k || n < min_rows || nq < min_queries) return p;
    if (budget < bigk_batch_query_bytes()) return p;
    p.cap = kBigkBatchCap;
    p.nblocks = (n + 63) / 64;
    p.stride = std::max<size_t>(1, (64 * p.nblocks + p.cap - 1) / p.cap);
    // Of the k nearest rows about Binomial(k, 1 / stride) are sampled: the mean plus four standard deviations puts the
    // radius short of the k-th distance once in about 1e4 queries.  Short is caught (count < k) and redone.
    const double mean = (double)k / (double)p.stride;
    p.rank = p.stride == 1 ? k : (size_t)std::ceil(mean + 4.0 * std::sqrt(mean) + 4.0);
    if (2 * p.stride * p.rank > p.cap) return p;   // the expected list is stride * rank keys
    const size_t sample_blocks = (p.nblocks + p.stride - 1) / p.stride;
    p.slice_queries = std::min(nq, budget / bigk_batch_query_bytes());
    p.slices = (nq + p.slice_queries - 1) / p.slice_queries;
    const size_t tiles = (p.slice_queries + kBigkBatchQueryTile - 1) / kBigkBatchQueryTile;
    p.grid_x = (p.nblocks + 3) / 4;
    p.grid_y = std::max<size_t>(1, std::min(tiles, (kBigkBatchTargetWgs + p.grid_x - 1) / p.grid_x));
    p.sample_grid_x = (sample_blocks + 3) / 4;
    p.sample_grid_y = std::max<size_t>(1, std::min(tiles, (kBigkBatchTargetWgs + p.sample_grid_x - 1) / p.sample_grid_x));
    p.use = true;
    return p;
}

// queries of slice s
inline size_t bigk_batch_slice_size(const BigkBatchPlan& p, size_t nq, size_t s) {
    const size_t q0 = s * p.slice_queries;
    return q0 >= nq ? 0 : std::min(p.slice_queries, nq - q0);
}

}  // namespace gfxknn
