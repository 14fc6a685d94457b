// Host arithmetic of a batched range query on the exact scan (range.cpp: Engine::range_batch_device):
// which route answers the batch, the grid of the match-bit kernel, the mask words per query, how the batch is cut into
// query slices and the workspace a slice takes.  Integer arithmetic only -- no HIP, nothing of the engine -- so that
// tests/range_batch_plan_check.cpp can check it without a GPU; tests/range_batch_plan_ref.py restates it.
#pragma once
#include <algorithm>
#include <cstddef>

namespace gfxknn {

// the match-bit kernel (kernels/range_batch_kernels.hip names the same numbers for its launch)
constexpr size_t kRangeBatchRowsPerWg = 256;   // four waves of 64 rows, a row's elements across the lanes
constexpr size_t kRangeBatchQueryTile = 32;    // queries staged in LDS at a time
constexpr size_t kRangeBatchMaxDim = 256;      // float rows: at most four elements of a row per lane
constexpr size_t kRangeBatchSelectRows = 1024; // rows per selection block (16 mask words), as in the single-query path
// workgroups the grid aims at: fewer row blocks than this are multiplied by query splits (grid.y), each taking every
// grid.y-th query tile
constexpr size_t kRangeBatchTargetWgs = 1024;
// queries of a slice at most: the selection kernels take one grid row (grid.y) per query
constexpr size_t kRangeBatchMaxSliceQueries = 32768;
// The bound of the mask workspace (masks and block counts of one slice).  The environment switch NMSLIB_GPU_RANGE_WS_BYTES
// lowers it for a call.  The grid itself has no cap: one workgroup per 256 rows, every workgroup takes one row block.
constexpr size_t kRangeBatchWsBytes = (size_t)256 << 20;

struct RangeBatchPlan {
    int route = 11;              // last_path: 10 the batched kernels, 11 the single-query launches per query
    size_t rows_per_wg = 0;      // route 10 from here on (route 11: all zero)
    size_t chunks = 0;           // elements of a row per lane: ceil(dim / 64) (uint8 rows: 1)
    size_t query_tile = 0;
    size_t grid_x = 0, grid_y = 0;
    size_t mask_words = 0;       // 64-bit words per query: ceil(n / 64)
    size_t blocks = 0;           // selection blocks per query: ceil(n / 1024)
    size_t slice_queries = 0;    // queries per slice (the last slice may hold fewer)
    size_t slices = 0;
    size_t workspace_bytes = 0;  // of a full slice: masks, then blocks + 1 counts per query
    bool count_only = false;     // capacity == 0: the chain stops after the scan
};

// bytes of the workspace one query takes
inline size_t range_batch_query_bytes(size_t n) {
    const size_t words = (n + 63) / 64, blocks = (n + kRangeBatchSelectRows - 1) / kRangeBatchSelectRows;
    return words * 8 + (blocks + 1) * 4;
}

// n rows of dim elements of elem bytes (4: float, 1: the 128 bytes of l2sqr_sift), nq queries, capacity per query,
// budget: the workspace bound of this call
inline RangeBatchPlan range_batch_plan(size_t n, size_t dim, size_t elem, size_t nq, size_t capacity, size_t budget) {
    RangeBatchPlan p;
    p.count_only = capacity == 0;
    const bool dim_ok = elem == 1 ? dim == 128 : dim >= 1 && dim <= kRangeBatchMaxDim;
    const size_t per_query = range_batch_query_bytes(n);
    if (!dim_ok || per_query > budget || nq == 0) return p;   // (an empty batch launches nothing on either route)
    p.route = 10;
    p.rows_per_wg = kRangeBatchRowsPerWg;
    p.chunks = elem == 1 ? 1 : (dim + 63) / 64;
    p.query_tile = kRangeBatchQueryTile;
    p.mask_words = (n + 63) / 64;
    p.blocks = (n + kRangeBatchSelectRows - 1) / kRangeBatchSelectRows;
    p.slice_queries = std::min({nq, budget / per_query, kRangeBatchMaxSliceQueries});
    p.slices = (nq + p.slice_queries - 1) / p.slice_queries;
    p.workspace_bytes = p.slice_queries * per_query;
    p.grid_x = (n + kRangeBatchRowsPerWg - 1) / kRangeBatchRowsPerWg;
    const size_t tiles = (p.slice_queries + kRangeBatchQueryTile - 1) / kRangeBatchQueryTile;
    const size_t want = p.grid_x ? (kRangeBatchTargetWgs + p.grid_x - 1) / p.grid_x : 1;
    p.grid_y = std::max<size_t>(1, std::min(tiles, want));
    return p;
}

// queries of slice s
inline size_t range_batch_slice_size(const RangeBatchPlan& p, size_t nq, size_t s) {
    const size_t q0 = s * p.slice_queries;
    return q0 >= nq ? 0 : std::min(p.slice_queries, nq - q0);
}

}  // namespace gfxknn
