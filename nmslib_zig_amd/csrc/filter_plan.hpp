// Host arithmetic of a filtered HNSW batch (filter.cpp): which of the two routes answers it, and the LDS the
// subset scan takes.  Integer arithmetic only -- no HIP, nothing of the engine -- so that tests/filter_plan_check.cpp can
// check it without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>

namespace gfxknn {

// capacity of hnsw_subset_knn_kernel (kernels.hpp names the same number for the launch)
constexpr size_t kFilterSubsetMax = 4096;
// LDS a workgroup of gfx950 can be given (160 KB)
constexpr size_t kFilterLdsMax = 160 * 1024;

enum class FilterRoute { Walk, Subset };

// The walk's result array: a filtered batch runs the search for this many results and keeps the first k allowed ones.
inline size_t filter_walk_results(size_t ef, size_t k) { return std::max(ef, k); }

// entries of the subset scan's key array for m listed rows: a power of two, at least 64
inline size_t filter_subset_keys(size_t m) {
    size_t mpad = 64;
    while (mpad < m) mpad <<= 1;
    return mpad;
}
// LDS of hnsw_subset_knn_kernel (the launch uses this very number): 64-bit keys, the staged query (query_bytes: ldv floats, or
// the 128 bytes of a u8 query), four waves' 64 positions and 64 distances, two shared words
inline size_t filter_subset_lds_bytes(size_t m, size_t query_bytes) {
    return filter_subset_keys(m) * 8 + query_bytes + 4 * 64 * 8 + 16;
}

// m allowed live rows, a batch asked for k results at efSearch = ef; scan_rows: the caller's bound (0 = none); query_bytes: see
// filter_subset_lds_bytes.
// A walk for k' = max(ef, k) results evaluates at least k' distances; a scan of m <= k' rows evaluates m and is exact, so up
// to there the scan is never the worse choice and the rule needs no measured threshold.  scan_rows moves the bound up for a
// caller who has measured; the kernel's capacity caps it, and a scan whose keys and query do not fit into LDS (rows of
// several thousand dimensions) is left to the walk.
inline FilterRoute filter_route(size_t m, size_t ef, size_t k, size_t scan_rows, size_t query_bytes) {
    const size_t bound = std::max(filter_walk_results(ef, k), scan_rows);
    const bool fits = filter_subset_lds_bytes(m, query_bytes) <= kFilterLdsMax;
    return m <= bound && m <= kFilterSubsetMax && fits ? FilterRoute::Subset : FilterRoute::Walk;
}

}  // namespace gfxknn
