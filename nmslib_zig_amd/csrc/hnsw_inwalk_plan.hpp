// Host arithmetic of the in-walk filtered HNSW search (gpu_inwalk=1; hnsw_search.cpp, kernels/hnsw_inwalk_kernels.hip;
// DESIGN.md 4.6e): whether the kernel serves a batch, and the LDS a workgroup takes.  Integer arithmetic only -- no HIP,
// nothing of the engine -- so that tests/hnsw_inwalk_plan_check.cpp can check it without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>

namespace gfxknn {

// W, the eligible nodes found so far: cap = max(efSearch, k) entries, at most this many (the LDS kernels' sorted array)
constexpr size_t kInwalkCapMax = 1024;
// C, the admitted nodes not yet expanded: CAPC entries, a ring (a power of two)
constexpr size_t kInwalkCandCap = 1024;
// the frontier arrays hold adjacency lists of up to 254 neighbours (kernels.hpp names the same number: HNSW_NBCAP_LDS)
constexpr size_t kInwalkNbcapMax = 256;
// the new keys of one step: a chunk of 64 neighbours
constexpr size_t kInwalkSortKeys = 64;
// LDS a workgroup of gfx950 can be given (160 KB)
constexpr size_t kInwalkLdsMax = 160 * 1024;

inline size_t inwalk_cap(size_t ef, size_t k) { return std::max(ef, k); }

// LDS of hnsw_inwalk_kernel (the launch uses this very number), every part a multiple of 16 bytes: the staged query
// (query_bytes: ldv floats, or the 128 bytes of a u8 query), the frontier's positions and distances (nbcap each), the sort
// area, W (cap 64-bit keys, an even number of them) and C.
inline size_t inwalk_lds_bytes(size_t cap, size_t nbcap, size_t query_bytes) {
    return (query_bytes + 15) / 16 * 16 + nbcap * 8 + kInwalkSortKeys * 8 + (cap + 1) / 2 * 16 + kInwalkCandCap * 8;
}

// A batch at efSearch = ef asked for k results on a graph whose frontier arrays take nbcap entries (hnsw_nbcap): served
// when W and the lists fit the kernel and everything fits into LDS (a query of several ten thousand dimensions does not).
// What is not served takes the two-stage route.
inline bool inwalk_served(size_t ef, size_t k, size_t nbcap, size_t query_bytes) {
    const size_t cap = inwalk_cap(ef, k);
    return cap >= 1 && cap <= kInwalkCapMax && nbcap <= kInwalkNbcapMax && nbcap % 64 == 0 &&
           inwalk_lds_bytes(cap, nbcap, query_bytes) <= kInwalkLdsMax;
}

}  // namespace gfxknn
