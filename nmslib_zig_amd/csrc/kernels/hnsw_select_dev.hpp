// Neighbour selection shared by the HNSW construction kernels (hnsw_build_kernels.hip) and the consolidation kernels
// (hnsw_consolidate_kernels.hip): a stored row as the query of frontier_distances, and the reference's selection
// heuristics over candidates sorted by distance.  One wavefront (wave64) per call.
#pragma once
#include "hnsw_common_dev.hpp"

namespace gfxknn {

// Stored row `node` becomes the "query" of frontier_distances (LDS copy; u8: bytes + norm).
template <int SPACE>
__device__ __forceinline__ void stage_row(const HnswDeviceGraph& g, int node, float* qv, int& qnorm, int lane) {
    if constexpr (DistTraits<SPACE>::kU8) {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(g.rows) + (size_t)node * 128;
        reinterpret_cast<uint16_t*>(qv)[lane] = reinterpret_cast<const uint16_t*>(src)[lane];
        qnorm = g.row_norm[node];
    } else {
        const float* src = reinterpret_cast<const float*>(g.rows) + (size_t)node * g.ldv;
        for (int d = lane; d < g.ldv; d += 64) qv[d] = src[d];
        qnorm = 0;
    }
    __builtin_amdgcn_wave_barrier();
}

// getNeighborsByHeuristic2 over candidates sorted by ascending distance to the centre node.
// A candidate is kept unless some already kept node is strictly closer to it than the centre is.
// Fewer than NN candidates: all are kept (hnsw.h:133-135).  delaunay_type 0: the NN closest.
template <int SPACE>
__device__ __forceinline__ int heuristic2(const HnswDeviceGraph& g, const int* cid, const float* cd, int nc, int NN,
                                          int delaunay, float* qv, float* nd, int* kept_id, float* kept_d, int lane) {
    if (nc < NN || delaunay == 0) {
        const int n = nc < NN ? nc : NN;
        for (int i = lane; i < n; i += 64) {
            kept_id[i] = cid[i];
            kept_d[i] = cd[i];
        }
        __builtin_amdgcn_wave_barrier();
        return n;
    }
    int nk = 0;
    for (int i = 0; i < nc && nk < NN; ++i) {
        const int c = cid[i];
        const float dc = cd[i];
        bool good = true;
        if (nk > 0) {
            int qnorm;
            stage_row<SPACE>(g, c, qv, qnorm, lane);
            frontier_distances<SPACE>(g, qv, reinterpret_cast<const uint8_t*>(qv), qnorm, kept_id, nd, nk, lane);
            bool bad = false;
            for (int j = lane; j < nk; j += 64) bad |= nd[j] < dc;
            good = !__any(bad);
        }
        if (good) {
            if (lane == 0) {
                kept_id[nk] = c;
                kept_d[nk] = dc;
            }
            nk++;
        }
        __builtin_amdgcn_wave_barrier();
    }
    return nk;
}

// getNeighborsByHeuristic1 (hnsw.h:82-127): heuristic 2, then the list is topped up to NN with the closest rejected
// candidates.  Candidates ascending by (distance, position); kept ones are marked in place (cid[i] = ~id), so the
// result comes out in candidate order again: ascending by (distance, position), like heuristic2's.
template <int SPACE>
__device__ __forceinline__ int heuristic1(const HnswDeviceGraph& g, int* cid, const float* cd, int nc, int NN, float* qv,
                                          float* nd, int* kept_id, float* kept_d, int lane) {
    if (nc < NN) {
        for (int i = lane; i < nc; i += 64) {
            kept_id[i] = cid[i];
            kept_d[i] = cd[i];
        }
        __builtin_amdgcn_wave_barrier();
        return nc;
    }
    int nk = 0;
    for (int i = 0; i < nc && nk < NN; ++i) {
        const int c = cid[i];
        const float dc = cd[i];
        bool good = true;
        if (nk > 0) {
            int qnorm;
            stage_row<SPACE>(g, c, qv, qnorm, lane);
            frontier_distances<SPACE>(g, qv, reinterpret_cast<const uint8_t*>(qv), qnorm, kept_id, nd, nk, lane);
            bool bad = false;
            for (int j = lane; j < nk; j += 64) bad |= nd[j] < dc;
            good = !__any(bad);
        }
        if (good) {
            if (lane == 0) {
                kept_id[nk] = c;
                kept_d[nk] = dc;
                cid[i] = ~c;
            }
            nk++;
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (nk == NN) return nk;   // (the loop stopped at NN kept: nothing is topped up)
    // every candidate was examined: the kept ones and the first NN - nk rejected ones, in candidate order
    const int need = NN - nk;
    const u64 below = (1ull << lane) - 1ull;
    int out = 0, rej = 0;
    for (int base = 0; base < nc; base += 64) {
        const int i = base + lane;
        const int c = i < nc ? cid[i] : 0;
        const bool isk = i < nc && c < 0, isr = i < nc && c >= 0;
        const u64 rm = __ballot(isr);
        const bool take = isk || (isr && rej + __popcll(rm & below) < need);
        const u64 tm = __ballot(take);
        if (take) {
            const int slot = out + __popcll(tm & below);
            kept_id[slot] = isk ? ~c : c;
            kept_d[slot] = cd[i];
        }
        out += __popcll(tm);
        rej += __popcll(rm);
    }
    __builtin_amdgcn_wave_barrier();
    return out;
}

// the selection of Hnsw::add (hnsw.cc:582-597) and of addFriendlevel's shrink (hnsw.h:283-289) by delaunay_type
template <int SPACE, int W>
__device__ __forceinline__ int select_neighbours(const HnswDeviceGraph& g, int* cid, const float* cd, int nc, int NN,
                                                 int delaunay, float* qv, float* nd, int* kept_id, float* kept_d,
                                                 int lane) {
    if constexpr (W > 128) {
        if (delaunay == 1) return heuristic1<SPACE>(g, cid, cd, nc, NN, qv, nd, kept_id, kept_d, lane);
    }
    return heuristic2<SPACE>(g, cid, cd, nc, NN, delaunay, qv, nd, kept_id, kept_d, lane);
}

}  // namespace gfxknn
