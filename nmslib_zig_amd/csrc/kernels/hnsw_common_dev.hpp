// Device helpers shared by the HNSW search and construction kernels (wave64).
#pragma once
#include <type_traits>

#include "common_dev.hpp"

namespace gfxknn {

// Host side: the space code of a graph as a compile-time constant.  f takes std::integral_constant<int, SP_...> and is
// instantiated for each of the nine spaces an HNSW graph can have; any other code is an invalid value.
template <class F>
static hipError_t hnsw_dispatch_space(int space, F&& f) {
    switch (space) {
        case SP_L2SQR: return f(std::integral_constant<int, SP_L2SQR>{});
        case SP_L2: return f(std::integral_constant<int, SP_L2>{});
        case SP_L1: return f(std::integral_constant<int, SP_L1>{});
        case SP_LINF: return f(std::integral_constant<int, SP_LINF>{});
        case SP_NORMCOS: return f(std::integral_constant<int, SP_NORMCOS>{});
        case SP_COSINE: return f(std::integral_constant<int, SP_COSINE>{});
        case SP_ANGULAR: return f(std::integral_constant<int, SP_ANGULAR>{});
        case SP_NEGDOT: return f(std::integral_constant<int, SP_NEGDOT>{});
        case SP_L2SQR_SIFT: return f(std::integral_constant<int, SP_L2SQR_SIFT>{});
        default: return hipErrorInvalidValue;
    }
}

template <int SPACE>
struct DistTraits {
    static constexpr bool kU8 = (SPACE == SP_L2SQR_SIFT);
    static constexpr bool kThree = (SPACE == SP_COSINE || SPACE == SP_ANGULAR);
    static constexpr bool kMax = (SPACE == SP_LINF);
};

template <int SPACE>
__device__ __forceinline__ void accum4(const f32x4& q, const f32x4& b, float& s0, float& s1, float& s2) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (SPACE == SP_L2SQR || SPACE == SP_L2) {
            const float t = q[j] - b[j];
            s0 = fmaf(t, t, s0);
        } else if constexpr (SPACE == SP_L1) {
            s0 += fabsf(q[j] - b[j]);
        } else if constexpr (SPACE == SP_LINF) {
            s0 = fmaxf(s0, fabsf(q[j] - b[j]));
        } else if constexpr (SPACE == SP_NORMCOS || SPACE == SP_NEGDOT) {
            s0 = fmaf(q[j], b[j], s0);
        } else {  // cosine / angular on raw rows: dot, |row|^2, |query|^2
            s0 = fmaf(b[j], q[j], s0);
            s1 = fmaf(b[j], b[j], s1);
            s2 = fmaf(q[j], q[j], s2);
        }
    }
}

template <int SPACE>
__device__ __forceinline__ float finish_dist(float s0, float s1, float s2) {
    if constexpr (SPACE == SP_L2) return sqrtf(s0);
    else if constexpr (SPACE == SP_NEGDOT) return -s0;
    else if constexpr (SPACE == SP_NORMCOS) {
        const float c = fmaxf(-1.0f, fminf(1.0f, s0));
        return fmaxf(0.0f, 1.0f - c);
    } else if constexpr (SPACE == SP_COSINE) return fmaxf(0.0f, 1.0f - normdot_finish(s0, s1, s2));
    else if constexpr (SPACE == SP_ANGULAR) return acosf(normdot_finish(s0, s1, s2));
    else return s0;
}

// 8-lane reductions with DPP (VALU speed; __shfl_xor would go through the LDS crossbar):
// row_half_mirror pairs lane i with 7-i inside each group of 8, then quad_perm swaps 1 and 2 apart.
template <typename T>
__device__ __forceinline__ T dpp_half_mirror(T v) {
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
}
template <typename T>
__device__ __forceinline__ T dpp_quad_xor1(T v) {  // quad_perm [1,0,3,2]
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
}
template <typename T>
__device__ __forceinline__ T dpp_quad_xor2(T v) {  // quad_perm [2,3,0,1]
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
}
__device__ __forceinline__ float group8_sum(float v) {
    v += dpp_half_mirror(v);
    v += dpp_quad_xor1(v);
    v += dpp_quad_xor2(v);
    return v;
}
__device__ __forceinline__ float group8_max(float v) {
    v = fmaxf(v, dpp_half_mirror(v));
    v = fmaxf(v, dpp_quad_xor1(v));
    v = fmaxf(v, dpp_quad_xor2(v));
    return v;
}
__device__ __forceinline__ int group8_sum_i(int v) {
    v += dpp_half_mirror(v);
    v += dpp_quad_xor1(v);
    v += dpp_quad_xor2(v);
    return v;
}

// ---- the row type of a gather -------------------------------------------------------------------------------------
// float: the rows the graph was built on (g.rows, stride g.ldv).  half_t: the fp16 traversal copy (g.rows16, stride
// g.ld16; fp16(2^e * row)).  Either way a lane's load is 16 bytes = kPer elements, the 8 lanes of a row cover kSpan
// consecutive elements, and a step of four such loads per lane covers kStep dimensions (128 floats / 256 halves).
// Per-lane element order, the same in every kernel (it fixes the bits of a distance): steps ascending, the four loads of
// a step ascending, the elements of a load ascending.
typedef _Float16 half_t;
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

template <class ROW>
struct RowTraits;
template <>
struct RowTraits<float> {
    using Vec = f32x4;
    static constexpr int kPer = 4, kSpan = 32, kStep = 128;
};
template <>
struct RowTraits<half_t> {
    using Vec = f16x8;
    static constexpr int kPer = 8, kSpan = 64, kStep = 256;
};
template <class ROW>
__device__ __forceinline__ const ROW* graph_rows(const HnswDeviceGraph& g) {
    if constexpr (std::is_same<ROW, half_t>::value) return reinterpret_cast<const half_t*>(g.rows16);
    else return reinterpret_cast<const float*>(g.rows);
}
template <class ROW>
__device__ __forceinline__ int graph_ld(const HnswDeviceGraph& g) {
    if constexpr (std::is_same<ROW, half_t>::value) return g.ld16;
    else return g.ldv;
}
// the query elements that face one load of a row (f32 in LDS); !ok: past the row, zeros
template <class ROW>
struct QueryVec {
    f32x4 v[RowTraits<ROW>::kPer / 4];
};
template <class ROW>
__device__ __forceinline__ QueryVec<ROW> load_query(const float* qd, bool ok) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    QueryVec<ROW> q;
#pragma unroll
    for (int h = 0; h < RowTraits<ROW>::kPer / 4; ++h) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(qd + 4 * h);
        q.v[h] = ok ? x : zero;
    }
    return q;
}
// one load of a row against the query; halves become floats and lose the copy's scale (a power of two: exact), then
// take the f32 formula
template <int SPACE, class ROW>
__device__ __forceinline__ void accum_load(const QueryVec<ROW>& q, const typename RowTraits<ROW>::Vec& b, bool ok,
                                           float inv_scale, float& s0, float& s1, float& s2) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    if constexpr (std::is_same<ROW, half_t>::value) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 x = {(float)b[4 * h] * inv_scale, (float)b[4 * h + 1] * inv_scale, (float)b[4 * h + 2] * inv_scale,
                             (float)b[4 * h + 3] * inv_scale};
            accum4<SPACE>(q.v[h], ok ? x : zero, s0, s1, s2);
        }
    } else {
        accum4<SPACE>(q.v[0], ok ? b : zero, s0, s1, s2);
    }
}

// Distances of the query to the m rows listed in nbr[0..m) -> nd[0..m).
// 8 lanes per row; 8 rows per pass; 4 passes issued together (32 rows in flight).
template <int SPACE, class ROW = float>
__device__ __forceinline__ void frontier_distances(const HnswDeviceGraph& g, const float* qv,
                                                   const uint8_t* qb, int qnorm, const int* nbr,
                                                   float* nd, int m, int lane) {
    using RT = RowTraits<ROW>;
    const int g8 = lane >> 3, sub = lane & 7;
    for (int base_i = 0; base_i < m; base_i += 32) {
        int ids[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            // slots past m re-read the last row (a cache hit) instead of branching: a load under its own
            // exec-masked branch is followed by a full vmcnt(0) wait, which serialises the whole gather
            const int idx = base_i + p * 8 + g8;
            ids[p] = nbr[idx < m ? idx : m - 1];
        }
        if constexpr (DistTraits<SPACE>::kU8) {
            // 128-byte rows: one 16-byte load per lane; exact integer n1 + n2 - 2*dot
            const i32x4 qq = *reinterpret_cast<const i32x4*>(qb + sub * 16);
            int dots[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                int dsum = 0;
                const i32x4 bb = *reinterpret_cast<const i32x4*>(
                    reinterpret_cast<const uint8_t*>(g.rows) + (size_t)ids[p] * 128 + sub * 16);
#pragma unroll
                for (int j = 0; j < 4; ++j) dsum = __builtin_amdgcn_udot4(qq[j], bb[j], dsum, false);
                dots[p] = dsum;
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int dot = group8_sum_i(dots[p]);
                const int idx = base_i + p * 8 + g8;
                if (sub == 0 && idx < m) nd[idx] = (float)(g.row_norm[ids[p]] + qnorm - 2 * dot);
            }
        } else {
            float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
            const ROW* rows = graph_rows<ROW>(g);
            const int ld = graph_ld<ROW>(g);
            // one step (128 floats / 256 halves) of the 4 rows per pass: all 16 row loads are issued before the first one
            // is waited for (random gathers of whole rows are latency-bound: the loads in flight per wave are the
            // throughput).  Out-of-range tails read a clamped address and are zeroed on both sides, so no load sits under
            // a divergent branch.
            const ROW* rp[4];
#pragma unroll
            for (int p = 0; p < 4; ++p) rp[p] = rows + (size_t)ids[p] * ld;
            const int dlast = ld - RT::kPer;
            for (int d0 = sub * RT::kPer; d0 < ld; d0 += RT::kStep) {
                typename RT::Vec bb[4][4];
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int d = d0 + RT::kSpan * it;
                    const int dc = d < dlast ? d : dlast;
#pragma unroll
                    for (int p = 0; p < 4; ++p) bb[it][p] = *reinterpret_cast<const typename RT::Vec*>(rp[p] + dc);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int d = d0 + RT::kSpan * it;
                    const bool ok = d < ld;
                    const int dc = d < dlast ? d : dlast;
                    const QueryVec<ROW> qq = load_query<ROW>(qv + dc, ok);
#pragma unroll
                    for (int p = 0; p < 4; ++p) accum_load<SPACE, ROW>(qq, bb[it][p], ok, g.inv_scale16, s0[p], s1[p], s2[p]);
                }
            }
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                float r0, r1 = 0.f, r2 = 0.f;
                if constexpr (DistTraits<SPACE>::kMax) r0 = group8_max(s0[p]);
                else r0 = group8_sum(s0[p]);
                if constexpr (DistTraits<SPACE>::kThree) {
                    r1 = group8_sum(s1[p]);
                    r2 = group8_sum(s2[p]);
                }
                const int idx = base_i + p * 8 + g8;
                if (sub == 0 && idx < m) nd[idx] = finish_dist<SPACE>(r0, r1, r2);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Split-phase form of frontier_distances for the software-pipelined search loop: issue() requests the first step (128
// floats / 256 halves; u8: the whole row) of the first 32 rows and returns; finish() consumes them, fetches whatever is
// left (longer rows, rows 32..m) and writes nd[0..m).  Same arithmetic, same order as frontier_distances (bit-identical
// results).
template <int SPACE, class ROW = float>
struct FrontierLoads {
    typename RowTraits<ROW>::Vec bb[4][4];
    i32x4 bu[4];
    int ids[4];
};

template <int SPACE, class ROW>
__device__ __forceinline__ void frontier_issue(FrontierLoads<SPACE, ROW>& L, const HnswDeviceGraph& g, const int* nbr, int m,
                                               int lane) {
    using RT = RowTraits<ROW>;
    const int g8 = lane >> 3, sub = lane & 7;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int idx = p * 8 + g8;
        L.ids[p] = nbr[idx < m ? idx : m - 1];
    }
    if constexpr (DistTraits<SPACE>::kU8) {
#pragma unroll
        for (int p = 0; p < 4; ++p)
            L.bu[p] = *reinterpret_cast<const i32x4*>(reinterpret_cast<const uint8_t*>(g.rows) + (size_t)L.ids[p] * 128 +
                                                       sub * 16);
    } else {
        const ROW* rows = graph_rows<ROW>(g);
        const int ld = graph_ld<ROW>(g);
        const int dlast = ld - RT::kPer;
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int d = sub * RT::kPer + RT::kSpan * it;
            const int dc = d < dlast ? d : dlast;
#pragma unroll
            for (int p = 0; p < 4; ++p)
                L.bb[it][p] = *reinterpret_cast<const typename RT::Vec*>(rows + (size_t)L.ids[p] * ld + dc);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <int SPACE, class ROW>
__device__ __forceinline__ void frontier_finish(FrontierLoads<SPACE, ROW>& L, const HnswDeviceGraph& g, const float* qv,
                                                const uint8_t* qb, int qnorm, const int* nbr, float* nd, int m,
                                                int lane) {
    using RT = RowTraits<ROW>;
    const int g8 = lane >> 3, sub = lane & 7;
    if constexpr (DistTraits<SPACE>::kU8) {
        const i32x4 qq = *reinterpret_cast<const i32x4*>(qb + sub * 16);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            int dsum = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) dsum = __builtin_amdgcn_udot4(qq[j], L.bu[p][j], dsum, false);
            const int dot = group8_sum_i(dsum);
            const int idx = p * 8 + g8;
            if (sub == 0 && idx < m) nd[idx] = (float)(g.row_norm[L.ids[p]] + qnorm - 2 * dot);
        }
    } else {
        float s0[4] = {0.f, 0.f, 0.f, 0.f}, s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
        const ROW* rows = graph_rows<ROW>(g);
        const int ld = graph_ld<ROW>(g);
        const int dlast = ld - RT::kPer;
        for (int d0 = sub * RT::kPer; d0 < ld; d0 += RT::kStep) {
            if (d0 != sub * RT::kPer) {  // steps after the first: fetched here (rows longer than one step)
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int d = d0 + RT::kSpan * it;
                    const int dc = d < dlast ? d : dlast;
#pragma unroll
                    for (int p = 0; p < 4; ++p)
                        L.bb[it][p] = *reinterpret_cast<const typename RT::Vec*>(rows + (size_t)L.ids[p] * ld + dc);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int d = d0 + RT::kSpan * it;
                const bool ok = d < ld;
                const int dc = d < dlast ? d : dlast;
                const QueryVec<ROW> qq = load_query<ROW>(qv + dc, ok);
#pragma unroll
                for (int p = 0; p < 4; ++p) accum_load<SPACE, ROW>(qq, L.bb[it][p], ok, g.inv_scale16, s0[p], s1[p], s2[p]);
            }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            float r0, r1 = 0.f, r2 = 0.f;
            if constexpr (DistTraits<SPACE>::kMax) r0 = group8_max(s0[p]);
            else r0 = group8_sum(s0[p]);
            if constexpr (DistTraits<SPACE>::kThree) {
                r1 = group8_sum(s1[p]);
                r2 = group8_sum(s2[p]);
            }
            const int idx = p * 8 + g8;
            if (sub == 0 && idx < m) nd[idx] = finish_dist<SPACE>(r0, r1, r2);
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (m > 32) frontier_distances<SPACE, ROW>(g, qv, qb, qnorm, nbr + 32, nd + 32, m - 32, lane);
}

// ---- adjacency lists of any length (round 3: M / maxM > 62, maxM0 > 126 -- hnsw.cc:189-208 takes any M) -------------
// The LDS search kernels give a list one or two words per lane.  SearchOld, the HBM-array SearchV1Merge and the in-walk kernel
// walk longer lists in chunks of 64 neighbours (list order kept: neighbour i is list word i + 1); their frontier arrays hold
// hnsw_nbcap(g) entries.
// unvisited neighbours of list[] -> nbr[0 .. m), returns m
template <class Visit>
__device__ __forceinline__ int collect_unvisited_any(const int* list, int* nbr, int lane, Visit&& visit) {
    const int cnt = __builtin_amdgcn_readfirstlane(list[0]);
    int m = 0;
    for (int c0 = 0; c0 < cnt; c0 += 64) {
        const int i = c0 + lane;
        const int nb = i < cnt ? list[i + 1] : 0;
        bool isn = false;
        if (i < cnt) isn = visit((uint32_t)nb);
        const u64 mask = __ballot(isn);
        if (isn) nbr[m + __popcll(mask & ((1ull << lane) - 1ull))] = nb;
        m += __popcll(mask);
    }
    return m;
}
// one greedy step on an upper level over a list of any length: the FIRST neighbour attaining the minimum, if it is closer
// than curdist (the sequential "if (d < curdist)" scan of hnsw.cc / hnsw_distfunc_opt.cc:176-196).  Returns the list length.
template <int SPACE, class ROW = float>
__device__ __forceinline__ int greedy_step_any(const HnswDeviceGraph& g, const int* list, const float* qv, const uint8_t* qb,
                                               int qnorm, int* nbr, float* nd, int lane, int& cur, float& curdist,
                                               bool& changed) {
    const int cnt = __builtin_amdgcn_readfirstlane(list[0]);
    for (int c0 = 0; c0 < cnt; c0 += 64)
        if (c0 + lane < cnt) nbr[c0 + lane] = list[c0 + lane + 1];
    __builtin_amdgcn_wave_barrier();
    if (cnt > 0) {
        frontier_distances<SPACE, ROW>(g, qv, qb, qnorm, nbr, nd, cnt, lane);
        u64 key = ~0ull;
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const int i = c0 + lane;
            if (i < cnt) {
                const u64 k2 = ((u64)f32_ord(nd[i]) << 32) | (uint32_t)i;
                key = k2 < key ? k2 : key;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 other = __shfl_xor(key, o, 64);
            key = other < key ? other : key;
        }
        const float dmin = ord_f32((uint32_t)(key >> 32));
        if (dmin < curdist) {
            curdist = dmin;
            cur = nbr[(uint32_t)key];
            changed = true;
        }
    }
    __builtin_amdgcn_wave_barrier();
    return cnt;
}

// ---- the filter of a query ----
// What a filter kernel is launched with: one filter for the whole launch, or a table and each query's entry.  at(q) is the
// entry of the workgroup's query as wave-uniform values: the per-query form reads the slot and the entry once, and every
// field goes through readfirstlane, so that the bitset tests behind it address from scalars as the one-filter form does.
struct FilterOne {
    FilterSlot f;
    __device__ __forceinline__ FilterSlot at(int) const { return f; }
};
__device__ __forceinline__ int uniform_i(int v) { return __builtin_amdgcn_readfirstlane(v); }
template <class T>
__device__ __forceinline__ const T* uniform_ptr(const T* p) {
    const unsigned long long v = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return reinterpret_cast<const T*>(((unsigned long long)hi << 32) | lo);
}
struct FilterPerQuery {
    FilterEach e;
    __device__ __forceinline__ FilterSlot at(int q) const {
        const FilterSlot s = e.table[uniform_i(e.slot[q])];
        return {uniform_ptr(s.allow), uniform_ptr(s.list), uniform_i(s.n_allow), uniform_i(s.m)};
    }
};

}  // namespace gfxknn
