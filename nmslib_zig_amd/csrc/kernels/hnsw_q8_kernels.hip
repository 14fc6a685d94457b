// gpu_rows=i8: the 8-bit traversal copy of the HNSW rows and the walk over it.
//
// The copy (q8_pack.hpp): per row the codes round(x / 2^e) in [-127, 127], zero padded to whole 16-byte loads, then one more
// 16-byte slot whose first int32 is the sum of the squared codes -- a visited row is ONE contiguous gather, no second array.
// The walk: the SearchV1Merge body that hnsw_search_kernel runs (hnsw_walk_dev.hpp), one wavefront per query, with
//   gather      8 lanes x 16 bytes per row and load = 128 dimensions; 8 rows per wave-load, 4 such passes (32 rows) and up
//               to 4 loads per row in flight before the first is waited for; a 768-D row is 6 loads per lane, the f32 form's
//               24.  Tails read a clamped address and are zeroed on both sides; the slot of the sum is one more load issued
//               with the others.  Nothing is loaded under a divergent branch.
//   arithmetic  integers only, exact in any order: v_dot4_i32_i8 for the dot kinds (key -dot) and for l2 (key |q|^2 + |x|^2
//               - 2 dot: the difference form would need 9-bit operands); v_sad_u8 on codes biased by 128 for l1.
//   keys        the int32 converted to f32 (v_cvt_f32_i32): monotone, exact below 2^24; beyond, neighbours may tie, which a
//               walk that is re-ranked can bear.  Never a bit-cast: comparing those depends on the denormal mode.
// cosinesimil on raw rows and angulardist order by dot / |x|, which is no integer: their key is -dot * rsq(sum of squared
// codes), two exact integers through one v_rsq_f32 and one multiplication in one lane, so still the same in every run.
// The kernel ends with its sorted array of max(ef, k) entries in the candidate workspace, array order and internal
// positions, for hnsw_rerank_kernel (hnsw_f16_kernels.hip): every distance returned is the f32 walk's.
//
// The body of the search is hnsw_walk_dev.hpp's, shared with hnsw_kernels.hip as source and instantiated here for this
// file's kernels: that file's compile time is the build's longest and this one adds no instantiation to it.  What is here
// is the pack kernel, the integer distances, the policy (query coding), the kernel's shell and the launcher.
#include <algorithm>

#include "../q8_pack.hpp"
#include "hnsw_args.hpp"
#include "hnsw_common_dev.hpp"
#include "hnsw_walk_dev.hpp"
#include "kernels.hpp"

namespace gfxknn {

enum Q8Kind : int { Q8_L2 = 0, Q8_L1 = 1, Q8_DOT = 2 };

// ---- the copy ------------------------------------------------------------------------------------------------------
// one wave per row: four codes a lane and store, the sum of squares through the wave, the slot by four lanes
__global__ __launch_bounds__(256) void hnsw_pack_rows8_kernel(const float* __restrict__ rows, int n, int ldv, int dim,
                                                              float inv_unit, uint8_t* __restrict__ out, int ld8) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lc = ld8 - 16;
    for (int r = blockIdx.x * 4 + w; r < n; r += gridDim.x * 4) {
        const float* src = rows + (size_t)r * ldv;
        uint32_t* dst = reinterpret_cast<uint32_t*>(out + (size_t)r * ld8);
        int ss = 0;
        for (int d0 = lane * 4; d0 < lc; d0 += 256) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = d0 + j < dim ? q8pack::code(src[d0 + j] * inv_unit) : 0;
                ss += c * c;
                word |= (uint32_t)(c & 0xFF) << (8 * j);
            }
            dst[d0 >> 2] = word;
        }
        ss = wave_sum_i(ss);
        if (lane < 4) dst[(lc >> 2) + lane] = lane == 0 ? (uint32_t)ss : 0u;
    }
}

hipError_t launch_hnsw_pack_rows8(const float* rows, int n, int ldv, int dim, int scale_exp, void* rows8, int ld8,
                                  hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (ld8 != (int)q8pack::row_stride((size_t)dim)) return hipErrorInvalidValue;
    const int blocks = (int)std::min<size_t>(((size_t)n + 3) / 4, 65536);
    hipLaunchKernelGGL(hnsw_pack_rows8_kernel, dim3(blocks), dim3(256), 0, s, rows, n, ldv, dim, q8pack::inv_unit_of(scale_exp),
                       static_cast<uint8_t*>(rows8), ld8);
    return hipGetLastError();
}

// ---- distances -----------------------------------------------------------------------------------------------------
// What a lane needs of the query next to its codes in LDS: the sum of the squared codes (l2) and whether the key divides by
// the row's norm (cosinesimil on raw rows, angulardist).
struct Q8Query {
    const uint8_t* codes;  // LDS, [ld8 - 16]; l1: biased by 128
    int qn;
    bool cosnorm;
};

constexpr int Q8_PER = 16, Q8_SPAN = 128, Q8_STEP = 512;  // bytes a lane loads; the 8 lanes of a row; four such loads

template <int KIND>
__device__ __forceinline__ int q8_accum(const i32x4& q, const i32x4& b, bool ok, int acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (KIND == Q8_L1) {
            // |a - b| of signed bytes = |(a + 128) - (b + 128)| of unsigned ones; the query is staged biased
            const uint32_t qq = ok ? (uint32_t)q[j] : 0u;
            const uint32_t bb = ok ? ((uint32_t)b[j] ^ 0x80808080u) : 0u;
            acc = (int)__builtin_amdgcn_sad_u8(qq, bb, (uint32_t)acc);
        } else {
            acc = __builtin_amdgcn_sdot4(ok ? q[j] : 0, ok ? b[j] : 0, acc, false);
        }
    }
    return acc;
}

// the walk's key of a row from the group's sum and the row's sum of squared codes
template <int KIND>
__device__ __forceinline__ float q8_key(int acc, int xn, const Q8Query& qq) {
    if constexpr (KIND == Q8_L2) return (float)(qq.qn + xn - 2 * acc);
    else if constexpr (KIND == Q8_L1) return (float)acc;
    else {
        if (qq.cosnorm) return xn > 0 ? -(float)acc * __builtin_amdgcn_rsqf((float)xn) : 0.f;
        return (float)(-acc);
    }
}

// the loads of up to 32 rows in flight: four loads of each row and its slot
struct Q8Loads {
    i32x4 bb[4][4];
    int xn[4];
    int ids[4];
};

__device__ __forceinline__ void q8_load_step(Q8Loads& L, const HnswDeviceGraph& g, int d0) {
    const uint8_t* rows = reinterpret_cast<const uint8_t*>(g.rows8);
    const int dlast = g.ld8 - 16 - Q8_PER;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int d = d0 + Q8_SPAN * it;
        const int dc = d < dlast ? d : dlast;
#pragma unroll
        for (int p = 0; p < 4; ++p) L.bb[it][p] = *reinterpret_cast<const i32x4*>(rows + (size_t)L.ids[p] * g.ld8 + dc);
    }
}
// (the 8 lanes of a row read the same word: one fetch, and no lane stands aside)
__device__ __forceinline__ void q8_load_norms(Q8Loads& L, const HnswDeviceGraph& g) {
    const uint8_t* rows = reinterpret_cast<const uint8_t*>(g.rows8);
#pragma unroll
    for (int p = 0; p < 4; ++p) L.xn[p] = *reinterpret_cast<const int*>(rows + (size_t)L.ids[p] * g.ld8 + (g.ld8 - 16));
}
template <int KIND>
__device__ __forceinline__ void q8_consume_step(const Q8Loads& L, const HnswDeviceGraph& g, const Q8Query& qq, int d0,
                                                int acc[4]) {
    const int lc = g.ld8 - 16, dlast = lc - Q8_PER;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int d = d0 + Q8_SPAN * it;
        const bool ok = d < lc;
        const int dc = d < dlast ? d : dlast;
        const i32x4 qv = *reinterpret_cast<const i32x4*>(qq.codes + dc);
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[p] = q8_accum<KIND>(qv, L.bb[it][p], ok, acc[p]);
    }
}

// Keys of the query to the m rows listed in nbr[0..m) -> nd[0..m).
template <int KIND>
__device__ __forceinline__ void q8_distances(const HnswDeviceGraph& g, const Q8Query& qq, const int* nbr, float* nd, int m,
                                             int lane) {
    const int g8 = lane >> 3, sub = lane & 7;
    const int lc = g.ld8 - 16;
    for (int base_i = 0; base_i < m; base_i += 32) {
        Q8Loads L;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            // slots past m re-read the last row (a cache hit) instead of branching
            const int idx = base_i + p * 8 + g8;
            L.ids[p] = nbr[idx < m ? idx : m - 1];
        }
        int acc[4] = {0, 0, 0, 0};
        q8_load_norms(L, g);
        for (int d0 = sub * Q8_PER; d0 < lc; d0 += Q8_STEP) {
            q8_load_step(L, g, d0);
            __builtin_amdgcn_sched_barrier(0);
            q8_consume_step<KIND>(L, g, qq, d0, acc);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int tot = group8_sum_i(acc[p]);
            const int idx = base_i + p * 8 + g8;
            if (sub == 0 && idx < m) nd[idx] = q8_key<KIND>(tot, L.xn[p], qq);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Split-phase form for the pipeline across expansions: issue() requests the first four loads and the slot of the first 32
// rows and returns; finish() consumes them, fetches what is left (longer rows, rows 32..m) and writes nd[0..m).
__device__ __forceinline__ void q8_issue(Q8Loads& L, const HnswDeviceGraph& g, const int* nbr, int m, int lane) {
    const int g8 = lane >> 3, sub = lane & 7;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int idx = p * 8 + g8;
        L.ids[p] = nbr[idx < m ? idx : m - 1];
    }
    q8_load_norms(L, g);
    q8_load_step(L, g, sub * Q8_PER);
    __builtin_amdgcn_sched_barrier(0);
}
template <int KIND>
__device__ __forceinline__ void q8_finish(Q8Loads& L, const HnswDeviceGraph& g, const Q8Query& qq, const int* nbr, float* nd,
                                          int m, int lane) {
    const int g8 = lane >> 3, sub = lane & 7;
    const int lc = g.ld8 - 16;
    int acc[4] = {0, 0, 0, 0};
    for (int d0 = sub * Q8_PER; d0 < lc; d0 += Q8_STEP) {
        if (d0 != sub * Q8_PER) {
            q8_load_step(L, g, d0);
            __builtin_amdgcn_sched_barrier(0);
        }
        q8_consume_step<KIND>(L, g, qq, d0, acc);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int tot = group8_sum_i(acc[p]);
        const int idx = p * 8 + g8;
        if (sub == 0 && idx < m) nd[idx] = q8_key<KIND>(tot, L.xn[p], qq);
    }
    __builtin_amdgcn_wave_barrier();
    if (m > 32) q8_distances<KIND>(g, qq, nbr + 32, nd + 32, m - 32, lane);
}

// ---- the walk ------------------------------------------------------------------------------------------------------
// hnsw_walk_body's policy for the copy.  LDS as hnsw_make_plan sizes it for the f32 kernel: the query's slot is [ldv]
// floats there; here it holds the codes, a quarter of it.  External queries on level 0 only (the graph is built from the
// f32 rows), no phase clocks, and the result is the sorted array as it stands, unpadded, for the re-rank.
template <int KIND>
struct Q8Walk {
    static constexpr bool kBuild = false, kProf = false, kRaw = true, kPad = false;
    using Loads = Q8Loads;
    Q8Query qq;
    static __device__ __forceinline__ int slot_floats(const HnswDeviceGraph& g) { return g.ldv; }
    // The query's codes: once, in LDS.
    // l2, l1: the index's unit, clamped (a query far outside the data saturates).  Dot kinds: only the order of q.x matters,
    // so the query -- normalised first where the f32 kernels normalise it, with their operations -- takes a unit of its own
    // that puts its largest |element| into [64, 128).
    __device__ __forceinline__ void stage(const HnswArgs& a, int q, float* slot, int lane) {
        const HnswDeviceGraph& g = a.g;
        uint8_t* qc = reinterpret_cast<uint8_t*>(slot);  // [ld8 - 16]
        qq.codes = qc;
        qq.cosnorm = g.space == SP_COSINE || g.space == SP_ANGULAR;
        const float* src = reinterpret_cast<const float*>(a.queries) + (size_t)q * g.dim;
        const int lc = g.ld8 - 16;
        float ss = 0.f, mx = 0.f;
        for (int d = lane; d < g.dim; d += 64) {
            const float v = src[d];
            ss = fmaf(v, v, ss);
            mx = fmaxf(mx, fabsf(v));
        }
        float inv = 1.0f;
        if (g.normalize_query) {
            ss = wave_sum(ss);
            if (ss != 0.0f) inv = 1.0f / sqrtf(ss);
        }
        float mult;
        if constexpr (KIND == Q8_DOT) {
            // (rounding is monotone: the largest |v * inv| is the largest |v| times inv)
            const float qmax = wave_max(mx) * inv;
            int ex = 0;
            const bool fin = qmax > 0.f && qmax < INFINITY;
            if (fin) (void)frexpf(qmax, &ex);
            const int e = 7 - ex;
            mult = fin ? ldexpf(1.0f, e < -100 ? -100 : (e > 100 ? 100 : e)) : 1.0f;
        } else {
            mult = ldexpf(1.0f, -g.scale8_exp);
        }
        int qn = 0;
        for (int d = lane; d < lc; d += 64) {
            int c = 0;
            if (d < g.dim) {
                float v = src[d];
                if (g.normalize_query) v *= inv;
                c = q8pack::code(v * mult);
            }
            qn += c * c;
            qc[d] = (uint8_t)(KIND == Q8_L1 ? (c + 128) : c);
        }
        qq.qn = KIND == Q8_L2 ? wave_sum_i(qn) : 0;
    }
    __device__ __forceinline__ void distances(const HnswDeviceGraph& g, const int* nbr, float* nd, int m, int lane) const {
        q8_distances<KIND>(g, qq, nbr, nd, m, lane);
    }
    __device__ __forceinline__ void issue(Loads& L, const HnswDeviceGraph& g, const int* nbr, int m, int lane) const {
        q8_issue(L, g, nbr, m, lane);
    }
    __device__ __forceinline__ void finish(Loads& L, const HnswDeviceGraph& g, const int* nbr, float* nd, int m, int lane) const {
        q8_finish<KIND>(L, g, qq, nbr, nd, m, lane);
    }
};

template <int KIND, bool BITSET, int EMAX, bool WIDE>
__global__ __launch_bounds__(64) void hnsw_search_q8_kernel(HnswArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using P = Q8Walk<KIND>;
    HNSW_WALK_QUERIES(P, BITSET, EMAX, WIDE, a, smem);
}

// ---- host side -----------------------------------------------------------------------------------------------------
template <int KIND, int EMAX, bool WIDE>
static hipError_t launch_q8_w(const HnswArgs& a, const HnswSearchPlan& p, hipStream_t s) {
    auto go = [&](auto kern, int grid) -> hipError_t {
        // (the dynamic LDS is named to the runtime: plans beyond the default 64 KiB exist for long rows)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64), p.lds_bytes, s, a);
        return hipGetLastError();
    };
    if (p.table_size == 0) return go(hnsw_search_q8_kernel<KIND, true, EMAX, WIDE>, a.fix_mode ? a.fix_mode : a.nq);
    return go(hnsw_search_q8_kernel<KIND, false, EMAX, WIDE>, a.nq);
}

template <int KIND>
static hipError_t launch_q8_kind(const HnswArgs& a, const HnswSearchPlan& p, hipStream_t s) {
    const bool wide = hnsw_wide(a.g);
    switch (hnsw_emax(p.cap)) {
        case 2: return wide ? launch_q8_w<KIND, 2, true>(a, p, s) : launch_q8_w<KIND, 2, false>(a, p, s);
        case 4: return wide ? launch_q8_w<KIND, 4, true>(a, p, s) : launch_q8_w<KIND, 4, false>(a, p, s);
        default: return wide ? launch_q8_w<KIND, 16, true>(a, p, s) : launch_q8_w<KIND, 16, false>(a, p, s);
    }
}

hipError_t launch_hnsw_search_q8(const HnswDeviceGraph& g, const HnswSearchPlan& p, const HnswQueries& q, uint32_t* bitset,
                                 const HnswOverflow& fix, const HnswOut& out, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    // the limits of launch_hnsw_search, and what is this kernel's own: a copy of these rows, external queries, the whole
    // array asked for, the codes within the query's slot
    if (p.cap > 64 * 16 || hnsw_nbcap(g) > HNSW_NBCAP_LDS || p.lds_bytes > HNSW_LDS_LIMIT) return hipErrorInvalidValue;
    if (!g.rows8 || g.ld8 != (int)q8pack::row_stride((size_t)g.dim) || g.ld8 - 16 > g.ldv * 4) return hipErrorInvalidValue;
    if (!q.queries || q.query_rows || q.start_nodes || q.level != 0 || p.k != p.cap) return hipErrorInvalidValue;
    if (p.table_size == 0 && !bitset) return hipErrorInvalidValue;
    const HnswArgs a = hnsw_walk_args(g, p, q, bitset, fix, out);
    switch (g.space) {
        case SP_L2:
        case SP_L2SQR: return launch_q8_kind<Q8_L2>(a, p, s);
        case SP_L1: return launch_q8_kind<Q8_L1>(a, p, s);
        case SP_NORMCOS:
        case SP_COSINE:
        case SP_ANGULAR:
        case SP_NEGDOT: return launch_q8_kind<Q8_DOT>(a, p, s);
        default: return hipErrorInvalidValue;  // linf, l2sqr_sift: not served
    }
}

}  // namespace gfxknn
