// Exact k-NN and range search over the divergence spaces of dense float rows: KL, generalized KL, Itakura-Saito
// (the Bregman family, src/distcomp_bregman.cc) and Jensen-Shannon (src/distcomp_js.cc).
//
// An object is its values plus their logarithms, both computed on the host (diverg.cpp) by the reference's rules, so
// the "fast" formulas contain no transcendental here.  Storage:
//   rows    : two planes (values, logs), each [ceil(n/64)][G][64][4] floats, G = ceil(D/4): the four elements of group
//             g of row r are one 16-byte load at ((r/64 * G + g) * 64 + r%64), consecutive rows in consecutive lanes
//   queries : planes (values, logs, and for Itakura-Saito the reciprocals), each [G][stride][4] floats: the group-g
//             elements of consecutive queries are consecutive, their address is the same for a whole wave
//
//   diverg_knn_kernel  : one workgroup scans one row range for a tile of TQ queries (16 when k is small, else 1),
//                        one row per thread.  A row group is loaded once and used against every query of the tile
//                        from registers; the query operands are wave-uniform loads (scalar registers).  The best kl
//                        keys per query are kept in LDS (SplitTopK, split_topk_dev.hpp); the per-split lists are
//                        merged by launch_merge_topk_ex.
//   diverg_dist_kernel : d(row, query) and d(query, row) for every row (range search: the filter uses the first, the
//                        reported distance is the second, rangequery.cc:78-82 and nmslib_c.cpp:1104-1113).
//   diverg_pair_kernel : nmslib_get_distance.
//
// Summation order of one pair (DivAcc), the same in every kernel, tile, split and batch:
//   KL / generalized KL / Itakura-Saito "fast": the reference's SSE order -- four running sums over i mod 4 for
//     i < 4*floor(D/4) with product and sum rounded separately, combined ((s0 + s1) + s2) + s3, then the last D mod 4
//     elements one by one as the reference's build evaluates them (clang contracts a*b + c of one expression: FMA).
//     Itakura-Saito multiplies by the rounded reciprocal of obj2 instead of dividing (at most 1.5 ulp per quotient).
//   kldivgenslow, Jensen-Shannon: one running sum (JS: two) over i = 0 .. D-1, the reference's loops.
// This file is compiled with -ffp-contract=off; the FMAs are explicit.
#include "kernels.hpp"
#include "split_topk_dev.hpp"

namespace gfxknn {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

enum DivergFormula : int { DV_KL, DV_KLGEN, DV_KLGEN_SLOW, DV_IS, DV_JS };

constexpr float kFltMin = 1.17549435e-38f;  // numeric_limits<float>::min()

// Accumulators of one pair: obj1 = (x, lx), obj2 = (y, ly, iy = 1 / y)
template <int F>
struct DivAcc {
    f32x2 s01 = {0.f, 0.f}, s23 = {0.f, 0.f};  // running sums of elements i mod 4 = 0, 1 and 2, 3 (packed f32 math)
    float r = 0.f, r2 = 0.f;                   // the sequential sums; after combine() the pair's sum

    __device__ __forceinline__ void seq(float x, float lx, float y, float ly) {
        if constexpr (F == DV_KLGEN_SLOW) {  // KLGeneralStandard, distcomp_bregman.cc:277-286
            r = r + (fmaf(x, logf(x / y), y) - x);
        } else {  // JSStandard / JSPrecomp, distcomp_js.cc:47-87
            r = r + (x * lx + y * ly);
            const float m = 0.5f * (x + y);
            if (m >= kFltMin) r2 = r2 + m * logf(m);
        }
    }

    // elements 4g .. 4g+3 of a complete group
    __device__ __forceinline__ void group(f32x4 x, f32x4 lx, f32x4 y, f32x4 ly, f32x4 iy) {
        if constexpr (F == DV_KL) {  // KLPrecompSIMD, distcomp_bregman.cc:213-273
            s01 = s01 + x.xy * (lx.xy - ly.xy);
            s23 = s23 + x.zw * (lx.zw - ly.zw);
        } else if constexpr (F == DV_KLGEN) {  // KLGeneralPrecompSIMD, :325-393
            s01 = (s01 + x.xy * (lx.xy - ly.xy)) + (y.xy - x.xy);
            s23 = (s23 + x.zw * (lx.zw - ly.zw)) + (y.zw - x.zw);
        } else if constexpr (F == DV_IS) {  // ItakuraSaitoPrecompSIMD, :80-146
            s01 = s01 + (x.xy * iy.xy - (lx.xy - ly.xy));
            s23 = s23 + (x.zw * iy.zw - (lx.zw - ly.zw));
        } else {
            seq(x.x, lx.x, y.x, ly.x);
            seq(x.y, lx.y, y.y, ly.y);
            seq(x.z, lx.z, y.z, ly.z);
            seq(x.w, lx.w, y.w, ly.w);
        }
    }

    // after the last complete group
    __device__ __forceinline__ void combine() {
        if constexpr (F == DV_KL || F == DV_KLGEN || F == DV_IS) r = ((s01.x + s01.y) + s23.x) + s23.y;
    }

    // one of the last D mod 4 elements
    __device__ __forceinline__ void tail(float x, float lx, float y, float ly, float iy) {
        if constexpr (F == DV_KL) r = fmaf(x, lx - ly, r);
        else if constexpr (F == DV_KLGEN) r = r + (fmaf(x, lx - ly, y) - x);
        else if constexpr (F == DV_IS) r = r + (x * iy - (lx - ly));
        else seq(x, lx, y, ly);
    }

    __device__ __forceinline__ float finish(int D, int metr) const {
        if constexpr (F == DV_IS) return r - (float)D;
        if constexpr (F == DV_JS) {
            const float v = 0.5f * r - r2;
            const float c = v < 0.0f ? 0.0f : v;  // std::max(v, 0)
            return metr ? sqrtf(c) : c;           // space_js.h:99-101
        }
        return r;
    }
};

// the last D mod 4 elements, held in one (partial) group
template <int F>
__device__ __forceinline__ void tail_group(DivAcc<F>& a, int rem, f32x4 x, f32x4 lx, f32x4 y, f32x4 ly, f32x4 iy) {
    if (rem > 0) a.tail(x.x, lx.x, y.x, ly.x, iy.x);
    if (rem > 1) a.tail(x.y, lx.y, y.y, ly.y, iy.y);
    if (rem > 2) a.tail(x.z, lx.z, y.z, ly.z, iy.z);
}

// TQ queries per workgroup; REV: the space's distance is the formula with its arguments exchanged (the *rq spaces)
template <int F, bool REV, int TQ>
__global__ __launch_bounds__(256) void diverg_knn_kernel(const f32x4* __restrict__ rv, const f32x4* __restrict__ rl,
                                                         int n, int D, int G, int rows_per_split,
                                                         const f32x4* __restrict__ qv, const f32x4* __restrict__ ql,
                                                         const f32x4* __restrict__ qi, int qstride, int q0, int nq,
                                                         int ntiles, int k, int kl, int P, int metr,
                                                         float* __restrict__ out_d, int32_t* __restrict__ out_pos) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_cnt[TQ];
    // the tiles of one row range run side by side: what one of them brings into the L2 the others find there
    const int tid = threadIdx.x, tile = blockIdx.x % ntiles, split = blockIdx.x / ntiles, q_first = tile * TQ;
    const int tile_n = min(TQ, nq - q_first);
    SplitTopK<TQ> sel{reinterpret_cast<u64*>(smem), s_cnt, P, kl, tile_n};
    sel.init(tid);
    __syncthreads();
    const int r0 = (int)min((long long)split * rows_per_split, (long long)n);
    const int r1 = min(n, r0 + rows_per_split);
    const int G4 = D >> 2, rem = D & 3;
    const size_t qb = (size_t)q0 + q_first;  // the pack holds TQ queries from here on (diverg.cpp pads it)
    for (int base = r0; base < r1; base += 256) {
        const int r = base + tid;
        const int rr = min(r, n - 1);  // a thread past the range works on a valid row and offers nothing
        const size_t ro = (size_t)(rr >> 6) * G * 64 + (rr & 63);
        const f32x4* pv = rv + ro;
        const f32x4* pl = rl + ro;
        DivAcc<F> acc[TQ];
        f32x4 x = pv[0], lx = pl[0];
        for (int g = 0; g < G4; ++g) {
            f32x4 xn = x, lxn = lx;
            if (g + 1 < G) {  // the next group's loads fly while this one is used
                xn = pv[(size_t)(g + 1) * 64];
                lxn = pl[(size_t)(g + 1) * 64];
            }
            const size_t qo = (size_t)g * qstride + qb;
#pragma unroll
            for (int t = 0; t < TQ; ++t) {
                const f32x4 y = qv[qo + t], ly = ql[qo + t];
                if constexpr (REV) {
                    acc[t].group(y, ly, x, lx, x);
                } else {
                    f32x4 iy = y;
                    if constexpr (F == DV_IS) iy = qi[qo + t];
                    acc[t].group(x, lx, y, ly, iy);
                }
            }
            x = xn;
            lx = lxn;
        }
        const size_t qo = (size_t)G4 * qstride + qb;
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
            acc[t].combine();
            if (rem) {
                const f32x4 y = qv[qo + t], ly = ql[qo + t];
                if constexpr (REV) {
                    tail_group<F>(acc[t], rem, y, ly, x, lx, x);
                } else {
                    f32x4 iy = y;
                    if constexpr (F == DV_IS) iy = qi[qo + t];
                    tail_group<F>(acc[t], rem, x, lx, y, ly, iy);
                }
            }
            const float d = acc[t].finish(D, metr);
            // -0 and +0 are one distance (the reference's queue compares them equal): one key for both
            if (t < tile_n && r < r1) sel.offer(t, f32_ord(d == 0.0f ? 0.0f : d), r);
        }
        sel.chunk_done(tid, base + 256 >= r1);
    }
    sel.write(tid, split, nq, q_first, k, out_d, out_pos, [](uint32_t hi) { return ord_f32(hi); });
}

// formula(obj1 = a, obj2 = b): group g of an object at p[g * stride]; the reciprocals of obj2 are taken here
template <int F>
__device__ __forceinline__ float diverg_eval(int D, const f32x4* av, const f32x4* al, size_t sa, const f32x4* bv,
                                             const f32x4* bl, size_t sb, int metr) {
    DivAcc<F> acc;
    const int G4 = D >> 2, rem = D & 3;
    for (int g = 0; g < G4; ++g) {
        const f32x4 y = bv[g * sb];
        acc.group(av[g * sa], al[g * sa], y, bl[g * sb], 1.0f / y);
    }
    acc.combine();
    if (rem) {
        const f32x4 y = bv[G4 * sb];
        f32x4 iy = {1.0f / y.x, rem > 1 ? 1.0f / y.y : 0.f, rem > 2 ? 1.0f / y.z : 0.f, 0.f};
        tail_group<F>(acc, rem, av[G4 * sa], al[G4 * sa], y, bl[G4 * sb], iy);
    }
    return acc.finish(D, metr);
}

template <int F, bool REV>
__global__ __launch_bounds__(256) void diverg_dist_kernel(const f32x4* __restrict__ rv, const f32x4* __restrict__ rl,
                                                          int n, int D, int G, const f32x4* __restrict__ qv,
                                                          const f32x4* __restrict__ ql, int qstride, int metr,
                                                          float* __restrict__ d_row_q, float* __restrict__ d_q_row) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
        const size_t ro = (size_t)(r >> 6) * G * 64 + (r & 63);
        const float f = diverg_eval<F>(D, rv + ro, rl + ro, 64, qv, ql, (size_t)qstride, metr);  // formula(row, query)
        const float b = diverg_eval<F>(D, qv, ql, (size_t)qstride, rv + ro, rl + ro, 64, metr);  // formula(query, row)
        d_row_q[r] = REV ? b : f;
        d_q_row[r] = REV ? f : b;
    }
}

// the two objects are queries 0 and 1 of a pack with stride 2
template <int F, bool REV>
__global__ void diverg_pair_kernel(const f32x4* __restrict__ v, const f32x4* __restrict__ l, int D, int metr,
                                   float* __restrict__ out) {
    if (threadIdx.x != 0) return;
    *out = REV ? diverg_eval<F>(D, v + 1, l + 1, 2, v, l, 2, metr) : diverg_eval<F>(D, v, l, 2, v + 1, l + 1, 2, metr);
}

template <template <int, bool> class Launch, typename... Args>
hipError_t dispatch_space(int space, Args... args) {
    switch (space) {
        case SP_KLDIV: return Launch<DV_KL, false>::run(0, args...);
        case SP_KLDIV_RQ: return Launch<DV_KL, true>::run(0, args...);
        case SP_KLDIVGEN: return Launch<DV_KLGEN, false>::run(0, args...);
        case SP_KLDIVGEN_RQ: return Launch<DV_KLGEN, true>::run(0, args...);
        case SP_KLDIVGEN_SLOW: return Launch<DV_KLGEN_SLOW, false>::run(0, args...);
        case SP_ITAKURASAITO: return Launch<DV_IS, false>::run(0, args...);
        case SP_JSDIV:
        case SP_JSDIV_SLOW: return Launch<DV_JS, false>::run(0, args...);
        case SP_JSMETR:
        case SP_JSMETR_SLOW: return Launch<DV_JS, false>::run(1, args...);
        default: return hipErrorInvalidValue;
    }
}

inline const f32x4* v4(const float* p) { return reinterpret_cast<const f32x4*>(p); }

template <int F, bool REV>
struct KnnLaunch {
    static hipError_t run(int metr, const ScanPlan& p, const DivergRows& rows, const DivergQueries& q, int q0,
                          float* out_d, int32_t* out_pos, hipStream_t s) {
        const int ntiles = (p.nq + p.tq - 1) / p.tq;
        const dim3 grid((unsigned)((size_t)ntiles * p.nsplit));
        const size_t lds = (size_t)p.tq * p.P * 8;
        if (p.tq == kDivergTileQ)
            return launch_with_lds(diverg_knn_kernel<F, REV, kDivergTileQ>, grid, lds, s, v4(rows.vals), v4(rows.logs),
                                   rows.n, rows.D, rows.G, p.rows_per_split, v4(q.vals), v4(q.logs), v4(q.inv),
                                   q.stride, q0, p.nq, ntiles, p.k, p.kl, p.P, metr, out_d, out_pos);
        return launch_with_lds(diverg_knn_kernel<F, REV, 1>, grid, lds, s, v4(rows.vals), v4(rows.logs), rows.n, rows.D,
                               rows.G, p.rows_per_split, v4(q.vals), v4(q.logs), v4(q.inv), q.stride, q0, p.nq, ntiles,
                               p.k, p.kl, p.P, metr, out_d, out_pos);
    }
};

template <int F, bool REV>
struct DistLaunch {
    static hipError_t run(int metr, const DivergRows& rows, const DivergQueries& q, float* d_row_q, float* d_q_row,
                          hipStream_t s) {
        int grid = (rows.n + 255) / 256;
        if (grid > 8192) grid = 8192;
        hipLaunchKernelGGL((diverg_dist_kernel<F, REV>), dim3(grid), dim3(256), 0, s, v4(rows.vals), v4(rows.logs),
                           rows.n, rows.D, rows.G, v4(q.vals), v4(q.logs), q.stride, metr, d_row_q, d_q_row);
        return hipGetLastError();
    }
};

template <int F, bool REV>
struct PairLaunch {
    static hipError_t run(int metr, const DivergQueries& objs, int D, float* out, hipStream_t s) {
        hipLaunchKernelGGL((diverg_pair_kernel<F, REV>), dim3(1), dim3(64), 0, s, v4(objs.vals), v4(objs.logs), D, metr,
                           out);
        return hipGetLastError();
    }
};

}  // namespace

hipError_t launch_diverg_knn(int space, const ScanPlan& p, const DivergRows& rows, const DivergQueries& q, int q0,
                             float* split_d, int32_t* split_pos, hipStream_t s) {
    if (p.nq <= 0) return hipSuccess;
    return dispatch_space<KnnLaunch>(space, p, rows, q, q0, split_d, split_pos, s);
}

hipError_t launch_diverg_dist(int space, const DivergRows& rows, const DivergQueries& q, float* d_row_q, float* d_q_row,
                              hipStream_t s) {
    if (rows.n <= 0) return hipSuccess;
    return dispatch_space<DistLaunch>(space, rows, q, d_row_q, d_q_row, s);
}

hipError_t launch_diverg_pair(int space, const DivergQueries& objs, int D, float* out, hipStream_t s) {
    return dispatch_space<PairLaunch>(space, objs, D, out, s);
}

}  // namespace gfxknn
