// Exact bit_jaccard k-NN on the int8 matrix cores (the plan: jac_fast_plan.hpp).
//
// d(q, b) = 1 - num / den,  num = |q & b| = sum_c b_c q_c,  den = |q | b| = |q| + |b| - num.  With both codes as int8 0 / 1,
// v_mfma_i32_32x32x32_i8 accumulates num exactly from 0.  The layout is the bit_hamming scan's (ham_mfma_kernels.hip): one
// wave per workgroup, 4 row groups x 2 query groups of 32 x 32 accumulators, packed words expanded to bytes in registers,
// the tile's query words word-major in LDS, a sample pass for the thresholds, per-split lists merged by
// launch_merge_topk_ex.  What the float distance changes:
//   |b|.  The lane that loads the word of row l31 of a row group counts it (one v_bcnt per K-step and row group); the
//   accumulator values of a lane belong to 16 other rows (8 j + 4 h + i), so after the K loop the 128 counts of the block go
//   through s_pb in LDS, once per block, and are read back as four 16-byte reads per row group.
//   No division in the loop.  A query's threshold is an f32 distance t; d <= t implies (below)
//       num - G |b| >= R,   G <= g,  R <= g |q|,  g = c / (1 + c),  c <= (1 - t - 2^-25) / (1 + 2^-24)
//   which costs a conversion, an FMA and a max per value; one max over a lane's 16 values stands in front of the
//   out-of-line path, which repeats the test per value, computes the exact distance with jac_distance (jaccard_dev.hpp)
//   and appends the key when it is below the threshold key.
//   The argument.  x -> fl(x) and x -> fl(1 - x) are monotone, and for x in [0, 1] the subtraction errs by at most 2^-25
//   (half an ulp of a result <= 1).  So d = fl(1 - fl(rho)) <= t gives 1 - fl(rho) <= t + 2^-25, and with
//   fl(rho) <= rho (1 + 2^-24):  rho = num / den >= (1 - t - 2^-25) / (1 + 2^-24) >= c.  For c >= 0 and den > 0 that is
//   num >= c (|q| + |b| - num), i.e. num >= g (|q| + |b|), i.e. num - g |b| >= g |q| >= 0.  The test evaluates
//   fma(-G, |b|, num) with G <= g in f32: the exact value num - G |b| is at least num - g |b|, and one rounding takes at most
//   2^-24 of it, so the result is at least g |q| (1 - 2^-24) >= R.  c < 0 (t = 1: every row is within the threshold) sets
//   G = 0, R = -1: every value passes.  den = 0 means num = |b| = |q| = 0: the test reads 0 >= R with R = 0 (or -1) and
//   passes, as it must (d = 0 <= t).  c, g, G and R are computed in double with relative margins of 2^-22, far above the
//   2^-52 of those few operations, and rounded down to f32.  The test is on the rational and only ever a superset: two
//   rationals that round to one f32 distance are told apart (or not) by the exact keys alone.
//   Keys.  (f32 bits of d << 32) | row within the split, u64: a non-negative float orders as its bits.  A key passes when it
//   is below the threshold key; the bound of the sample pass gives ((bits of t) + 1) << 32, so rows AT the k-th sample
//   distance pass and position decides among them.  Lists are [cap][64] u64 in LDS, cut as in the bit_hamming scan.
#include "bit_list_dev.hpp"
#include "jaccard_dev.hpp"

namespace gfxknn {

namespace {

constexpr uint32_t kOnes = 0x01010101u;
constexpr u64 kNoKey = ~0ull;
constexpr uint32_t kOneBits = 0x3F800000u;   // 1.0f

// the 16 operand bytes (0 / 1) of a lane from one packed word (xs = word >> 4 h): bits d + 8 j of xs in dword d, byte j
__device__ __forceinline__ i32x4 jac_operand(uint32_t xs) {
    i32x4 v;
    v[0] = (int)(xs & kOnes);
    v[1] = (int)((xs >> 1) & kOnes);
    v[2] = (int)((xs >> 2) & kOnes);
    v[3] = (int)((xs >> 3) & kOnes);
    return v;
}

// the superset test's constants of a query with |q| = pq whose keys must stay below thr
__device__ __forceinline__ void jac_filter(u64 thr, int pq, float& G, float& R) {
    const uint32_t hi = (uint32_t)(thr >> 32);   // a passing key has d <= the float of these bits (d < it when the low half is 0)
    G = 0.0f;
    R = -1.0f;
    if (hi >= kOneBits) return;
    const double margin = 1.0 - 0x1p-22;
    const double c = (1.0 - (double)__uint_as_float(hi) - 0x1p-25) / (1.0 + 0x1p-24) * margin;
    if (c < 0.0) return;
    const double g = c / (1.0 + c) * margin;
    G = __double2float_rd(g);
    R = __double2float_rd(g * (double)pq * margin);
}

template <bool VEC>
__global__ __launch_bounds__(64) void jac_mfma_knn_kernel(const uint32_t* __restrict__ rows, int W, int n,
                                                          int rows_per_split, const uint32_t* __restrict__ q, int nq,
                                                          int k, int cap, const float* __restrict__ bound,
                                                          float* __restrict__ out_d, int32_t* __restrict__ out_pos) {
    constexpr int QB = hamfast::kQueryGroups;
    constexpr int QT = 32 * QB;   // queries of the tile = lists = lanes
    static_assert(QT == 64, "a cut gives every lane one list");
    static_assert(jacfast::kPopRows == 128, "four row groups of 32");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* s_q = reinterpret_cast<uint32_t*>(smem);                   // [W][QT]
    u64* s_keys = reinterpret_cast<u64*>(s_q + (size_t)W * QT);          // [cap][QT]
    int* s_cnt = reinterpret_cast<int*>(s_keys + (size_t)cap * QT);      // [QT]
    int* s_pb = s_cnt + QT;                                              // [128]: |b| of the block's rows
    const int lane = threadIdx.x, l31 = lane & 31, h = lane >> 5;
    const int split = blockIdx.x, q_first = blockIdx.y * QT;

    // the queries of a partial tile repeat the batch's last one (their results are not written)
    for (int i = lane; i < W * QT; i += 64) {
        const int w = i / QT, t = i - w * QT;
        s_q[i] = q[(size_t)min(q_first + t, nq - 1) * W + w];
    }
    s_cnt[lane] = 0;
    __syncthreads();

    int pq[QB];
    u64 thr[QB];
    float G[QB], R[QB];
#pragma unroll
    for (int g = 0; g < QB; ++g) {
        int s = 0;
        for (int w = 0; w < W; ++w) s += __popc(s_q[w * QT + g * 32 + l31]);
        pq[g] = s;
        // bound: the k best distances of the query over a sample of the rows.  k rows lie within the k-th of them, so no
        // row beyond it is among the k nearest; rows AT it still pass (position decides among equal distances)
        thr[g] = bound ? ((u64)__float_as_uint(bound[(size_t)min(q_first + g * 32 + l31, nq - 1) * k + (k - 1)]) + 1) << 32
                       : kNoKey;
        jac_filter(thr[g], pq[g], G[g], R[g]);
    }

    // every list cut to its k smallest keys (bit_list_dev.hpp); a full list's k-th key is its query's new threshold
    auto cut = [&]() __attribute__((always_inline)) {
        bit_list_cut<u64, QT>(s_keys, s_cnt, lane, cap, k, kNoKey);
#pragma unroll
        for (int g = 0; g < QB; ++g)
            if (s_cnt[g * 32 + l31] >= k) {
                thr[g] = s_keys[(size_t)(k - 1) * QT + g * 32 + l31];
                jac_filter(thr[g], pq[g], G[g], R[g]);
            }
    };

    const int r0 = (int)min((long long)split * rows_per_split, (long long)n);
    const int lim = min(n - r0, rows_per_split);   // rows of the split
    const uint32_t sh = 4u * h;

    for (int base = 0; base < lim; base += hamfast::kRowBlock) {
        // rows at or beyond the split's end read the store's last row; they are never offered
        const uint32_t* rp[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) rp[rb] = rows + (size_t)min(r0 + base + rb * 32 + l31, n - 1) * W;
        i32x16 acc[4][QB];
        int pb[4];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            pb[rb] = 0;
#pragma unroll
            for (int g = 0; g < QB; ++g)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[rb][g][i] = 0;
        }

        uint32_t cur[4][4], nxt[4][4] = {};
        bit_rows_load<VEC>(rp, 0, W, cur);
        for (int w0 = 0; w0 < W; w0 += 4) {
            // the next four words are in flight under this chunk's MFMAs
            if (w0 + 4 < W) bit_rows_load<VEC>(rp, w0 + 4, W, nxt);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (w0 + j < W) {
                    i32x4 a[4], b[QB];
#pragma unroll
                    for (int rb = 0; rb < 4; ++rb) {
                        a[rb] = jac_operand(cur[rb][j] >> sh);
                        pb[rb] += __popc(cur[rb][j]);
                    }
#pragma unroll
                    for (int g = 0; g < QB; ++g) b[g] = jac_operand(s_q[(w0 + j) * QT + g * 32 + l31] >> sh);
#pragma unroll
                    for (int g = 0; g < QB; ++g)
#pragma unroll
                        for (int rb = 0; rb < 4; ++rb)
                            acc[rb][g] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[rb], b[g], acc[rb][g], 0, 0, 0);
                }
            }
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
#pragma unroll
                for (int j = 0; j < 4; ++j) cur[rb][j] = nxt[rb][j];
        }

        // |b| of row rb * 32 + l31 of the block, from the lanes that loaded it (both halves hold the same count) to the
        // lanes that hold its accumulator values
        __syncthreads();   // (one wave: the previous block's reads of s_pb are done)
        if (h == 0) {
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) s_pb[rb * 32 + l31] = pb[rb];
        }
        __syncthreads();

        // accumulator register 4 j + i of half h = row 8 j + 4 h + i of its 32-row group, query l31 of its group
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            float pbf[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int4 v = *reinterpret_cast<const int4*>(s_pb + rb * 32 + 8 * j + 4 * h);
                pbf[4 * j + 0] = (float)v.x;
                pbf[4 * j + 1] = (float)v.y;
                pbf[4 * j + 2] = (float)v.z;
                pbf[4 * j + 3] = (float)v.w;
            }
#pragma unroll
            for (int g = 0; g < QB; ++g) {
                const i32x16& c = acc[rb][g];
                float m = fmaf(-G[g], pbf[0], (float)c[0]);
#pragma unroll
                for (int i = 1; i < 16; ++i) m = fmaxf(m, fmaf(-G[g], pbf[i], (float)c[i]));
                if (__builtin_expect(__any(m >= R[g]), 0)) {
                    // the two lanes of a query append up to 32 keys: cap >= k + 32 always leaves room behind a cut
                    __syncthreads();
                    if (__any(s_cnt[g * 32 + l31] + 32 > cap)) cut();
                    const int rr0 = base + rb * 32 + 4 * h;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int rr = rr0 + 8 * (i >> 2) + (i & 3);
                        if (rr < lim && fmaf(-G[g], pbf[i], (float)c[i]) >= R[g]) {
                            const float d = jac_distance(c[i], pq[g] + (int)pbf[i] - c[i]);
                            const u64 key = ((u64)__float_as_uint(d) << 32) | (uint32_t)rr;
                            if (key < thr[g]) s_keys[(size_t)atomicAdd(&s_cnt[g * 32 + l31], 1) * QT + g * 32 + l31] = key;
                        }
                    }
                }
            }
        }
    }

    // lane t writes the list of query t; queries beyond nq write nothing
    cut();
    const int qi = q_first + lane;
    if (qi < nq) {
        const int c = s_cnt[lane];
        const size_t o = ((size_t)split * nq + qi) * (size_t)k;
        for (int e = 0; e < k; ++e) {
            const u64 key = s_keys[(size_t)min(e, cap - 1) * QT + lane];
            out_pos[o + e] = e < c ? r0 + (int)(uint32_t)key : -1;
            out_d[o + e] = e < c ? __uint_as_float((uint32_t)(key >> 32)) : INFINITY;
        }
    }
}

template <bool VEC>
hipError_t launch_one(const jacfast::Plan& p, int nsplit, int rows_per_split, const uint32_t* rows, int n, const uint32_t* q,
                      int nq, int k, const float* bound, float* split_d, int32_t* split_pos, hipStream_t s) {
    auto kernel = jac_mfma_knn_kernel<VEC>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)p.lds);
    if (e != hipSuccess) return e;
    const dim3 grid(nsplit, (nq + p.tile - 1) / p.tile);
    hipLaunchKernelGGL(kernel, grid, dim3(64), p.lds, s, rows, p.W, n, rows_per_split, q, nq, k, p.cap, bound, split_d,
                       split_pos);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_jac_mfma_knn(const jacfast::Plan& p, bool sample, const uint32_t* rows, int n, const uint32_t* q, int nq,
                               int k, const float* bound, float* split_d, int32_t* split_pos, hipStream_t s) {
    if (!p.use || nq <= 0 || p.qb != hamfast::kQueryGroups || p.lds != jacfast::lds_bytes(p.W, p.cap, p.tile))
        return hipErrorInvalidValue;
    const int nsplit = sample ? p.sample_nsplit : p.nsplit, rps = sample ? p.sample_rows / p.sample_nsplit : p.rows_per_split;
    if (sample) n = p.sample_rows;
    return (p.W & 3) == 0 ? launch_one<true>(p, nsplit, rps, rows, n, q, nq, k, bound, split_d, split_pos, s)
                          : launch_one<false>(p, nsplit, rps, rows, n, q, nq, k, bound, split_d, split_pos, s);
}

}  // namespace gfxknn
