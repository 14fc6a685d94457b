// Fast path of the exact scan over jsdivslow, jsdivfast, jsmetrslow and jsmetrfast.  Jensen-Shannon has no
// inner-product form, but it has one with a single logarithm per element: JS = R_row + C_q - (ln2 / 2) sum s log2 s,
// s = x + y.  A filter scan takes that sum with the raw logarithm instruction (v_log_f32) where the exact scan spends an
// accurate logf, the exact scan's own formula (diverg_dev.hpp) re-ranks the rows it lists, and a per-query proof shows that
// no unlisted row can belong to the top k (re-rank and proof: diverg_mfma_kernels.hip).  Constants and the bound:
// ../diverg_js_filter.hpp.
// This file is compiled with diverg_kernels.hip's flags (-ffp-contract=off: the FMAs are explicit).
#include "kernels.hpp"
#include "diverg_dev.hpp"
#include "split_topk_dev.hpp"   // launch_with_lds

namespace gfxknn {

namespace {

using djs::kTileQ;
using dvf::kBuf;
using dvf::kKeep;

static_assert(kTileQ == dvf::kGroup && kBuf >= djs::kRowBlock + kKeep, "a step's 64 offers fit behind the kept keys");

// ---- per batch: the queries clamped to >= 2^-100, with C_q and E_q; the groups' flags cleared -----------------------------
// One thread per padded query.  The clamped plane is [G][qpad][4]; padding queries and the elements past D are the clamp
// (with the value plane's zeros they add 4 G 2^-100 log2 2^-100 at most, which the bound counts).
__global__ __launch_bounds__(64) void diverg_js_prep_kernel(const f32x4* qv, int qstride, int nq, int qpad, int dim, int G,
                                                            djs::RowMax m, f32x4* qclamp, double* ce, int* flags) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= qpad) return;
    const float c = djs::kClamp;
    for (int g = 0; g < G; ++g) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (q < nq) v = qv[(size_t)g * qstride + q];
        // (a NaN compares false and becomes the clamp: its query has no proof)
        qclamp[(size_t)g * qpad + q] = f32x4{v.x > c ? v.x : c, v.y > c ? v.y : c, v.z > c ? v.z : c, v.w > c ? v.w : c};
    }
    double C = 0, E = INFINITY;
    if (q < nq) djs::query(reinterpret_cast<const float*>(qv + q), (size_t)qstride * 4, (size_t)dim, m, &C, &E);
    ce[2 * (size_t)q] = C;
    ce[2 * (size_t)q + 1] = E;
    if (q % dvf::kGroup == 0) flags[q / dvf::kGroup] = 0;
}

// ---- the scan ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int lane_i(int v, int t) { return __builtin_amdgcn_readlane(v, t); }
__device__ __forceinline__ float lane_f(float v, int t) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), t)); }

// keeps the kKeep smallest of the c > kKeep buffered keys of one query (sorted) and returns the key part of the kKeep-th
__device__ __forceinline__ float js_compact(u64* keys, int c, int lane) {
    for (int i = lane; i < kBuf; i += 64)
        if (i >= c) keys[i] = ~0ull;
    __builtin_amdgcn_wave_barrier();
    wave_bitonic_u64(keys, kBuf, lane, false);
    const float t = ord_f32((uint32_t)(keys[kKeep - 1] >> 32));
    __builtin_amdgcn_wave_barrier();
    return t;
}

// Grid: (group of four neighbouring row splits, tile of kTileQ queries); a wave owns one split -- a contiguous 1/64 of the
// 64-row blocks -- and its kTileQ lists, and the four waves of a workgroup read the same query operands through the scalar
// cache.  One row per lane.  A row's value groups (16 bytes per lane per group of four elements) are loaded one group ahead,
// across block ends too: the groups of consecutive blocks are consecutive in the plane.  The clamped query operands of the
// tile have a wave-uniform address and come as scalar loads.  Per (row, query) two packed accumulators hold the lane sums
// i mod 4 = 0, 1 and 2, 3: per group 2 v_pk_add_f32, 4 v_log_f32, 2 v_pk_fma_f32.  key = fma(-ln2 / 2, ((a0 + a1) + a2) + a3,
// R32).  A query's threshold and list length live in lane t of two registers and are read as scalars (v_readlane); offers
// (key < threshold) take their places in the wave's own LDS buffer by ballot and mbcnt.  A buffer that the next block's 64
// offers could overflow is sorted and cut to the kKeep smallest, the largest of which becomes the threshold.  No barrier, no
// atomic, and no load under a divergent branch (an index past the plane is clamped, not skipped).
__global__ __launch_bounds__(256) void diverg_js_filter_kernel(const f32x4* __restrict__ rv, const float* __restrict__ r32,
                                                               const f32x4* __restrict__ qc, int n, int G, int nblocks,
                                                               int blocks_per_split, int qpad, int nsplit,
                                                               u64* __restrict__ cand, int* __restrict__ cand_cnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    u64* keys = reinterpret_cast<u64*>(smem) + (size_t)wave * kTileQ * kBuf;   // [kTileQ][kBuf]
    const int sgroups = nsplit >> 2;
    const int split = (int)(blockIdx.x % sgroups) * 4 + wave, q0 = (int)(blockIdx.x / sgroups) * kTileQ;
    const int blk0 = split * blocks_per_split;
    const int blk1 = blk0 + blocks_per_split < nblocks ? blk0 + blocks_per_split : nblocks;
    const long long last = (long long)nblocks * G - 1;   // the plane's last group of 64 rows
    const f32x4* qp = qc + q0;
    const float nhl2 = -(float)djs::kHalfLn2;

    int cnt_l = 0;             // lane t: keys in the buffer of query t
    float thr_l = INFINITY;    // lane t: its threshold

    long long li = (long long)blk0 * G;   // linear index of the group in hand
    f32x4 x = rv[(size_t)(li < last ? li : last) * 64 + lane];
    for (int blk = blk0; blk < blk1; ++blk) {
        const float r = r32[(size_t)blk * 64 + lane];
        f32x2 a01[kTileQ], a23[kTileQ];
#pragma unroll
        for (int t = 0; t < kTileQ; ++t) a01[t] = a23[t] = f32x2{0.f, 0.f};
        for (int g = 0; g < G; ++g, ++li) {
            const f32x4 xn = rv[(size_t)(li < last ? li + 1 : last) * 64 + lane];   // flies while this group is used
            const f32x4* qg = qp + (size_t)g * qpad;
#pragma unroll
            for (int t = 0; t < kTileQ; ++t) {
                const f32x4 y = qg[t];
                const f32x2 s01 = x.xy + y.xy, s23 = x.zw + y.zw;
                const f32x2 l01 = {__builtin_amdgcn_logf(s01.x), __builtin_amdgcn_logf(s01.y)};
                const f32x2 l23 = {__builtin_amdgcn_logf(s23.x), __builtin_amdgcn_logf(s23.y)};
                a01[t] = __builtin_elementwise_fma(s01, l01, a01[t]);
                a23[t] = __builtin_elementwise_fma(s23, l23, a23[t]);
            }
            x = xn;
        }
        const int row = blk * 64 + lane;
        const uint32_t in_split = (uint32_t)((blk - blk0) * 64 + lane);
#pragma unroll
        for (int t = 0; t < kTileQ; ++t) {
            const float key = fmaf(nhl2, ((a01[t].x + a01[t].y) + a23[t].x) + a23[t].y, r);
            // (rows of the padding carry R32 = +inf and are never below a threshold; the row bound is checked all the same)
            const bool offer = row < n && key < lane_f(thr_l, t);
            const u64 mask = __builtin_amdgcn_ballot_w64(offer);
            if (mask != 0) {
                const int c = lane_i(cnt_l, t);
                const int at = c + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                if (offer) keys[t * kBuf + at] = ((u64)f32_ord(key) << 32) | in_split;
                cnt_l = lane == t ? c + __builtin_popcountll(mask) : cnt_l;
            }
        }
        // a buffer holds at most kBuf - 64 keys before a block and takes at most 64 from it
        for (u64 big = __builtin_amdgcn_ballot_w64(cnt_l > kBuf - djs::kRowBlock); big != 0; big &= big - 1) {
            const int t = __builtin_amdgcn_readfirstlane(__builtin_ctzll(big));
            __builtin_amdgcn_wave_barrier();
            const float th = js_compact(keys + t * kBuf, lane_i(cnt_l, t), lane);
            if (lane == t) {
                cnt_l = kKeep;
                thr_l = th;
            }
        }
    }

    // the lists: sorted, then out with the rows' positions (a split past the last block has empty lists)
    for (int t = 0; t < kTileQ; ++t) {
        const int c = lane_i(cnt_l, t), kept = c < kKeep ? c : kKeep;
        __builtin_amdgcn_wave_barrier();
        if (c > 0) js_compact(keys + t * kBuf, c, lane);
        const size_t o = (size_t)(q0 + t) * nsplit + split;
        if (lane < kept) cand[o * kKeep + lane] = keys[t * kBuf + lane] + (u64)((uint32_t)blk0 * 64u);
        if (lane == 0) cand_cnt[o] = kept;
    }
}

}  // namespace

bool diverg_js_space(int space) {
    return space == SP_JSDIV || space == SP_JSDIV_SLOW || space == SP_JSMETR || space == SP_JSMETR_SLOW;
}

hipError_t launch_diverg_js_fast(int space, const dvf::Plan& p, int nq, int k, const DivergRows& rows, const float* r32,
                                 const djs::RowMax& m, const DivergQueries& q, const DivergFastWs& ws, const int32_t* ext_ids,
                                 float* out_d, int32_t* out_ids, int32_t* out_cnt, hipStream_t s) {
    if (!diverg_js_space(space) || !p.use || nq <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(diverg_js_prep_kernel, dim3((p.qpad + 63) / 64), dim3(64), 0, s, reinterpret_cast<const f32x4*>(q.vals),
                       q.stride, nq, p.qpad, rows.D, rows.G, m, reinterpret_cast<f32x4*>(ws.qclamp), ws.ce, ws.flags);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = launch_with_lds(diverg_js_filter_kernel, dim3((unsigned)(p.nsplit / 4 * p.nqt)), diverg_js_scan_lds(), s,
                        reinterpret_cast<const f32x4*>(rows.vals), r32, reinterpret_cast<const f32x4*>(ws.qclamp), rows.n, rows.G,
                        p.nblocks, p.rows_per_split / djs::kRowBlock, p.qpad, p.nsplit, ws.cand, ws.cand_cnt);
    if (e != hipSuccess) return e;
    return launch_diverg_fast_rerank_verify(space, p, nq, k, rows, q, ws, ext_ids, out_d, out_ids, out_cnt, s);
}

}  // namespace gfxknn
