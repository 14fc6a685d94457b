// Exact bit_hamming k-NN on the int8 matrix cores (the plan: ham_fast_plan.hpp).
//
// For a row b with bits in {0, 1} and a query q:  ham(q, b) = |q| + sum_c b_c * s_c,  s_c = 1 - 2 q_c, |q| = popcount(q).
// With b as int8 0 / 1 and s as int8 +1 / -1, v_mfma_i32_32x32x32_i8 accumulates the sum exactly in i32 and, started from
// |q|, leaves the distance itself in the accumulator: no filter, no bound, no re-rank.
//
//   Operands.  One K-step is one packed word of every row.  Lane (l31, h) of the wave holds the 16 bytes made of bits
//   d + 4 h + 8 j (d = dword 0..3, j = byte 0..3) of the word of row / query l31: (x >> (d + 4 h)) & 0x01010101.  Rows and
//   queries use the same order, which is all a dot product asks.  A query's byte is then (b << 8) - b | 0x01010101 per
//   dword: 0xFF where the bit is set, 0x01 where it is clear.  Words above `bits` are zero on both sides (a zero row bit
//   adds nothing) and |q| counts real bits only.
//   Work.  Grid (row splits, query tiles), ONE wave per workgroup: nothing is shared between waves, so a barrier never waits
//   for another wave.  A wave holds 4 row groups x QB = 2 query groups of 32 x 32 accumulators (128 registers,
//   so two waves share a SIMD and one expands operands while the other's MFMAs run; 4 x 4 left no registers for the
//   operands and spilled) and walks its split in blocks of 128 rows; per K-step it expands 4 row and QB query operands
//   and issues 4 QB MFMAs.  The tile's packed query words sit in LDS, word-major ([W][tile]: lanes read neighbouring
//   banks); row words come from global memory, 16 bytes per load where W % 4 == 0.
//   Selection.  Queries are the column operand: a lane's 16 values of an accumulator belong to query l31 and to rows
//   8 j + 4 h + i, so a query's threshold is one register.  Keys are (distance << 16) | row within the split; a value is
//   appended to its query's list in LDS ([cap][64], a counter per list: the query's two lanes append side by side) when
//   its key is below the threshold, out of line, behind one min over the 16 values.  Before a list could overflow with 32
//   more keys every list is cut to its k smallest, lane t sorting list t (the same network for all lanes), and the k-th
//   key becomes the threshold.  Order of arrival plays no part: the k smallest (distance, position) keys are kept, which
//   is the reference's rule (a later row enters only below the k-th distance).
//   Thresholds.  A list that starts empty takes about k ln(rows / k) keys before its threshold is tight, and every split
//   of every query pays that again.  So the first kSampleRows rows are scanned first (the same kernel, `sample`), their
//   lists merged, and the k-th distance of each query there bounds the scan of all rows from its first block on: a list
//   then takes about rows * k / kSampleRows keys and is rarely cut before the end.
//   Output.  The per-split format of the other scans: split_d / split_pos [nsplit][nq][k], ascending, padded with
//   (+inf, -1); launch_merge_topk_ex merges the splits.
#include "bit_list_dev.hpp"

namespace gfxknn {

namespace {

constexpr uint32_t kOnes = 0x01010101u;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

// the 16 operand bytes of a lane from one packed word (xs = word >> 4 h)
__device__ __forceinline__ i32x4 ham_row_operand(uint32_t xs) {
    i32x4 v;
    v[0] = (int)(xs & kOnes);
    v[1] = (int)((xs >> 1) & kOnes);
    v[2] = (int)((xs >> 2) & kOnes);
    v[3] = (int)((xs >> 3) & kOnes);
    return v;
}
__device__ __forceinline__ i32x4 ham_query_operand(uint32_t xs) {
    i32x4 v = ham_row_operand(xs);
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const uint32_t b = (uint32_t)v[d];
        v[d] = (int)(((b << 8) - b) | kOnes);
    }
    return v;
}

template <bool VEC>
__global__ __launch_bounds__(64) void ham_mfma_knn_kernel(const uint32_t* __restrict__ rows, int W, int n,
                                                          int rows_per_split, const uint32_t* __restrict__ q, int nq,
                                                          int k, int cap, const float* __restrict__ bound,
                                                          float* __restrict__ out_d, int32_t* __restrict__ out_pos) {
    constexpr int QB = hamfast::kQueryGroups;
    constexpr int QT = 32 * QB;   // queries of the tile = lists = lanes
    static_assert(QT == 64, "a cut gives every lane one list");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t* s_q = reinterpret_cast<uint32_t*>(smem);   // [W][QT]
    uint32_t* s_keys = s_q + (size_t)W * QT;             // [cap][QT]
    int* s_cnt = reinterpret_cast<int*>(s_keys + (size_t)cap * QT);   // [QT]
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
    uint32_t thr[QB];
#pragma unroll
    for (int g = 0; g < QB; ++g) {
        int s = 0;
        for (int w = 0; w < W; ++w) s += __popc(s_q[w * QT + g * 32 + l31]);
        pq[g] = s;
        // bound: the k best distances of the query over a sample of the rows.  k rows lie within the k-th of them, so no
        // row beyond it is among the k nearest; rows AT it still pass (position decides among equal distances)
        thr[g] = bound ? ((uint32_t)bound[(size_t)min(q_first + g * 32 + l31, nq - 1) * k + (k - 1)] + 1u) << 16 : kNoKey;
    }

    // every list cut to its k smallest keys (bit_list_dev.hpp); a full list's k-th key is its query's new threshold
    auto cut = [&]() __attribute__((always_inline)) {
        bit_list_cut<uint32_t, QT>(s_keys, s_cnt, lane, cap, k, kNoKey);
#pragma unroll
        for (int g = 0; g < QB; ++g)
            if (s_cnt[g * 32 + l31] >= k) thr[g] = s_keys[(size_t)(k - 1) * QT + g * 32 + l31];
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
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
#pragma unroll
            for (int g = 0; g < QB; ++g)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[rb][g][i] = pq[g];

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
                    for (int rb = 0; rb < 4; ++rb) a[rb] = ham_row_operand(cur[rb][j] >> sh);
#pragma unroll
                    for (int g = 0; g < QB; ++g) b[g] = ham_query_operand(s_q[(w0 + j) * QT + g * 32 + l31] >> sh);
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

        // accumulator register 4 j + i of half h = row 8 j + 4 h + i of its 32-row group, query l31 of its group
#pragma unroll
        for (int g = 0; g < QB; ++g) {
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) {
                const i32x16& c = acc[rb][g];
                int m = min(min(c[0], c[1]), c[2]);
#pragma unroll
                for (int i = 3; i + 1 < 16; i += 2) m = min(min(m, c[i]), c[i + 1]);
                m = min(m, c[15]);
                if (__builtin_expect(__any((uint32_t)m <= (thr[g] >> 16)), 0)) {
                    // the two lanes of a query append up to 32 keys: cap >= k + 32 always leaves room behind a cut
                    __syncthreads();
                    if (__any(s_cnt[g * 32 + l31] + 32 > cap)) cut();
                    const int rr0 = base + rb * 32 + 4 * h;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int rr = rr0 + 8 * (i >> 2) + (i & 3);
                        const uint32_t key = ((uint32_t)c[i] << 16) | (uint32_t)rr;
                        if (rr < lim && key < thr[g])
                            s_keys[(size_t)atomicAdd(&s_cnt[g * 32 + l31], 1) * QT + g * 32 + l31] = key;
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
            const uint32_t key = s_keys[(size_t)min(e, cap - 1) * QT + lane];
            out_pos[o + e] = e < c ? r0 + (int)(key & 0xFFFFu) : -1;
            out_d[o + e] = e < c ? (float)(key >> 16) : INFINITY;
        }
    }
}

template <bool VEC>
hipError_t launch_one(const hamfast::Plan& p, int nsplit, int rows_per_split, const uint32_t* rows, int n, const uint32_t* q,
                      int nq, int k, const float* bound, float* split_d, int32_t* split_pos, hipStream_t s) {
    auto kernel = ham_mfma_knn_kernel<VEC>;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)p.lds);
    if (e != hipSuccess) return e;
    const dim3 grid(nsplit, (nq + p.tile - 1) / p.tile);
    hipLaunchKernelGGL(kernel, grid, dim3(64), p.lds, s, rows, p.W, n, rows_per_split, q, nq, k, p.cap, bound, split_d,
                       split_pos);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ham_mfma_knn(const hamfast::Plan& p, bool sample, const uint32_t* rows, int n, const uint32_t* q, int nq,
                               int k, const float* bound, float* split_d, int32_t* split_pos, hipStream_t s) {
    if (!p.use || nq <= 0 || p.qb != hamfast::kQueryGroups) return hipErrorInvalidValue;
    const int nsplit = sample ? p.sample_nsplit : p.nsplit, rps = sample ? p.sample_rows / p.sample_nsplit : p.rows_per_split;
    if (sample) n = p.sample_rows;
    return (p.W & 3) == 0 ? launch_one<true>(p, nsplit, rps, rows, n, q, nq, k, bound, split_d, split_pos, s)
                          : launch_one<false>(p, nsplit, rps, rows, n, q, nq, k, bound, split_d, split_pos, s);
}

}  // namespace gfxknn
