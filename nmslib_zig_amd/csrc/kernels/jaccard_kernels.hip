// Exact k-NN, range and pair distances over bit_jaccard (data type 3, float distance): 1 - |a & b| / |a | b| over the packed
// words of the bit_hamming store (string_kernels.hip).
//   jac_knn_kernel<TQ>: ham_knn_kernel's shape.  Grid (splits, query tiles); each lane streams one row (16-byte loads when
//                       W % 4 == 0) against the tile's queries, staged in LDS.  Per word one popcount of x & q per query and
//                       one of x for the row; |q| is counted once per query when the tile is staged; |a | b| is
//                       |q| + |b| - |a & b|, and one division per (row, query) follows the row.
//   jac_dist_kernel, jac_pair_kernel: one distance per row / one pair, by the same jac_distance (jaccard_dev.hpp).
//   Selection: SplitTopK with the f32 bits of the distance as the upper half of the key.
#include <algorithm>

#include "jaccard_dev.hpp"
#include "split_topk_dev.hpp"

namespace gfxknn {

namespace {

// (|a & b|, |a | b|) of two codes of W words
__device__ __forceinline__ float jac_words(const uint32_t* a, const uint32_t* b, int W) {
    int num = 0, den = 0;
    for (int w = 0; w < W; ++w) {
        num += __popc(a[w] & b[w]);
        den += __popc(a[w] | b[w]);
    }
    return jac_distance(num, den);
}

template <int TQ>
__global__ __launch_bounds__(256) void jac_knn_kernel(const uint32_t* __restrict__ rows, int W, int n,
                                                      int rows_per_split, const uint32_t* __restrict__ q, int nq,
                                                      int k, int kl, int P, float* __restrict__ out_d,
                                                      int32_t* __restrict__ out_pos) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_cnt[TQ];
    __shared__ int s_pq[TQ];
    const int tid = threadIdx.x, split = blockIdx.x, q_first = blockIdx.y * TQ;
    const int tile_n = min(TQ, nq - q_first);
    SplitTopK<TQ> sel{reinterpret_cast<u64*>(smem), s_cnt, P, kl, tile_n};
    uint32_t* s_q = reinterpret_cast<uint32_t*>(reinterpret_cast<u64*>(smem) + (size_t)TQ * P);
    const bool q_staged = (size_t)TQ * W * 4 <= kStrHamQStage;
    // the queries of a partial tile repeat its first one (their results are not written)
    if (q_staged)
        for (int i = tid; i < TQ * W; i += 256) {
            const int t = i / W;
            s_q[i] = q[(size_t)(q_first + (t < tile_n ? t : 0)) * W + (i - t * W)];
        }
    if (tid < TQ) {  // |q|, once per query of the tile
        const uint32_t* qt = q + (size_t)(q_first + (tid < tile_n ? tid : 0)) * W;
        int s = 0;
        for (int w = 0; w < W; ++w) s += __popc(qt[w]);
        s_pq[tid] = s;
    }
    const uint32_t* qb = q_staged ? s_q : q + (size_t)q_first * W;
    sel.init(tid);
    __syncthreads();
    int pq[TQ];
#pragma unroll
    for (int t = 0; t < TQ; ++t) pq[t] = s_pq[t];
    const int r0 = (int)min((long long)split * rows_per_split, (long long)n);
    const int r1 = min(n, r0 + rows_per_split);
    for (int base = r0; base < r1; base += 256) {
        const int r = base + tid;
        if (r < r1) {
            const uint32_t* row = rows + (size_t)r * W;
            int acc[TQ], pb = 0;
#pragma unroll
            for (int t = 0; t < TQ; ++t) acc[t] = 0;
            int w = 0;
            if ((W & 3) == 0) {
                for (; w < W; w += 4) {
                    const uint4 x = *reinterpret_cast<const uint4*>(row + w);
                    pb += __popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w);
#pragma unroll
                    for (int t = 0; t < TQ; ++t) {
                        const uint32_t* qt = qb + (size_t)(t < tile_n ? t : 0) * W + w;
                        acc[t] += __popc(x.x & qt[0]) + __popc(x.y & qt[1]) + __popc(x.z & qt[2]) + __popc(x.w & qt[3]);
                    }
                }
            }
            for (; w < W; ++w) {
                const uint32_t x = row[w];
                pb += __popc(x);
#pragma unroll
                for (int t = 0; t < TQ; ++t) acc[t] += __popc(x & qb[(size_t)(t < tile_n ? t : 0) * W + w]);
            }
#pragma unroll
            for (int t = 0; t < TQ; ++t)
                if (t < tile_n) sel.offer(t, __float_as_uint(jac_distance(acc[t], pq[t] + pb - acc[t])), r);
        }
        sel.chunk_done(tid, base + 256 >= r1);
    }
    sel.write(tid, split, nq, q_first, k, out_d, out_pos, JacKeyToDist{});
}

__global__ __launch_bounds__(256) void jac_dist_kernel(const uint32_t* __restrict__ rows, int W, int n,
                                                       const uint32_t* __restrict__ q, float* __restrict__ d_out) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256)
        d_out[r] = jac_words(rows + (size_t)r * W, q, W);
}

__global__ void jac_pair_kernel(const uint32_t* __restrict__ rows, int W, int p1, int p2, float* out) {
    if (threadIdx.x != 0) return;
    *out = jac_words(rows + (size_t)p1 * W, rows + (size_t)p2 * W, W);
}

}  // namespace

hipError_t launch_jac_knn(const ScanPlan& p, const uint32_t* rows, int W, const uint32_t* q, float* split_d,
                          int32_t* split_pos, hipStream_t s) {
    const dim3 grid(p.nsplit, (p.nq + p.tq - 1) / p.tq);
    const size_t lds = (size_t)p.tq * p.P * 8 + kStrHamQStage;
    if (p.tq == kStrTileQ)
        return launch_with_lds(jac_knn_kernel<kStrTileQ>, grid, lds, s, rows, W, p.n, p.rows_per_split, q, p.nq, p.k,
                               p.kl, p.P, split_d, split_pos);
    return launch_with_lds(jac_knn_kernel<1>, grid, lds, s, rows, W, p.n, p.rows_per_split, q, p.nq, p.k, p.kl, p.P,
                           split_d, split_pos);
}

hipError_t launch_jac_dist(const uint32_t* rows, int W, int n, const uint32_t* q, float* d_out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    int grid = std::max(1, std::min((n + 255) / 256, 8192));
    hipLaunchKernelGGL(jac_dist_kernel, dim3(grid), dim3(256), 0, s, rows, W, n, q, d_out);
    return hipGetLastError();
}

hipError_t launch_jac_pair(const uint32_t* rows, int W, int p1, int p2, float* out, hipStream_t s) {
    hipLaunchKernelGGL(jac_pair_kernel, dim3(1), dim3(64), 0, s, rows, W, p1, p2, out);
    return hipGetLastError();
}

}  // namespace gfxknn
