// Exact k-NN and range search over sparse vectors (the SpaceSparseVectorSimpleStorage spaces).
//
// The reference's sparse distance (ComputeDistanceHelper, include/space/space_sparse_vector.h:137-215) merges the
// two sorted id lists into union order, writes 0 for an id missing on one side, and calls the DENSE function on the
// two union arrays.  So a pair is evaluated here by one thread that walks both lists in union order and feeds every
// union position into accumulators laid out like the dense SSE function: lane = union position mod 4, products and
// sums as separate roundings (the intrinsics are never contracted), the four lanes summed left to right, then the
// scalar tail -- the last (union length mod 4) positions -- which the reference's build (clang, -ffp-contract=on,
// x86-64-v3) evaluates with fused multiply-adds.  The union length is not known before the merge ends, so the
// current group of four positions is held back in registers: a complete group goes into the lanes, the group that is
// left incomplete at the end is the tail.  Everything is named registers: no array is indexed by the run-time union
// position (that would spill to scratch).  This file is compiled with -ffp-contract=off; the tail's FMAs are explicit.
//
// Storage: rows are CSR in HBM (row_ptr int64 [n+1], ids uint32 [nnz], vals f32 [nnz]); a batch of queries is CSR too.
//   sparse_knn_kernel  : grid (splits, query tiles).  One workgroup scans one row range for a tile of TQ queries
//                        (8 when k is small, else 1): a row is read once and merged against every query of the tile;
//                        the tile's queries are staged in LDS when they fit (kSparseQCap elements together), otherwise
//                        read from HBM (the long-list path: same code, slower, exact); the best kl keys
//                        (distance, position) of the range are kept in LDS (SplitTopK, split_topk_dev.hpp).  The per-split lists are merged by
//                        launch_merge_topk_ex (bf_kernels.hip), which also maps positions to external ids.
//   sparse_dist_kernel : both argument orders of the distance for every row (range search: the filter uses
//                        d(row, query), the reported distance is d(query, row), rangequery.cc:78-82 and
//                        nmslib_c.cpp:1104-1113); the selection is range_kernels.hip's.
//   sparse_pair_kernel : nmslib_get_distance.
#include "kernels.hpp"
#include "split_topk_dev.hpp"

namespace gfxknn {

namespace {

constexpr float kEps = 1.17549435e-38f * 2.0f;  // numeric_limits<float>::min() * 2

// Accumulators of one pair in union order.  x = value of obj1, y = value of obj2 (0 where the id is missing).
template <int SP>
struct UnionAcc {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;  // L2: (x-y)^2, L1: |x-y|, dot: x*y, cosine: x*y
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;  // cosine: x*x  (query-norm: sequential x*x)
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;  // cosine: y*y  (query-norm: sequential y*y)
    float px0 = 0.f, px1 = 0.f, px2 = 0.f, py0 = 0.f, py1 = 0.f, py2 = 0.f;  // held-back group
    float m = 0.f;   // Linf: running max (order-independent)
    float qs = 0.f;  // query-norm: sequential sum of x*y
    int c = 0;       // positions in the held-back group

    __device__ __forceinline__ static void lane(float x, float y, float& a, float& b, float& cc) {
        if constexpr (SP == SP_L2) {
            const float d = x - y;
            a = a + d * d;
        } else if constexpr (SP == SP_L1) {
            a = a + fabsf(x - y);
        } else if constexpr (SP == SP_NEGDOT) {
            a = a + x * y;
        } else {  // cosine / angular
            a = a + x * y;
            b = b + x * x;
            cc = cc + y * y;
        }
    }

    __device__ __forceinline__ void push(float x, float y) {
        if constexpr (SP == SP_LINF) {
            const float d = fabsf(x - y);
            m = m > d ? m : d;
        } else if constexpr (SP == SP_QNORM_NEGDOT) {
            // QueryNormScalarProduct (src/distcomp_scalar.cc:64-79): one sequential loop, contracted
            b0 = fmaf(x, x, b0);
            c0 = fmaf(y, y, c0);
            qs = fmaf(x, y, qs);
        } else {
            if (c == 3) {
                lane(px0, py0, a0, b0, c0);
                lane(px1, py1, a1, b1, c1);
                lane(px2, py2, a2, b2, c2);
                lane(x, y, a3, b3, c3);
            } else {
                px0 = c == 0 ? x : px0;
                py0 = c == 0 ? y : py0;
                px1 = c == 1 ? x : px1;
                py1 = c == 1 ? y : py1;
                px2 = c == 2 ? x : px2;
                py2 = c == 2 ? y : py2;
            }
            c = (c + 1) & 3;
        }
    }

    // fwd = distance(obj1, obj2), rev = distance(obj2, obj1)
    __device__ __forceinline__ void finish(float& fwd, float& rev) const {
        if constexpr (SP == SP_LINF) {
            fwd = rev = m;
        } else if constexpr (SP == SP_QNORM_NEGDOT) {
            // -QueryNormScalarProduct(p1, p2): normalised by the norm of the SECOND argument
            fwd = -(qs / sqrtf(fmaxf(c0, kEps)));
            rev = -(qs / sqrtf(fmaxf(b0, kEps)));
        } else if constexpr (SP == SP_L1) {
            double r = (double)(((a0 + a1) + a2) + a3);  // distcomp_lp.cc:190-251: float lanes, double tail
            if (c > 0) r += (double)fabsf(px0 - py0);
            if (c > 1) r += (double)fabsf(px1 - py1);
            if (c > 2) r += (double)fabsf(px2 - py2);
            fwd = rev = (float)r;
        } else if constexpr (SP == SP_L2) {
            float r = ((a0 + a1) + a2) + a3;  // distcomp_lp.cc:304-371
            float d;
            if (c > 0) { d = px0 - py0; r = fmaf(d, d, r); }
            if (c > 1) { d = px1 - py1; r = fmaf(d, d, r); }
            if (c > 2) { d = px2 - py2; r = fmaf(d, d, r); }
            fwd = rev = sqrtf(r);
        } else if constexpr (SP == SP_NEGDOT) {
            float r = ((a0 + a1) + a2) + a3;  // distcomp_scalar.cc:193-245
            if (c > 0) r = fmaf(px0, py0, r);
            if (c > 1) r = fmaf(px1, py1, r);
            if (c > 2) r = fmaf(px2, py2, r);
            fwd = rev = -r;
        } else {  // NormScalarProductSIMD, distcomp_scalar.cc:83-168
            float s = ((a0 + a1) + a2) + a3;
            float n1 = ((b0 + b1) + b2) + b3;
            float n2 = ((c0 + c1) + c2) + c3;
            if (c > 0) { s = fmaf(px0, py0, s); n1 = fmaf(px0, px0, n1); n2 = fmaf(py0, py0, n2); }
            if (c > 1) { s = fmaf(px1, py1, s); n1 = fmaf(px1, px1, n1); n2 = fmaf(py1, py1, n2); }
            if (c > 2) { s = fmaf(px2, py2, s); n1 = fmaf(px2, px2, n1); n2 = fmaf(py2, py2, n2); }
            float vf = 0.f, vr = 0.f;
            if (!(n1 < kEps || n2 < kEps)) {
                vf = s / sqrtf(n1) / sqrtf(n2);
                vr = s / sqrtf(n2) / sqrtf(n1);
                vf = fmaxf(-1.0f, fminf(1.0f, vf));
                vr = fmaxf(-1.0f, fminf(1.0f, vr));
            }
            if constexpr (SP == SP_ANGULAR) {  // AngularDistance, distcomp_scalar.cc:254-258
                fwd = acosf(vf);
                rev = acosf(vr);
            } else {  // CosineSimilarity, distcomp_scalar.cc:267-271
                fwd = fmaxf(0.0f, 1.0f - vf);
                rev = fmaxf(0.0f, 1.0f - vr);
            }
        }
    }
};

// One pair, obj1 = (ia, va, na), obj2 = (ib, vb, nb), merged in union order (space_sparse_vector.h:170-200).
template <int SP>
__device__ __forceinline__ void sparse_pair(const uint32_t* ia, const float* va, int na, const uint32_t* ib,
                                            const float* vb, int nb, float& fwd, float& rev) {
    UnionAcc<SP> acc;
    int i = 0, j = 0;
    while (i < na && j < nb) {
        const uint32_t a = ia[i], b = ib[j];
        const float xa = va[i], yb = vb[j];
        const bool ta = a <= b, tb = b <= a;
        acc.push(ta ? xa : 0.f, tb ? yb : 0.f);
        i += ta;
        j += tb;
    }
    for (; i < na; ++i) acc.push(va[i], 0.f);
    for (; j < nb; ++j) acc.push(0.f, vb[j]);
    acc.finish(fwd, rev);
}

// TQ queries per workgroup: a row is read from memory once per tile and merged against each query of the tile (the
// tile's queries sit in LDS when their elements fit kSparseQCap together; otherwise they are read from HBM).
template <int SP, int TQ>
__global__ __launch_bounds__(256) void sparse_knn_kernel(const int64_t* __restrict__ row_ptr,
                                                         const uint32_t* __restrict__ ids,
                                                         const float* __restrict__ vals, int n, int rows_per_split,
                                                         const int64_t* __restrict__ q_ptr,
                                                         const uint32_t* __restrict__ q_ids,
                                                         const float* __restrict__ q_vals, int nq, int k, int kl, int P,
                                                         float* __restrict__ out_d, int32_t* __restrict__ out_pos) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_cnt[TQ];
    const int tid = threadIdx.x, split = blockIdx.x, q_first = blockIdx.y * TQ;
    const int tile_n = min(TQ, nq - q_first);
    SplitTopK<TQ> sel{reinterpret_cast<u64*>(smem), s_cnt, P, kl, tile_n};
    uint32_t* sq_ids = reinterpret_cast<uint32_t*>(sel.keys + (size_t)TQ * P);  // [kSparseQCap]
    float* sq_vals = reinterpret_cast<float*>(sq_ids + kSparseQCap);
    const int64_t t0 = q_ptr[q_first], t1 = q_ptr[q_first + tile_n];
    const bool staged = t1 - t0 <= kSparseQCap;
    if (staged)
        for (int i = tid; i < (int)(t1 - t0); i += 256) {
            sq_ids[i] = q_ids[t0 + i];
            sq_vals[i] = q_vals[t0 + i];
        }
    const uint32_t* qi[TQ];
    const float* qv[TQ];
    int qn[TQ];
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
        const int64_t b = t < tile_n ? q_ptr[q_first + t] : t1;
        qn[t] = t < tile_n ? (int)(q_ptr[q_first + t + 1] - b) : 0;
        qi[t] = staged ? sq_ids + (b - t0) : q_ids + b;
        qv[t] = staged ? sq_vals + (b - t0) : q_vals + b;
    }
    sel.init(tid);
    __syncthreads();
    const int r0 = (int)min((long long)split * rows_per_split, (long long)n);
    const int r1 = min(n, r0 + rows_per_split);
    for (int base = r0; base < r1; base += 256) {
        const int r = base + tid;
        if (r < r1) {
            const int64_t p0 = row_ptr[r];
            const int rn = (int)(row_ptr[r + 1] - p0);
#pragma unroll
            for (int t = 0; t < TQ; ++t) {
                if (t < tile_n) {
                    float d, unused;
                    // the scan calls IndexTimeDistance(row, query) (DistanceObjLeft, src/query.cc:60-62)
                    sparse_pair<SP>(ids + p0, vals + p0, rn, qi[t], qv[t], qn[t], d, unused);
                    // -0 and +0 are one distance (the reference's queue compares them equal): one key for both
                    sel.offer(t, f32_ord(d == 0.0f ? 0.0f : d), r);
                }
            }
        }
        sel.chunk_done(tid, base + 256 >= r1);
    }
    sel.write(tid, split, nq, q_first, k, out_d, out_pos, [](uint32_t hi) { return ord_f32(hi); });
}

template <int SP>
__global__ __launch_bounds__(256) void sparse_dist_kernel(const int64_t* __restrict__ row_ptr,
                                                          const uint32_t* __restrict__ ids,
                                                          const float* __restrict__ vals, int n,
                                                          const uint32_t* __restrict__ q_ids,
                                                          const float* __restrict__ q_vals, int qn,
                                                          float* __restrict__ d_row_q, float* __restrict__ d_q_row) {
    __shared__ uint32_t sq_ids[kSparseQCap / 2];
    __shared__ float sq_vals[kSparseQCap / 2];
    const uint32_t* qi = q_ids;
    const float* qv = q_vals;
    if (qn <= kSparseQCap / 2) {
        for (int i = threadIdx.x; i < qn; i += 256) {
            sq_ids[i] = q_ids[i];
            sq_vals[i] = q_vals[i];
        }
        __syncthreads();
        qi = sq_ids;
        qv = sq_vals;
    }
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256) {
        const int64_t p0 = row_ptr[r];
        float f, b;
        sparse_pair<SP>(ids + p0, vals + p0, (int)(row_ptr[r + 1] - p0), qi, qv, qn, f, b);
        d_row_q[r] = f;
        d_q_row[r] = b;
    }
}

template <int SP>
__global__ void sparse_pair_kernel(const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ ids,
                                   const float* __restrict__ vals, int p1, int p2, float* out) {
    if (threadIdx.x != 0) return;
    const int64_t a = row_ptr[p1], b = row_ptr[p2];
    float f, r;
    sparse_pair<SP>(ids + a, vals + a, (int)(row_ptr[p1 + 1] - a), ids + b, vals + b, (int)(row_ptr[p2 + 1] - b), f, r);
    *out = f;
}

template <template <int> class Launch, typename... Args>
hipError_t dispatch_space(int space, Args... args) {
    switch (space) {
        case SP_L2: return Launch<SP_L2>::run(args...);
        case SP_L1: return Launch<SP_L1>::run(args...);
        case SP_LINF: return Launch<SP_LINF>::run(args...);
        case SP_COSINE: return Launch<SP_COSINE>::run(args...);
        case SP_ANGULAR: return Launch<SP_ANGULAR>::run(args...);
        case SP_NEGDOT: return Launch<SP_NEGDOT>::run(args...);
        case SP_QNORM_NEGDOT: return Launch<SP_QNORM_NEGDOT>::run(args...);
        default: return hipErrorInvalidValue;
    }
}

template <int SP>
struct KnnLaunch {
    static hipError_t run(const ScanPlan& p, const int64_t* row_ptr, const uint32_t* ids, const float* vals,
                          const int64_t* q_ptr, const uint32_t* q_ids, const float* q_vals, float* out_d,
                          int32_t* out_pos, hipStream_t s) {
        const dim3 grid(p.nsplit, (p.nq + p.tq - 1) / p.tq);
        const size_t lds = (size_t)p.tq * p.P * 8 + (size_t)kSparseQCap * 8;
        if (p.tq == kSparseTileQ)
            return launch_with_lds(sparse_knn_kernel<SP, kSparseTileQ>, grid, lds, s, row_ptr, ids, vals, p.n,
                                   p.rows_per_split, q_ptr, q_ids, q_vals, p.nq, p.k, p.kl, p.P, out_d, out_pos);
        return launch_with_lds(sparse_knn_kernel<SP, 1>, grid, lds, s, row_ptr, ids, vals, p.n, p.rows_per_split, q_ptr,
                               q_ids, q_vals, p.nq, p.k, p.kl, p.P, out_d, out_pos);
    }
};

template <int SP>
struct DistLaunch {
    static hipError_t run(const int64_t* row_ptr, const uint32_t* ids, const float* vals, int n, const uint32_t* q_ids,
                          const float* q_vals, int qn, float* d_row_q, float* d_q_row, hipStream_t s) {
        int grid = (n + 255) / 256;
        if (grid > 8192) grid = 8192;
        if (grid < 1) grid = 1;
        hipLaunchKernelGGL(sparse_dist_kernel<SP>, dim3(grid), dim3(256), 0, s, row_ptr, ids, vals, n, q_ids, q_vals, qn,
                           d_row_q, d_q_row);
        return hipGetLastError();
    }
};

template <int SP>
struct PairLaunch {
    static hipError_t run(const int64_t* row_ptr, const uint32_t* ids, const float* vals, int p1, int p2, float* out,
                          hipStream_t s) {
        hipLaunchKernelGGL(sparse_pair_kernel<SP>, dim3(1), dim3(64), 0, s, row_ptr, ids, vals, p1, p2, out);
        return hipGetLastError();
    }
};

}  // namespace

hipError_t launch_sparse_knn(int space, const ScanPlan& p, const int64_t* row_ptr, const uint32_t* ids,
                             const float* vals, const int64_t* q_ptr, const uint32_t* q_ids, const float* q_vals,
                             float* split_d, int32_t* split_pos, hipStream_t s) {
    return dispatch_space<KnnLaunch>(space, p, row_ptr, ids, vals, q_ptr, q_ids, q_vals, split_d, split_pos, s);
}

hipError_t launch_sparse_dist(int space, const int64_t* row_ptr, const uint32_t* ids, const float* vals, int n,
                              const uint32_t* q_ids, const float* q_vals, int qn, float* d_row_q, float* d_q_row,
                              hipStream_t s) {
    if (n <= 0) return hipSuccess;
    return dispatch_space<DistLaunch>(space, row_ptr, ids, vals, n, q_ids, q_vals, qn, d_row_q, d_q_row, s);
}

hipError_t launch_sparse_pair(int space, const int64_t* row_ptr, const uint32_t* ids, const float* vals, int p1, int p2,
                              float* out, hipStream_t s) {
    return dispatch_space<PairLaunch>(space, row_ptr, ids, vals, p1, p2, out, s);
}

}  // namespace gfxknn
