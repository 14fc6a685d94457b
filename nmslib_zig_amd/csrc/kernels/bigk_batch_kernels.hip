// Exact k-NN for BF_MAX_K < k <= kBigkBatchMaxK in one batched scan: the rows are read once per slice
// of queries and no query sorts more than its own short list.
//   1. bigk_collect (sample): the arrangement of row_tile_dev.hpp -- a wave keeps 64 rows in registers, a tile of 32
//                       queries sits in LDS, lane i ends with row i's distance -- over every stride-th 64-row block with
//                       no radius: each query's list holds the keys (f32_ord(distance) << 32 | position) of the sample;
//   2. bigk_radius    : one workgroup per query sorts the sample keys in LDS; the rank-th smallest distance is the
//                       query's radius; the list is emptied;
//   3. bigk_collect   : the same kernel over all blocks: the lanes whose distance is <= the radius append their keys.  One
//                       atomic add per (wave, query) that has a match reserves popcount(ballot) slots, a lane's slot is
//                       its rank in the ballot.  A reservation that would pass the capacity stores nothing; the counter
//                       keeps counting, so count > capacity tells the overflow;
//   4. bigk_select    : one workgroup per query: count < k (the radius fell short) or count > capacity flags the query;
//                       otherwise the list is sorted in LDS and its first k keys are the answer -- the key carries the
//                       exact distance, nothing is computed again;
//   5. bigk_redo      : one workgroup per flagged query (the others leave at once): the exact k-th distance by a radix
//                       select over f32_ord(distance), four passes of 8 bits that compute the distances again with
//                       wave_exact_distance_*, then one pass that keeps the rows below it and, in ascending position, as
//                       many rows equal to it as k still needs.  Slow and rare; it makes the route exact on any data.
// Keys are distinct and their order (distance, position) is total, so the order of the appends never reaches the answer.
// Every distance is, bit for bit, what wave_exact_distance_f32 / _u8 returns (row_tile_dev.hpp's rule): a row of the
// answer is what launch_bf_bigk writes for that query.
#include "../bigk_batch_plan.hpp"
#include "kernels.hpp"
#include "row_tile_dev.hpp"

namespace gfxknn {

namespace {

constexpr int kTile = (int)kBigkBatchQueryTile;
constexpr int kSortThreads = 1024;
constexpr int kRedoWaves = kSortThreads / 64;
constexpr u64 kPadKey = ~0ull;

__global__ void bigk_clear_kernel(int* __restrict__ counts, int* __restrict__ flags, int nq) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    counts[q] = 0;
    flags[q] = 0;
}

// lane i holds row pos's distance to one query: the lanes inside the radius append their keys to the query's list
__device__ __forceinline__ void bigk_append(float d, size_t pos, int n, uint32_t radius, u64* __restrict__ list,
                                            int* __restrict__ count, int cap, int lane) {
    const uint32_t o = f32_ord(d);
    const bool hit = pos < (size_t)n && o <= radius;
    const u64 b = __ballot(hit);
    if (b == 0) return;
    const int m = __popcll(b);
    int base = 0;
    if (lane == 0) base = atomicAdd(count, m);
    base = __shfl(base, 0, 64);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    if (hit && base + m <= cap) list[base + rank] = ((u64)o << 32) | (u64)(uint32_t)pos;
}

// grid (groups of 4 sampled row blocks, query splits); radius == null: every row matches (the sample pass).  A wave takes
// block (4 blockIdx.x + wave) * stride.
template <int KIND, int C, bool TAIL>
__global__ __launch_bounds__(256) void bigk_collect_kernel(int space, const float* __restrict__ rows, int ld, int n,
                                                           const float* __restrict__ queries, int dim, int nq,
                                                           const uint32_t* __restrict__ radius, int stride,
                                                           u64* __restrict__ lists, int* __restrict__ counts, int cap) {
    __shared__ float qs[kTile * C * 64];
    __shared__ float qnorm[kTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t first = ((size_t)blockIdx.x * 4 + wave) * (size_t)stride * 64;
    const bool active = first < (size_t)n;   // (a wave past the rows only keeps the barriers)
    const bool last_ok = lane + 64 * (C - 1) < dim;

    float rv[64][C];
    float rnorm = 0.f;
    if (active) rnorm = rb_load_rows<KIND, C, TAIL>(rows, ld, n, first, dim, lane, last_ok, rv);

    const int ntiles = (nq + kTile - 1) / kTile;
    for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
        const int q0 = t * kTile;
        const int tq = nq - q0 < kTile ? nq - q0 : kTile;
        __syncthreads();   // the last tile has been read
        rb_stage_queries<KIND, C, TAIL, kTile>(queries, dim, q0, tq, last_ok, qs, qnorm);
        if (!active) continue;
        for (int qi = 0; qi < tq; ++qi) {
            const float d = rb_tile_distance<KIND, C, TAIL>(space, rv, qs + qi * C * 64, lane, last_ok, rnorm,
                                                            KIND == RB_COS ? qnorm[qi] : 0.f);
            const int q = q0 + qi;
            bigk_append(d, first + lane, n, radius ? radius[q] : 0xFFFFFFFFu, lists + (size_t)q * cap, counts + q, cap, lane);
        }
    }
}

__global__ __launch_bounds__(256) void bigk_collect_u8_kernel(const uint8_t* __restrict__ rows, int n,
                                                              const uint8_t* __restrict__ queries, int nq,
                                                              const uint32_t* __restrict__ radius, int stride,
                                                              u64* __restrict__ lists, int* __restrict__ counts, int cap) {
    __shared__ uint8_t qs[kTile * 128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t first = ((size_t)blockIdx.x * 4 + wave) * (size_t)stride * 64;
    const bool active = first < (size_t)n;
    rb_short2 rv[64];
    if (active) rb_load_rows_u8(rows, n, first, lane, rv);
    const int ntiles = (nq + kTile - 1) / kTile;
    for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
        const int q0 = t * kTile;
        const int tq = nq - q0 < kTile ? nq - q0 : kTile;
        __syncthreads();
        rb_stage_queries_u8<kTile>(queries, q0, tq, qs);
        if (!active) continue;
        for (int qi = 0; qi < tq; ++qi) {
            const float d = rb_tile_distance_u8(rv, qs + qi * 128, lane);
            const int q = q0 + qi;
            bigk_append(d, first + lane, n, radius ? radius[q] : 0xFFFFFFFFu, lists + (size_t)q * cap, counts + q, cap, lane);
        }
    }
}

// m keys of list into s, padded to the next power of two P (>= 1) with kPadKey, sorted ascending; -> P.  kSortThreads threads.
__device__ __forceinline__ int bigk_load_sorted(const u64* __restrict__ list, int m, u64* s) {
    const int P = next_pow2(m > 1 ? m : 1);
    for (int i = threadIdx.x; i < P; i += kSortThreads) s[i] = i < m ? list[i] : kPadKey;
    __syncthreads();
    block_bitonic_u64_asc(s, P, threadIdx.x, kSortThreads);
    return P;
}

// the first k keys of s (sorted) as query q's row of the answer
__device__ __forceinline__ void bigk_emit(const u64* s, int k, int q, const int32_t* __restrict__ ext_ids,
                                          int32_t* __restrict__ out_ids, float* __restrict__ out_dists,
                                          int32_t* __restrict__ out_cnt) {
    for (int i = threadIdx.x; i < k; i += kSortThreads) {
        const u64 key = s[i];
        const uint32_t pos = (uint32_t)key;
        out_ids[(size_t)q * k + i] = ext_ids ? ext_ids[pos] : (int32_t)pos;
        out_dists[(size_t)q * k + i] = ord_f32((uint32_t)(key >> 32));
    }
    if (threadIdx.x == 0 && out_cnt) out_cnt[q] = k;
}

// one workgroup per query; dynamic LDS: cap keys
__global__ __launch_bounds__(kSortThreads) void bigk_radius_kernel(const u64* __restrict__ lists, int* __restrict__ counts,
                                                                   uint32_t* __restrict__ radius, int cap, int rank) {
    extern __shared__ u64 bigk_keys[];
    const int q = blockIdx.x;
    const int c = counts[q];
    const int m = c < cap ? c : cap;
    bigk_load_sorted(lists + (size_t)q * cap, m, bigk_keys);
    if (threadIdx.x == 0) {
        // (fewer sample rows than the rank, which the plan's gates exclude: every row matches and the select decides)
        radius[q] = m >= rank ? (uint32_t)(bigk_keys[rank - 1] >> 32) : 0xFFFFFFFFu;
        counts[q] = 0;
    }
}

__global__ __launch_bounds__(kSortThreads) void bigk_select_kernel(const u64* __restrict__ lists, const int* __restrict__ counts,
                                                                   int* __restrict__ flags, int cap, int k,
                                                                   const int32_t* __restrict__ ext_ids,
                                                                   int32_t* __restrict__ out_ids, float* __restrict__ out_dists,
                                                                   int32_t* __restrict__ out_cnt) {
    extern __shared__ u64 bigk_keys[];
    const int q = blockIdx.x;
    const int c = counts[q];
    if (c < k || c > cap) {
        if (threadIdx.x == 0) flags[q] = 1;
        return;
    }
    bigk_load_sorted(lists + (size_t)q * cap, c, bigk_keys);
    bigk_emit(bigk_keys, k, q, ext_ids, out_ids, out_dists, out_cnt);
}

// f32_ord of the distances of rows r0 .. r0 + 3 (< end) to the query, all four rows' loads issued before the first use
template <bool U8>
__device__ __forceinline__ void bigk_redo_ords(int space, const void* __restrict__ rows, int ld, int dim,
                                               const void* __restrict__ query, int r0, int end, int lane, uint32_t (&o)[4]) {
    if (U8) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + i < end ? r0 + i : end - 1;
            o[i] = f32_ord((float)wave_exact_distance_u8(static_cast<const uint8_t*>(rows) + (size_t)r * 128,
                                                         static_cast<const uint8_t*>(query), lane));
        }
    } else {
        const float* a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = static_cast<const float*>(rows) + (size_t)(r0 + i < end ? r0 + i : end - 1) * ld;
        float d[4];
        wave_exact_distance_f32_x4(space, a, static_cast<const float*>(query), dim, lane, d);
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = f32_ord(d[i]);
    }
}

// One workgroup of 16 waves per query; wave w owns the rows [w * per, (w + 1) * per), so that "ascending position" among
// equal distances is the waves' order, then each wave's own.  The histograms are one per wave (only lane 0 of the owner
// touches one: plain LDS adds).  n >= 2 k rows (the plan's gate), so a k-th distance exists.
template <bool U8>
__global__ __launch_bounds__(kSortThreads) void bigk_redo_kernel(int space, const void* __restrict__ rows, int ld, int n,
                                                                 int dim, const void* __restrict__ queries,
                                                                 const int* __restrict__ flags, int k,
                                                                 const int32_t* __restrict__ ext_ids,
                                                                 int32_t* __restrict__ out_ids, float* __restrict__ out_dists,
                                                                 int32_t* __restrict__ out_cnt) {
    const int q = blockIdx.x;
    if (!flags[q]) return;
    __shared__ u64 keys[kBigkBatchMaxK];
    __shared__ int hist[kRedoWaves][256];
    __shared__ int tot[256];
    __shared__ int eq_before[kRedoWaves];
    __shared__ uint32_t sh_prefix;
    __shared__ int sh_need, sh_digit, sh_kept;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const void* query = static_cast<const char*>(queries) + (size_t)q * (U8 ? 128 : (size_t)dim * 4);
    const int per = (n + kRedoWaves - 1) / kRedoWaves;
    const int begin = wave * per < n ? wave * per : n;
    const int end = begin + per < n ? begin + per : n;

    if (threadIdx.x == 0) {
        sh_prefix = 0;
        sh_need = k;
        sh_kept = 0;
    }
    for (int pass = 0; pass < 4; ++pass) {
        for (int i = threadIdx.x; i < kRedoWaves * 256; i += kSortThreads) (&hist[0][0])[i] = 0;
        __syncthreads();
        const int shift = 24 - 8 * pass;
        const uint32_t above = pass == 0 ? 0u : 0xFFFFFFFFu << (shift + 8);   // the digits already fixed
        const uint32_t prefix = sh_prefix;
        for (int r0 = begin; r0 < end; r0 += 4) {
            uint32_t o[4];
            bigk_redo_ords<U8>(space, rows, ld, dim, query, r0, end, lane, o);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (r0 + i < end && (o[i] & above) == prefix) hist[wave][(o[i] >> shift) & 255] += 1;
            }
        }
        __syncthreads();
        if (threadIdx.x < 256) {
            int t = 0;
            for (int w = 0; w < kRedoWaves; ++w) t += hist[w][threadIdx.x];
            tot[threadIdx.x] = t;
        }
        __syncthreads();
        if (threadIdx.x == 0) {   // the digit that holds the sh_need-th smallest of the rows under the prefix
            int acc = 0, b = 0;
            while (b < 255 && acc + tot[b] < sh_need) acc += tot[b++];
            sh_need -= acc;
            sh_digit = b;
            sh_prefix = prefix | ((uint32_t)b << shift);
        }
        __syncthreads();
    }
    // hist holds the last pass: a wave's rows equal to the k-th distance are its count of the last digit
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int w = 0; w < kRedoWaves; ++w) {
            eq_before[w] = acc;
            acc += hist[w][sh_digit];
        }
    }
    __syncthreads();
    const uint32_t kth = sh_prefix;
    const int need = sh_need;   // rows equal to kth that the answer takes: those of the lowest positions
    int eq = eq_before[wave];
    for (int r0 = begin; r0 < end; r0 += 4) {
        uint32_t o[4];
        bigk_redo_ords<U8>(space, rows, ld, dim, query, r0, end, lane, o);
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (r0 + i >= end) continue;
                bool take = o[i] < kth;
                if (o[i] == kth) take = eq++ < need;
                if (take) {
                    const int at = atomicAdd(&sh_kept, 1);
                    if (at < (int)kBigkBatchMaxK) keys[at] = ((u64)o[i] << 32) | (u64)(uint32_t)(r0 + i);
                }
            }
        }
    }
    __syncthreads();
    const int P = next_pow2(k);
    for (int i = sh_kept + threadIdx.x; i < P; i += kSortThreads) keys[i] = kPadKey;
    __syncthreads();
    block_bitonic_u64_asc(keys, P, threadIdx.x, kSortThreads);
    bigk_emit(keys, k, q, ext_ids, out_ids, out_dists, out_cnt);
}

template <int KIND, int C>
void bigk_launch_collect(bool tail, dim3 grid, hipStream_t s, const BigkBatchArgs& a, const uint32_t* radius, int stride) {
    const float* rows = static_cast<const float*>(a.rows);
    const float* q = static_cast<const float*>(a.queries);
    if (tail)
        hipLaunchKernelGGL((bigk_collect_kernel<KIND, C, true>), grid, dim3(256), 0, s, a.space, rows, a.ld, a.n, q, a.dim,
                           a.nq, radius, stride, a.lists, a.counts, a.cap);
    else
        hipLaunchKernelGGL((bigk_collect_kernel<KIND, C, false>), grid, dim3(256), 0, s, a.space, rows, a.ld, a.n, q, a.dim,
                           a.nq, radius, stride, a.lists, a.counts, a.cap);
}

template <int KIND>
void bigk_launch_collect_c(dim3 grid, hipStream_t s, const BigkBatchArgs& a, const uint32_t* radius, int stride) {
    const int chunks = (a.dim + 63) / 64;
    const bool tail = a.dim % 64 != 0;
    if (chunks == 1) bigk_launch_collect<KIND, 1>(tail, grid, s, a, radius, stride);
    else if (chunks == 2) bigk_launch_collect<KIND, 2>(tail, grid, s, a, radius, stride);
    else if (chunks == 3) bigk_launch_collect<KIND, 3>(tail, grid, s, a, radius, stride);
    else bigk_launch_collect<KIND, 4>(tail, grid, s, a, radius, stride);
}

// one pass of the collect kernel: the sample (radius == null, the plan's stride) or all blocks (stride 1)
hipError_t bigk_collect(const BigkBatchArgs& a, const uint32_t* radius, int stride, dim3 grid, hipStream_t s) {
    if (a.space == SP_L2SQR_SIFT) {
        hipLaunchKernelGGL(bigk_collect_u8_kernel, grid, dim3(256), 0, s, static_cast<const uint8_t*>(a.rows), a.n,
                           static_cast<const uint8_t*>(a.queries), a.nq, radius, stride, a.lists, a.counts, a.cap);
        return hipGetLastError();
    }
    switch (a.space) {
        case SP_L2:
        case SP_L2SQR: bigk_launch_collect_c<RB_L2>(grid, s, a, radius, stride); break;
        case SP_L1: bigk_launch_collect_c<RB_L1>(grid, s, a, radius, stride); break;
        case SP_LINF: bigk_launch_collect_c<RB_LINF>(grid, s, a, radius, stride); break;
        case SP_NEGDOT:
        case SP_NORMCOS: bigk_launch_collect_c<RB_DOT>(grid, s, a, radius, stride); break;
        case SP_COSINE:
        case SP_ANGULAR: bigk_launch_collect_c<RB_COS>(grid, s, a, radius, stride); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_bf_bigk_batch(const BigkBatchArgs& a, const BfOut& out, hipStream_t s) {
    if (a.nq <= 0) return hipSuccess;
    const bool u8 = a.space == SP_L2SQR_SIFT;
    const size_t nblocks = ((size_t)a.n + 63) / 64;
    if (a.k < 1 || a.k > (int)kBigkBatchMaxK || a.n < 2 * a.k || a.cap < a.k || a.cap > (int)kBigkBatchCap || (a.cap & (a.cap - 1)) != 0 || a.stride < 1 ||
        a.rank < 1 || (!u8 && (a.dim < 1 || a.dim > (int)kBigkBatchMaxDim)) || (u8 && a.dim != 128) || a.grid_y < 1 ||
        a.sample_grid_y < 1 || (size_t)a.grid_x * 4 < nblocks ||
        (size_t)a.sample_grid_x * 4 * a.stride < nblocks ||
        (nblocks + a.stride - 1) / a.stride * 64 > (size_t)a.cap)   // the sample fits a list
        return hipErrorInvalidValue;
    const size_t lds = (size_t)a.cap * 8;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(bigk_radius_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(bigk_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bigk_clear_kernel, dim3((a.nq + 255) / 256), dim3(256), 0, s, a.counts, a.flags, a.nq);
    e = bigk_collect(a, nullptr, a.stride, dim3(a.sample_grid_x, a.sample_grid_y), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bigk_radius_kernel, dim3(a.nq), dim3(kSortThreads), lds, s, a.lists, a.counts, a.radius, a.cap, a.rank);
    e = bigk_collect(a, a.radius, 1, dim3(a.grid_x, a.grid_y), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bigk_select_kernel, dim3(a.nq), dim3(kSortThreads), lds, s, a.lists, a.counts, a.flags, a.cap, a.k,
                       out.ext_ids, out.ids, out.dists, out.cnt);
    if (u8)
        hipLaunchKernelGGL(bigk_redo_kernel<true>, dim3(a.nq), dim3(kSortThreads), 0, s, a.space, a.rows, a.ld, a.n, a.dim,
                           a.queries, a.flags, a.k, out.ext_ids, out.ids, out.dists, out.cnt);
    else
        hipLaunchKernelGGL(bigk_redo_kernel<false>, dim3(a.nq), dim3(kSortThreads), 0, s, a.space, a.rows, a.ld, a.n, a.dim,
                           a.queries, a.flags, a.k, out.ext_ids, out.ids, out.dists, out.cnt);
    return hipGetLastError();
}

}  // namespace gfxknn
