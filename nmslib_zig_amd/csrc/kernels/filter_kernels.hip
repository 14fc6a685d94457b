// Filtered search: a bitset of allowed positions becomes what the two index kinds need.
//   exact scan: the ascending list of allowed device rows (filter_count / filter_write), then the rows and ids gathered into
//               an index of their own (filter_gather_rows / filter_gather_ids);
//   HNSW:       the walk's results filtered through the allow bitset and the tombstones (hnsw_keep_topk_kernel in
//               hnsw_live_kernels.hip), or, for a subset no larger than the walk's own result array, an exact scan of the listed rows (hnsw_subset_knn_kernel).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <type_traits>

#include "../filter_plan.hpp"
#include "hnsw_common_dev.hpp"
#include "kernels.hpp"

namespace gfxknn {

// ---- ordered compaction ---------------------------------------------------------------------------------------------
// One thread per word of 32 device rows: which of them are taken, and how many.
__global__ __launch_bounds__(256) void filter_mask_kernel(const uint32_t* __restrict__ allow, int n_pos,
                                                          const uint32_t* __restrict__ tomb,
                                                          const int32_t* __restrict__ row_pos, int n_rows, int words,
                                                          uint32_t* __restrict__ mask, int32_t* __restrict__ cnt) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    const int base = w * 32;
    uint32_t m = 0;
    if (!row_pos) {
        // rows are positions: the words line up; positions at or beyond min(n_pos, n_rows) are cut off the last word
        const int lim = n_pos < n_rows ? n_pos : n_rows;
        if (base < lim) {
            m = allow[w];
            if (tomb) m &= ~tomb[w];
            const int valid = lim - base;
            if (valid < 32) m &= (1u << valid) - 1u;
        }
    } else {
        for (int b = 0; b < 32; ++b) {
            const int r = base + b;
            if (r >= n_rows) break;
            const int p = row_pos[r];
            if ((unsigned)p >= (unsigned)n_pos) continue;
            uint32_t on = (allow[p >> 5] >> (p & 31)) & 1u;
            if (tomb) on &= ~(tomb[p >> 5] >> (p & 31)) & 1u;
            m |= on << b;
        }
    }
    mask[w] = m;
    cnt[w] = __popc(m);
}

// Exclusive prefix over the words' counts, in place, by one workgroup: a thread sums its run of consecutive words, the runs
// are scanned in LDS, and the thread writes its run's prefixes.  total[0] = rows taken.
__global__ __launch_bounds__(1024) void filter_prefix_kernel(int32_t* __restrict__ cnt, int words, int32_t* __restrict__ total) {
    __shared__ int run[1024];
    const int t = threadIdx.x;
    const int per = (words + 1023) / 1024;
    const int lo = t * per < words ? t * per : words;
    const int hi = lo + per < words ? lo + per : words;
    int sum = 0;
    for (int w = lo; w < hi; ++w) sum += cnt[w];
    run[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = t >= d ? run[t - d] : 0;
        __syncthreads();
        run[t] += v;
        __syncthreads();
    }
    int at = run[t] - sum;
    for (int w = lo; w < hi; ++w) {
        const int c = cnt[w];
        cnt[w] = at;
        at += c;
    }
    if (t == 1023) total[0] = run[1023];
}

// One thread per word: its taken rows go to the list from the word's prefix on, ascending.
__global__ __launch_bounds__(256) void filter_write_kernel(const uint32_t* __restrict__ mask, const int32_t* __restrict__ prefix,
                                                           int words, int32_t* __restrict__ list) {
    const int w = blockIdx.x * 256 + threadIdx.x;
    if (w >= words) return;
    uint32_t m = mask[w];
    int at = prefix[w];
    while (m) {
        const int b = __ffs((int)m) - 1;
        list[at++] = w * 32 + b;
        m &= m - 1;
    }
}

hipError_t launch_filter_count(const uint32_t* allow, int n_pos, const uint32_t* tomb, const int32_t* row_pos, int n_rows,
                               uint32_t* mask, int32_t* prefix, int32_t* count, hipStream_t s) {
    if (n_rows < 0 || n_pos < 0 || !count) return hipErrorInvalidValue;
    const int words = (n_rows + 31) / 32;
    if (words == 0 || n_pos == 0) return hipMemsetAsync(count, 0, 4, s);
    if (!allow || !mask || !prefix) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_mask_kernel, dim3((words + 255) / 256), dim3(256), 0, s, allow, n_pos, tomb, row_pos, n_rows,
                       words, mask, prefix);
    hipLaunchKernelGGL(filter_prefix_kernel, dim3(1), dim3(1024), 0, s, prefix, words, count);
    return hipGetLastError();
}

hipError_t launch_filter_write(const uint32_t* mask, const int32_t* prefix, int n_rows, int32_t* list, hipStream_t s) {
    const int words = (n_rows + 31) / 32;
    if (words <= 0) return hipSuccess;
    if (!mask || !prefix || !list) return hipErrorInvalidValue;
    hipLaunchKernelGGL(filter_write_kernel, dim3((words + 255) / 256), dim3(256), 0, s, mask, prefix, words, list);
    return hipGetLastError();
}

// ---- row gather -----------------------------------------------------------------------------------------------------
// A row is vpr 16-byte pieces; a lane moves one piece per step.  Lanes beyond the last piece read the last one again (in
// bounds) and do not store: no load sits under a divergent branch.
__global__ __launch_bounds__(256) void filter_gather_rows_kernel(const uint4* __restrict__ src, const int32_t* __restrict__ list,
                                                                 int m, int vpr, uint4* __restrict__ dst) {
    const size_t total = (size_t)m * vpr;
    for (size_t t0 = (size_t)blockIdx.x * 256; t0 < total; t0 += (size_t)gridDim.x * 256) {
        const size_t t = t0 + threadIdx.x;
        const bool ok = t < total;
        const size_t tc = ok ? t : total - 1;
        const size_t i = tc / vpr;
        const size_t c = tc - i * vpr;
        const uint4 v = src[(size_t)list[i] * vpr + c];
        if (ok) dst[tc] = v;
    }
}

__global__ __launch_bounds__(256) void filter_gather_ids_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ list,
                                                                int m, int32_t* __restrict__ dst) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)m; i += (size_t)gridDim.x * 256) dst[i] = src[list[i]];
}

hipError_t launch_filter_gather_rows(const void* src, const int32_t* list, int m, size_t row_bytes, void* dst, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    if (!src || !list || !dst || row_bytes == 0 || row_bytes % 16 != 0 || row_bytes / 16 > (size_t)INT32_MAX)
        return hipErrorInvalidValue;
    const size_t total = (size_t)m * (row_bytes / 16);
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(filter_gather_rows_kernel, dim3(blocks), dim3(256), 0, s, static_cast<const uint4*>(src), list, m,
                       (int)(row_bytes / 16), static_cast<uint4*>(dst));
    return hipGetLastError();
}

hipError_t launch_filter_gather_ids(const int32_t* src, const int32_t* list, int m, int32_t* dst, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    if (!src || !list || !dst) return hipErrorInvalidValue;
    const int blocks = (int)std::min<size_t>(((size_t)m + 255) / 256, 65536);
    hipLaunchKernelGGL(filter_gather_ids_kernel, dim3(blocks), dim3(256), 0, s, src, list, m, dst);
    return hipGetLastError();
}

// ---- HNSW, subset route: exact scan of the listed rows ------------------------------------------------------------------
// a float's bits as an unsigned that orders like the float, and back.  (-0.0 orders before +0.0; the keys keep the bits, which
// are the walk's.  No space returns both: every sum starts at +0 and fmaf / fmaxf / fabsf never turn it into -0, so a zero
// distance is -0 for negdotprod, which negates the sum, and +0 everywhere else.  Equal distances are equal keys' high words.)
__device__ __forceinline__ uint32_t float_ord(float f) {
    const uint32_t b = __float_as_uint(f);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ord_float(uint32_t o) { return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }

constexpr int SUBSET_WAVES = 4;

// One workgroup of four waves per query.  LDS: keys [mpad] (distance order bits << 32 | position; all ones = no entry),
// the query [ldv] (u8: 128 bytes), per wave 64 positions and 64 distances, the u8 query norm.
// Wave 0 stages the query as the search kernels do (same operations in the same order: the same bits).  The waves then take
// chunks of 64 list entries through frontier_distances on the f32 rows; a deleted row's key stays "no entry".  A bitonic
// sort of the padded keys orders the entries by (distance, position).
// FILTER: FilterOne (one list of m rows for the launch, mpad its keys) or FilterPerQuery (the query's own list;
// mpad, the keys of the launch's largest list, places what stands behind the keys in LDS, and the workgroup fills and sorts
// only the keys of its own m).
template <int SPACE, class FILTER>
__global__ __launch_bounds__(64 * SUBSET_WAVES) void hnsw_subset_knn_kernel(HnswDeviceGraph g, const void* __restrict__ queries,
                                                                            FILTER flt, int mpad,
                                                                            const uint32_t* __restrict__ tomb, int k,
                                                                            int32_t* out_ids, float* out_dists, int32_t* out_cnt,
                                                                            int32_t* out_ndc, int32_t* out_hops,
                                                                            int32_t* out_hops_up) {
    using u64 = unsigned long long;
    constexpr bool kU8 = DistTraits<SPACE>::kU8;
    constexpr u64 kNone = ~0ull;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);                                   // [mpad]
    const int qfloats = kU8 ? 32 : g.ldv;
    float* qv = reinterpret_cast<float*>(keys + mpad);                          // [ldv] (u8: 128 bytes)
    int* nbr_all = reinterpret_cast<int*>(qv + qfloats);                        // [waves][64]
    float* nd_all = reinterpret_cast<float*>(nbr_all + 64 * SUBSET_WAVES);      // [waves][64]
    int* shared_i = reinterpret_cast<int*>(nd_all + 64 * SUBSET_WAVES);         // [0] u8 query norm, [1] entries
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FilterSlot fs = flt.at(q);
    const int32_t* __restrict__ list = fs.list;
    const int m = fs.m < mpad ? fs.m : mpad;  // (a list never outgrows the launch's keys)
    int msort = mpad;
    if constexpr (std::is_same<FILTER, FilterPerQuery>::value) {
        msort = 64;
        while (msort < m) msort <<= 1;
    }

    for (int i = tid; i < msort; i += 64 * SUBSET_WAVES) keys[i] = kNone;
    if (tid == 0) shared_i[1] = 0;
    if (wave == 0) {
        int qnorm = 0;
        if constexpr (kU8) {
            const uint8_t* src = reinterpret_cast<const uint8_t*>(queries) + (size_t)q * 128;
            const int x0 = src[2 * lane], x1 = src[2 * lane + 1];
            reinterpret_cast<uint8_t*>(qv)[2 * lane] = (uint8_t)x0;
            reinterpret_cast<uint8_t*>(qv)[2 * lane + 1] = (uint8_t)x1;
            qnorm = wave_sum_i(x0 * x0 + x1 * x1);
        } else {
            const float* src = reinterpret_cast<const float*>(queries) + (size_t)q * g.dim;
            float ss = 0.f;
            for (int d = lane; d < g.ldv; d += 64) {
                const float v = d < g.dim ? src[d] : 0.f;
                qv[d] = v;
                ss = fmaf(v, v, ss);
            }
            if (g.normalize_query) {
                ss = wave_sum(ss);
                if (ss != 0.0f) {
                    const float inv = 1.0f / sqrtf(ss);
                    for (int d = lane; d < g.dim; d += 64) qv[d] *= inv;
                }
            }
        }
        if (lane == 0) shared_i[0] = qnorm;
    }
    __syncthreads();
    const uint8_t* qb = reinterpret_cast<const uint8_t*>(qv);
    const int qnorm = shared_i[0];
    int* nbr = nbr_all + 64 * wave;
    float* nd = nd_all + 64 * wave;
    for (int base = 64 * wave; base < m; base += 64 * SUBSET_WAVES) {
        const int cnt = m - base < 64 ? m - base : 64;
        int pos = 0;
        if (lane < cnt) {
            pos = list[base + lane];
            pos = pos < 0 ? 0 : (pos < g.n ? pos : g.n - 1);  // (the list's positions are in range; never read outside the rows)
            nbr[lane] = pos;
        }
        __builtin_amdgcn_wave_barrier();
        frontier_distances<SPACE, float>(g, qv, qb, qnorm, nbr, nd, cnt, lane);
        __builtin_amdgcn_wave_barrier();
        if (lane < cnt) {
            const bool dead = tomb && ((tomb[pos >> 5] >> (pos & 31)) & 1u);
            if (!dead) keys[base + lane] = ((u64)float_ord(nd[lane]) << 32) | (uint32_t)pos;
        }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    for (int size = 2; size <= msort; size <<= 1) {
        for (int j = size >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < msort; i += 64 * SUBSET_WAVES) {
                const int o = i ^ j;
                if (o > i) {
                    const u64 a = keys[i], b = keys[o];
                    const bool up = (i & size) == 0;
                    if ((a > b) == up) {
                        keys[i] = b;
                        keys[o] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    // the entries stand in front of the "no entry" keys
    for (int i = tid; i < msort; i += 64 * SUBSET_WAVES)
        if (keys[i] != kNone && (i + 1 == msort || keys[i + 1] == kNone)) shared_i[1] = i + 1;
    __syncthreads();
    const int live = shared_i[1];
    const int kk = k < live ? k : live;
    for (int i = tid; i < k; i += 64 * SUBSET_WAVES) {
        if (i < kk) {
            const u64 key = keys[i];
            const int pos = (int)(uint32_t)key;
            out_ids[(size_t)q * k + i] = g.ext_ids ? g.ext_ids[pos] : pos;
            out_dists[(size_t)q * k + i] = ord_float((uint32_t)(key >> 32));
        } else {
            out_ids[(size_t)q * k + i] = -1;
            out_dists[(size_t)q * k + i] = INFINITY;
        }
    }
    if (tid == 0) {
        out_cnt[q] = kk;
        if (out_ndc) out_ndc[q] = m;
        if (out_hops) out_hops[q] = 0;
        if (out_hops_up) out_hops_up[q] = 0;
    }
}

template <class FILTER>
static hipError_t subset_launch(const HnswDeviceGraph& g, int nq, int k, const void* queries, const FILTER& flt, int m,
                                const uint32_t* tomb, const HnswOut& out, hipStream_t s) {
    static_assert(SUBSET_WAVES == 4, "filter_subset_lds_bytes counts four waves' scratch");
    const int mpad = (int)filter_subset_keys((size_t)m);
    return hnsw_dispatch_space(g.space, [&](auto sp) -> hipError_t {
        const size_t lds = filter_subset_lds_bytes((size_t)m, hnsw_subset_query_bytes(g));
        if (lds > kFilterLdsMax) return hipErrorInvalidValue;  // (filter_route sends such a batch to the walk)
        auto kern = hnsw_subset_knn_kernel<sp.value, FILTER>;
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(nq), dim3(64 * SUBSET_WAVES), lds, s, g, queries, flt, mpad, tomb, k, out.ids,
                           out.dists, out.cnt, out.ndc, out.hops, out.hops_up);
        return hipGetLastError();
    });
}

hipError_t launch_hnsw_subset_knn(const HnswDeviceGraph& g, int nq, int k, const void* queries, const int32_t* list, int m,
                                  const uint32_t* tomb, const HnswOut& out, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    if (k < 1 || m < 0 || m > HNSW_SUBSET_MAX || (m > 0 && (!list || g.n <= 0)) || !out.cnt) return hipErrorInvalidValue;
    return subset_launch(g, nq, k, queries, FilterOne{{nullptr, list, 0, m}}, m, tomb, out, s);
}

// m_max: the largest m among the launch's entries (the host knows every filter's m)
hipError_t launch_hnsw_subset_knn_each(const HnswDeviceGraph& g, int nq, int k, const void* queries, const FilterEach& each,
                                       int m_max, const uint32_t* tomb, const HnswOut& out, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    if (k < 1 || m_max < 0 || m_max > HNSW_SUBSET_MAX || (m_max > 0 && g.n <= 0) || !each.table || !each.slot || !out.cnt)
        return hipErrorInvalidValue;
    return subset_launch(g, nq, k, queries, FilterPerQuery{each}, m_max, tomb, out, s);
}

// ---- rows of any multiple of four bytes ---------------------------------------------------------------------------------
// The results of a per-query-filter batch go back to the caller's order row by row: k entries, or one counter, are rows that
// the 16-byte gather above does not take.  One word per lane and step; the same in-bounds reload for the lanes past the end.
__global__ __launch_bounds__(256) void filter_gather_words_kernel(const uint32_t* __restrict__ src,
                                                                  const int32_t* __restrict__ list, int m, int wpr,
                                                                  uint32_t* __restrict__ dst) {
    const size_t total = (size_t)m * wpr;
    for (size_t t0 = (size_t)blockIdx.x * 256; t0 < total; t0 += (size_t)gridDim.x * 256) {
        const size_t t = t0 + threadIdx.x;
        const bool ok = t < total;
        const size_t tc = ok ? t : total - 1;
        const size_t i = tc / wpr;
        const size_t c = tc - i * wpr;
        const uint32_t v = src[(size_t)list[i] * wpr + c];
        if (ok) dst[tc] = v;
    }
}

hipError_t launch_filter_gather_words(const void* src, const int32_t* list, int m, size_t row_bytes, void* dst, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    if (!src || !list || !dst || row_bytes == 0 || row_bytes % 4 != 0 || row_bytes / 4 > (size_t)INT32_MAX)
        return hipErrorInvalidValue;
    const size_t total = (size_t)m * (row_bytes / 4);
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(filter_gather_words_kernel, dim3(blocks), dim3(256), 0, s, static_cast<const uint32_t*>(src), list, m,
                       (int)(row_bytes / 4), static_cast<uint32_t*>(dst));
    return hipGetLastError();
}

}  // namespace gfxknn
