// The result filter behind an HNSW walk: deleted rows and the walk route of a filtered batch (4.6d).  The
// walk is untouched -- a deleted or disallowed node stays in the graph as a stepping stone -- and its results are filtered.
// The search is launched for cap = max(ef, k) results as internal positions into a workspace; this kernel takes, per query,
// the first k of them that the allow bitset takes and whose tombstone bit is clear.
#include <hip/hip_runtime.h>

#include <cmath>

#include "hnsw_common_dev.hpp"
#include "kernels.hpp"

namespace gfxknn {

// One wave per query.  cand / cand_d [nq][cap]: the search's results in its order, cand_n [nq] how many it wrote (nothing
// beyond them is read).  allow, tomb: either may be null (kernel arguments: the tests are wave-uniform).  Per chunk of 64
// entries a ballot of "keep" and the popcount of the ballot below the lane give a kept entry its place: the order of the
// kept entries is the search's.  FILTER: FilterOne (the launch's filter) or FilterPerQuery (the query's own).
template <class FILTER>
__global__ __launch_bounds__(64) void hnsw_keep_topk_kernel(const int32_t* __restrict__ cand, const float* __restrict__ cand_d,
                                                            const int32_t* __restrict__ cand_n, int cap, FILTER flt,
                                                            const uint32_t* __restrict__ tomb, int n,
                                                            const int32_t* __restrict__ ext_ids, int k, int32_t* out_ids,
                                                            float* out_dists, int32_t* out_cnt) {
    using u64 = unsigned long long;
    const int q = blockIdx.x, lane = threadIdx.x;
    const FilterSlot fs = flt.at(q);
    const uint32_t* __restrict__ allow = fs.allow;
    const int n_allow = fs.n_allow;
    int cnt = cand_n[q];
    cnt = cnt < 0 ? 0 : (cnt < cap ? cnt : cap);
    const int32_t* c = cand + (size_t)q * cap;
    const float* cd = cand_d + (size_t)q * cap;
    int taken = 0;  // entries kept so far (wave-uniform)
    for (int base = 0; base < cnt && taken < k; base += 64) {
        const int i = base + lane;
        int pos = -1;
        float d = INFINITY;
        bool keep = false;
        if (i < cnt) {
            pos = c[i];
            d = cd[i];
            // (the search's positions are in range, and a row added after the filter was made stands at or beyond n_allow: no
            // word outside either bitset is read)
            keep = true;
            if (allow) keep = (unsigned)pos < (unsigned)n_allow && ((allow[pos >> 5] >> (pos & 31)) & 1u) != 0;
            if (keep && tomb) keep = (unsigned)pos < (unsigned)n && ((tomb[pos >> 5] >> (pos & 31)) & 1u) == 0;
        }
        const u64 mask = __ballot(keep);
        const int at = taken + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && at < k) {
            out_ids[(size_t)q * k + at] = ext_ids ? ext_ids[pos] : pos;
            out_dists[(size_t)q * k + at] = d;
        }
        taken += __popcll(mask);
    }
    if (taken > k) taken = k;
    for (int i = taken + lane; i < k; i += 64) {
        out_ids[(size_t)q * k + i] = -1;
        out_dists[(size_t)q * k + i] = INFINITY;
    }
    if (lane == 0) out_cnt[q] = taken;
}

hipError_t launch_hnsw_keep_topk(const int32_t* cand, const float* cand_d, const int32_t* cand_n, int nq, int cap,
                                 const uint32_t* allow, int n_allow, const uint32_t* tomb, int n, const int32_t* ext_ids,
                                 int k, const HnswOut& out, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    if (k < 1 || cap < 1 || n_allow < 0 || (!allow && !tomb) || !out.cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hnsw_keep_topk_kernel<FilterOne>, dim3(nq), dim3(64), 0, s, cand, cand_d, cand_n, cap,
                       FilterOne{{allow, nullptr, n_allow, 0}}, tomb, n, ext_ids, k, out.ids, out.dists, out.cnt);
    return hipGetLastError();
}

hipError_t launch_hnsw_keep_topk_each(const int32_t* cand, const float* cand_d, const int32_t* cand_n, int nq, int cap,
                                      const FilterEach& each, const uint32_t* tomb, int n, const int32_t* ext_ids, int k,
                                      const HnswOut& out, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    if (k < 1 || cap < 1 || !each.table || !each.slot || !out.cnt) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hnsw_keep_topk_kernel<FilterPerQuery>, dim3(nq), dim3(64), 0, s, cand, cand_d, cand_n, cap,
                       FilterPerQuery{each}, tomb, n, ext_ids, k, out.ids, out.dists, out.cnt);
    return hipGetLastError();
}

}  // namespace gfxknn
