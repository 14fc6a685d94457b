// The fp16 traversal copy of the HNSW rows and the exact f32 re-rank behind an fp16 walk.  The walk itself is
// hnsw_search_kernel / hnsw_search_mw_kernel instantiated for half_t rows (hnsw_kernels.hip, hnsw_mw_kernels.hip).
#include <algorithm>

#include "../f16_pack.hpp"
#include "hnsw_common_dev.hpp"
#include "kernels.hpp"

namespace gfxknn {

__global__ __launch_bounds__(256) void hnsw_pack_rows16_kernel(const float* __restrict__ rows, int n, int ldv, int dim,
                                                               float scale, uint16_t* __restrict__ out, int ld16) {
    const size_t total = (size_t)n * ld16;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / ld16;
        const int d = (int)(i - r * ld16);
        out[i] = d < dim ? f16pack::round_f16(scale * rows[r * ldv + d]) : (uint16_t)0;
    }
}

hipError_t launch_hnsw_pack_rows16(const float* rows, int n, int ldv, int dim, float scale, void* rows16, int ld16,
                                   hipStream_t s) {
    if (n <= 0) return hipSuccess;
    const size_t total = (size_t)n * ld16;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(hnsw_pack_rows16_kernel, dim3(blocks), dim3(256), 0, s, rows, n, ldv, dim, scale,
                       static_cast<uint16_t*>(rows16), ld16);
    return hipGetLastError();
}

// One wave per query.  LDS: the query [ldv]; the candidates' positions and f32 distances [capa] each; the k best [capa] each.
// Order: (f32 distance, place in the walk's array) -- where the f32 distances order the entries as the walk's did, the first
// k are the walk's first k -- and those k come out as the search kernels emit theirs, equal distances by position.
template <int SPACE>
__global__ __launch_bounds__(64) void hnsw_rerank_kernel(HnswDeviceGraph g, const float* __restrict__ queries,
                                                         const int32_t* __restrict__ cand, const int32_t* __restrict__ cand_n,
                                                         int cap, int capa, int rerank, int k, int32_t* out_ids,
                                                         float* out_dists, int32_t* out_cnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* qv = reinterpret_cast<float*>(smem);        // [ldv]
    int* pos = reinterpret_cast<int*>(qv + g.ldv);     // [capa]
    float* nd = reinterpret_cast<float*>(pos + capa);  // [capa]
    float* sk = nd + capa;                             // [capa] the k best, in order
    int* sp = reinterpret_cast<int*>(sk + capa);       // [capa]
    const int q = blockIdx.x, lane = threadIdx.x;
    // the query as the search kernels stage it (same operations, same order: the same bits)
    {
        const float* src = queries + (size_t)q * g.dim;
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
    int n = g.n > 0 ? cand_n[q] : 0;
    n = n < cap ? n : cap;
    n = n < rerank ? n : rerank;
    for (int i = lane; i < n; i += 64) {
        const int id = cand[(size_t)q * cap + i];
        pos[i] = id < 0 ? 0 : (id < g.n ? id : g.n - 1);  // (the walk's positions are in range; never read outside the rows)
    }
    __builtin_amdgcn_wave_barrier();
    if (n > 0) frontier_distances<SPACE, float>(g, qv, reinterpret_cast<const uint8_t*>(qv), 0, pos, nd, n, lane);
    __builtin_amdgcn_wave_barrier();
    // an entry's place is the number of entries in front of it
    const int kk = k < n ? k : n;
    for (int i = lane; i < n; i += 64) {
        const float di = nd[i];
        int r = 0;
        for (int j = 0; j < n; ++j) {
            const float dj = nd[j];
            r += (dj < di || (dj == di && j < i)) ? 1 : 0;
        }
        if (r < kk) {
            sk[r] = di;
            sp[r] = pos[i];
        }
    }
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < k; i += 64) {
        if (i < kk) {
            const float ki = sk[i];
            const int id = sp[i];
            int r = i;
            for (int j = i - 1; j >= 0 && sk[j] == ki; --j) r -= (sp[j] > id) ? 1 : 0;
            for (int j = i + 1; j < kk && sk[j] == ki; ++j) r += (sp[j] < id) ? 1 : 0;
            out_ids[(size_t)q * k + r] = g.ext_ids ? g.ext_ids[id] : id;
            out_dists[(size_t)q * k + r] = ki;
        } else {
            out_ids[(size_t)q * k + i] = -1;
            out_dists[(size_t)q * k + i] = INFINITY;
        }
    }
    if (lane == 0) out_cnt[q] = kk;
}

hipError_t launch_hnsw_rerank(const HnswDeviceGraph& g, int nq, int k, int cap, int rerank, const void* queries,
                              const int32_t* cand, const int32_t* cand_n, const HnswOut& out, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    if (cap > 1024 || rerank < 1 || k < 1) return hipErrorInvalidValue;  // (the LDS search kernels' sorted array)
    const int capa = (cap + 3) & ~3;
    const size_t lds = (size_t)g.ldv * 4 + (size_t)capa * 16;
    return hnsw_dispatch_space(g.space, [&](auto sp) -> hipError_t {
        if constexpr (sp.value == SP_L2SQR_SIFT) return hipErrorInvalidValue;
        else {
            auto kern = hnsw_rerank_kernel<sp.value>;
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, dim3(nq), dim3(64), lds, s, g, static_cast<const float*>(queries), cand, cand_n, cap,
                               capa, rerank, k, out.ids, out.dists, out.cnt);
            return hipGetLastError();
        }
    });
}

}  // namespace gfxknn
