// HNSW search that filters inside the walk (gpu_inwalk=1): one wavefront per query.
//
// The two-stage route (hnsw_live_kernels.hip) walks for max(ef, k) results and then drops what the filter or the tombstones
// do not take, so a selective filter is left with a handful of results.  Here the walk itself knows who is eligible:
// disallowed and deleted nodes stay stepping stones, but only eligible nodes enter the result set, and the walk goes on
// until that set is full or the graph around the query is used up.  The rule, with cap = max(ef, k) and every order by
// (distance, position):
//   upper levels  the greedy descent of the other kernels (every node a stepping stone);
//   level 0       W = the cap smallest eligible nodes found, C = the CAPC smallest admitted nodes not yet expanded.
//                 Start: the descent's node is visited, enters C, and W if it is eligible.  While C is not empty: pop its
//                 smallest entry c; full = |W| == cap; bound = W's largest distance if full; stop if full and d(c) > bound;
//                 the unvisited neighbours of c are marked, evaluated, and admitted when !full or d < bound (full and
//                 bound as taken before the expansion); the admitted enter C, the admitted and eligible enter W, each
//                 keeping its smallest.  What falls off C stays visited.
//   result        the first min(k, |W|) entries of W.
// Keys are f32_ord(distance) << 32 | position, the subset scan's form.  W is a sorted array, C a sorted ring (a pop moves its
// head); a chunk of up to 64 new keys is merged into either the way hnsw_search_old_kernel merges into its closest-distance
// array: the new keys are ranked among themselves, an old key moves up by the number of new keys below it (chunks from the top
// down), a new key lands at its rank plus the number of old keys below it.  Keeping the smallest of a union does not depend on
// the order of the merges, so the chunks of one expansion give what one merge of the whole expansion would.
// The visited set is a per-query HBM bitset: an LDS table fills up at exactly the selectivities this kernel is for.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../hnsw_inwalk_plan.hpp"
#include "hnsw_common_dev.hpp"
#include "kernels.hpp"

namespace gfxknn {

template <class FILTER>
struct InwalkArgs {
    HnswDeviceGraph g;
    const void* queries;
    uint32_t* bitset;        // [nq][bitset_words], cleared
    size_t bitset_words;
    FILTER flt;              // allow: bit = position, n_allow positions; or null (FilterPerQuery: the query's own entry)
    const uint32_t* tomb;    // bit = position, every position of the graph; or null
    int32_t* out_ids;
    float* out_dists;
    int32_t *out_cnt, *out_ndc, *out_hops, *out_hops_up;
    int k, cap, nbcap;
};

// LDS operations of one wave execute in order; this pins the compiler's order around them
__device__ __forceinline__ void inwalk_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

template <int SPACE, class FILTER>
__global__ __launch_bounds__(64) void hnsw_inwalk_kernel(InwalkArgs<FILTER> a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const HnswDeviceGraph& g = a.g;
    const int q = blockIdx.x, lane = threadIdx.x;
    constexpr bool kU8 = DistTraits<SPACE>::kU8;
    constexpr int CAPC = (int)kInwalkCandCap;
    static_assert((CAPC & (CAPC - 1)) == 0, "C is a ring");

    // ---- LDS carve-up (inwalk_lds_bytes) ----
    const int qbytes = ((kU8 ? 128 : g.ldv * 4) + 15) & ~15;
    float* qv = reinterpret_cast<float*>(smem);                        // [ldv] (u8: 128 bytes)
    int* nbr = reinterpret_cast<int*>(smem + qbytes);                  // [nbcap]
    float* nd = reinterpret_cast<float*>(nbr + a.nbcap);               // [nbcap]
    u64* sk = reinterpret_cast<u64*>(nd + a.nbcap);                    // [64] the new keys of a chunk, sorted
    u64* W = sk + kInwalkSortKeys;                                     // [cap]
    u64* Cq = W + ((a.cap + 1) & ~1);                                  // [CAPC], entry i at (head + i) % CAPC
    uint32_t* bits = a.bitset + (size_t)q * a.bitset_words;
    // the query's filter, once and in scalars: `eligible` below runs per lane and per neighbour
    const FilterSlot fs = a.flt.at(q);
    const uint32_t* __restrict__ allow = fs.allow;
    const int n_allow = fs.n_allow;

    // ---- stage the query (as the other search kernels: the same operations in the same order) ----
    int qnorm = 0;
    if constexpr (kU8) {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(a.queries) + (size_t)q * 128;
        const int x0 = src[2 * lane], x1 = src[2 * lane + 1];
        reinterpret_cast<uint8_t*>(qv)[2 * lane] = (uint8_t)x0;
        reinterpret_cast<uint8_t*>(qv)[2 * lane + 1] = (uint8_t)x1;
        qnorm = wave_sum_i(x0 * x0 + x1 * x1);
    } else {
        const float* src = reinterpret_cast<const float*>(a.queries) + (size_t)q * g.dim;
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
    __builtin_amdgcn_wave_barrier();
    const uint8_t* qb = reinterpret_cast<const uint8_t*>(qv);

    auto visit = [&](uint32_t id) -> bool {
        const uint32_t bit = 1u << (id & 31);
        const uint32_t old = atomicOr(&bits[id >> 5], bit);
        return (old & bit) == 0;
    };
    // the two tests of hnsw_keep_topk_kernel (a row added after the filter was made stands at or beyond n_allow)
    auto eligible = [&](int p) -> bool {
        bool ok = true;
        if (allow) ok = (unsigned)p < (unsigned)n_allow && ((allow[p >> 5] >> (p & 31)) & 1u) != 0;
        if (ok && a.tomb) ok = ((a.tomb[p >> 5] >> (p & 31)) & 1u) == 0;
        return ok;
    };

    int ndc = 0, hops = 0, hops_up = 0, nW = 0;
    if (g.n > 0) {
        // ---- entry point + greedy descent (hnsw_search_old_kernel's, lists walked in chunks) ----
        int cur = g.enterpoint;
        if (lane == 0) nbr[0] = cur;
        __builtin_amdgcn_wave_barrier();
        frontier_distances<SPACE>(g, qv, qb, qnorm, nbr, nd, 1, lane);
        float curdist = nd[0];
        ndc += 1;
        for (int lvl = g.maxlevel; lvl > 0; --lvl) {
            bool changed = true;
            while (changed) {
                changed = false;
                const int64_t off = g.up_off[cur] + (int64_t)(lvl - 1) * (g.maxM + 1);
                hops_up++;
                ndc += greedy_step_any<SPACE>(g, g.up_links + off, qv, qb, qnorm, nbr, nd, lane, cur, curdist, changed);
            }
        }

        // One chunk's keys (lanes with `in`) merged into the sorted keys arr[(hd + i) & mask], i < n; the capn smallest
        // stay.  Keys are distinct (their positions are).  Returns the new length.
        auto merge = [&](u64* arr, int hd, int mask, int n, int capn, bool in, u64 key) -> int {
            const u64 amask = __ballot(in);
            const int m2 = __popcll(amask);
            if (m2 == 0) return n;
            const int khi = (int)(uint32_t)(key >> 32), klo = (int)(uint32_t)key;
            int rank = 0;
            for (u64 mm = amask; mm;) {
                const int j = __ffsll((long long)mm) - 1;
                mm &= mm - 1;
                const u64 other = ((u64)(uint32_t)__builtin_amdgcn_readlane(khi, j) << 32) |
                                  (uint32_t)__builtin_amdgcn_readlane(klo, j);
                rank += other < key ? 1 : 0;
            }
            // #{old keys below the new one}, counted before anything moves
            int lo = 0, hi = in ? n : 0;
            while (__any(lo < hi)) {
                if (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (arr[(hd + mid) & mask] < key) lo = mid + 1;
                    else hi = mid;
                }
            }
            if (in) sk[rank] = key;
            inwalk_sync();
            const int newn = n + m2 < capn ? n + m2 : capn;
            // old keys below the smallest new one stay where they are
            const int first = __builtin_amdgcn_readlane(lo, __ffsll((long long)__ballot(in && rank == 0)) - 1);
            for (int base = n > 0 ? ((n - 1) / 64) * 64 : -64; base >= 0 && base + 64 > first; base -= 64) {
                const int i = base + lane;
                u64 kv = 0;
                int sh = 0;
                if (i < n) {
                    kv = arr[(hd + i) & mask];
                    int l2 = 0, h2 = m2;
                    while (l2 < h2) {  // #{sk < kv}
                        const int mid = (l2 + h2) >> 1;
                        if (sk[mid] < kv) l2 = mid + 1;
                        else h2 = mid;
                    }
                    sh = l2;
                }
                inwalk_sync();
                if (i < n && sh > 0 && i + sh < newn) arr[(hd + i + sh) & mask] = kv;
                inwalk_sync();
            }
            if (in) {
                const int np = lo + rank;
                if (np < newn) arr[(hd + np) & mask] = key;
            }
            inwalk_sync();
            return newn;
        };

        // ---- level 0 ----
        const u64 key0 = ((u64)f32_ord(curdist) << 32) | (uint32_t)cur;
        const bool e0 = eligible(cur);
        if (lane == 0) {
            (void)visit((uint32_t)cur);
            Cq[0] = key0;
            if (e0) W[0] = key0;
        }
        nW = e0 ? 1 : 0;
        int nC = 1, head = 0;
        inwalk_sync();
        while (nC > 0) {
            const u64 ckey = Cq[head];
            const bool full = nW == a.cap;
            const uint32_t bound = full ? (uint32_t)(W[nW - 1] >> 32) : 0xFFFFFFFFu;
            if (full && (uint32_t)(ckey >> 32) > bound) break;
            head = (head + 1) & (CAPC - 1);
            nC--;
            hops++;
            const int c = (int)(uint32_t)ckey;
            const int m = collect_unvisited_any(g.links0 + (size_t)c * (g.maxM0 + 1), nbr, lane, visit);
            __builtin_amdgcn_wave_barrier();
            if (m == 0) continue;
            ndc += m;
            frontier_distances<SPACE>(g, qv, qb, qnorm, nbr, nd, m, lane);
            for (int r0 = 0; r0 < m; r0 += 64) {  // list order; one trip unless the lists are wide
                const bool valid = r0 + lane < m;
                const int p = valid ? nbr[r0 + lane] : 0;
                const uint32_t od = valid ? f32_ord(nd[r0 + lane]) : 0xFFFFFFFFu;
                const u64 key = ((u64)od << 32) | (uint32_t)p;
                const bool adm = valid && (!full || od < bound);
                const bool elig = adm && eligible(p);
                nC = merge(Cq, head, CAPC - 1, nC, CAPC, adm, key);
                nW = merge(W, 0, -1, nW, a.cap, elig, key);
            }
        }
    }

    const int kk = a.k < nW ? a.k : nW;
    for (int i = lane; i < a.k; i += 64) {
        if (i < kk) {
            const u64 key = W[i];
            const int pos = (int)(uint32_t)key;
            a.out_ids[(size_t)q * a.k + i] = g.ext_ids ? g.ext_ids[pos] : pos;
            a.out_dists[(size_t)q * a.k + i] = ord_f32((uint32_t)(key >> 32));
        } else {
            a.out_ids[(size_t)q * a.k + i] = -1;
            a.out_dists[(size_t)q * a.k + i] = INFINITY;
        }
    }
    if (lane == 0) {
        if (a.out_cnt) a.out_cnt[q] = kk;
        if (a.out_ndc) a.out_ndc[q] = ndc;
        if (a.out_hops) a.out_hops[q] = hops;
        if (a.out_hops_up) a.out_hops_up[q] = hops_up;
    }
}

template <class FILTER>
static hipError_t inwalk_launch(const HnswDeviceGraph& g, int nq, int k, int ef, const void* queries, uint32_t* bitset,
                                size_t bitset_words, const FILTER& flt, const uint32_t* tomb, const HnswOut& out, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    const size_t qbytes = hnsw_subset_query_bytes(g);
    const int nbcap = hnsw_nbcap(g);
    static_assert(kInwalkNbcapMax == (size_t)HNSW_NBCAP_LDS, "the routing rule and the LDS kernels name one list length");
    if (k < 1 || ef < 1 || !bitset || bitset_words < ((size_t)(g.n > 0 ? g.n : 0) + 31) / 32 ||
        !inwalk_served((size_t)ef, (size_t)k, (size_t)nbcap, qbytes))
        return hipErrorInvalidValue;
    InwalkArgs<FILTER> a{};
    a.g = g;
    a.queries = queries;
    a.bitset = bitset;
    a.bitset_words = bitset_words;
    a.flt = flt;
    a.tomb = tomb;
    a.out_ids = out.ids;
    a.out_dists = out.dists;
    a.out_cnt = out.cnt;
    a.out_ndc = out.ndc;
    a.out_hops = out.hops;
    a.out_hops_up = out.hops_up;
    a.k = k;
    a.cap = (int)inwalk_cap((size_t)ef, (size_t)k);
    a.nbcap = nbcap;
    return hnsw_dispatch_space(g.space, [&](auto sp) -> hipError_t {
        const size_t lds = inwalk_lds_bytes((size_t)a.cap, (size_t)nbcap, qbytes);
        auto kern = hnsw_inwalk_kernel<sp.value, FILTER>;
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(nq), dim3(64), lds, s, a);
        return hipGetLastError();
    });
}

hipError_t launch_hnsw_inwalk(const HnswDeviceGraph& g, int nq, int k, int ef, const void* queries, uint32_t* bitset,
                              size_t bitset_words, const uint32_t* allow, int n_allow, const uint32_t* tomb, const HnswOut& out,
                              hipStream_t s) {
    if (n_allow < 0) return hipErrorInvalidValue;
    return inwalk_launch(g, nq, k, ef, queries, bitset, bitset_words, FilterOne{{allow, nullptr, n_allow, 0}}, tomb, out, s);
}

hipError_t launch_hnsw_inwalk_each(const HnswDeviceGraph& g, int nq, int k, int ef, const void* queries, uint32_t* bitset,
                                   size_t bitset_words, const FilterEach& each, const uint32_t* tomb, const HnswOut& out,
                                   hipStream_t s) {
    if (nq > 0 && (!each.table || !each.slot)) return hipErrorInvalidValue;
    return inwalk_launch(g, nq, k, ef, queries, bitset, bitset_words, FilterPerQuery{each}, tomb, out, s);
}

}  // namespace gfxknn
