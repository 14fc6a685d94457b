// gpu_rows=i8: the 8-bit traversal copy of the HNSW rows and the walk over it.
//
// The copy (q8_pack.hpp): per row the codes round(x / 2^e) in [-127, 127], zero padded to whole 16-byte loads, then one more
// 16-byte slot whose first int32 is the sum of the squared codes -- a visited row is ONE contiguous gather, no second array.
// The walk: hnsw_search_kernel's SearchV1Merge (hnsw_kernels.hip), decision for decision, one wavefront per query, with
//   gather      8 lanes x 16 bytes per row and load = 128 dimensions; 8 rows per wave-load, 4 such passes (32 rows) and up
//               to 4 loads per row in flight before the first is waited for; a 768-D row is 6 loads per lane, the f32 form's
//               24.  Tails read a clamped address and are zeroed on both sides; the slot of the sum is one more load issued
//               with the others.  Nothing is loaded under a divergent branch.
//   arithmetic  integers only, exact in any order: v_dot4_i32_i8 for the dot kinds (key -dot) and for l2 (key |q|^2 + |x|^2
//               - 2 dot: the difference form would need 9-bit operands); v_sad_u8 on codes biased by 128 for l1.
//   keys        the int32 converted to f32 (v_cvt_f32_i32): monotone, exact below 2^24; beyond, neighbours may tie, which a
//               walk that is re-ranked can bear.  Never a bit-cast: comparing those depends on the denormal mode.
// cosinesimil on raw rows and angulardist order by dot / |x|, which is no integer: their key is -dot * rsq(sum of squared
// codes), two exact integers through one v_rsq_f32 and one multiplication in one lane, so still the same in every run.
// The kernel ends with its sorted array of max(ef, k) entries in the candidate workspace, array order and internal
// positions, for hnsw_rerank_kernel (hnsw_f16_kernels.hip): every distance returned is the f32 walk's.
//
// What lives only inside hnsw_kernels.hip (the body of the search, the argument filler) is restated here: that file's
// compile time is the build's longest and this one must not add to it.
#include <algorithm>
#include <cstdlib>

#include "../q8_pack.hpp"
#include "hnsw_args.hpp"
#include "hnsw_common_dev.hpp"
#include "kernels.hpp"

namespace gfxknn {

enum Q8Kind : int { Q8_L2 = 0, Q8_L1 = 1, Q8_DOT = 2 };

// ---- the copy ------------------------------------------------------------------------------------------------------
// one wave per row: four codes a lane and store, the sum of squares through the wave, the slot by four lanes
__global__ __launch_bounds__(256) void hnsw_pack_rows8_kernel(const float* __restrict__ rows, int n, int ldv, int dim,
                                                              float inv_unit, uint8_t* __restrict__ out, int ld8) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lc = ld8 - 16;
    for (int r = blockIdx.x * 4 + w; r < n; r += gridDim.x * 4) {
        const float* src = rows + (size_t)r * ldv;
        uint32_t* dst = reinterpret_cast<uint32_t*>(out + (size_t)r * ld8);
        int ss = 0;
        for (int d0 = lane * 4; d0 < lc; d0 += 256) {
            uint32_t word = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int c = d0 + j < dim ? q8pack::code(src[d0 + j] * inv_unit) : 0;
                ss += c * c;
                word |= (uint32_t)(c & 0xFF) << (8 * j);
            }
            dst[d0 >> 2] = word;
        }
        ss = wave_sum_i(ss);
        if (lane < 4) dst[(lc >> 2) + lane] = lane == 0 ? (uint32_t)ss : 0u;
    }
}

hipError_t launch_hnsw_pack_rows8(const float* rows, int n, int ldv, int dim, int scale_exp, void* rows8, int ld8,
                                  hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (ld8 != (int)q8pack::row_stride((size_t)dim)) return hipErrorInvalidValue;
    const int blocks = (int)std::min<size_t>(((size_t)n + 3) / 4, 65536);
    hipLaunchKernelGGL(hnsw_pack_rows8_kernel, dim3(blocks), dim3(256), 0, s, rows, n, ldv, dim, q8pack::inv_unit_of(scale_exp),
                       static_cast<uint8_t*>(rows8), ld8);
    return hipGetLastError();
}

// ---- distances -----------------------------------------------------------------------------------------------------
// What a lane needs of the query next to its codes in LDS: the sum of the squared codes (l2) and whether the key divides by
// the row's norm (cosinesimil on raw rows, angulardist).
struct Q8Query {
    const uint8_t* codes;  // LDS, [ld8 - 16]; l1: biased by 128
    int qn;
    bool cosnorm;
};

constexpr int Q8_PER = 16, Q8_SPAN = 128, Q8_STEP = 512;  // bytes a lane loads; the 8 lanes of a row; four such loads

template <int KIND>
__device__ __forceinline__ int q8_accum(const i32x4& q, const i32x4& b, bool ok, int acc) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if constexpr (KIND == Q8_L1) {
            // |a - b| of signed bytes = |(a + 128) - (b + 128)| of unsigned ones; the query is staged biased
            const uint32_t qq = ok ? (uint32_t)q[j] : 0u;
            const uint32_t bb = ok ? ((uint32_t)b[j] ^ 0x80808080u) : 0u;
            acc = (int)__builtin_amdgcn_sad_u8(qq, bb, (uint32_t)acc);
        } else {
            acc = __builtin_amdgcn_sdot4(ok ? q[j] : 0, ok ? b[j] : 0, acc, false);
        }
    }
    return acc;
}

// the walk's key of a row from the group's sum and the row's sum of squared codes
template <int KIND>
__device__ __forceinline__ float q8_key(int acc, int xn, const Q8Query& qq) {
    if constexpr (KIND == Q8_L2) return (float)(qq.qn + xn - 2 * acc);
    else if constexpr (KIND == Q8_L1) return (float)acc;
    else {
        if (qq.cosnorm) return xn > 0 ? -(float)acc * __builtin_amdgcn_rsqf((float)xn) : 0.f;
        return (float)(-acc);
    }
}

// the loads of up to 32 rows in flight: four loads of each row and its slot
struct Q8Loads {
    i32x4 bb[4][4];
    int xn[4];
    int ids[4];
};

__device__ __forceinline__ void q8_load_step(Q8Loads& L, const HnswDeviceGraph& g, int d0) {
    const uint8_t* rows = reinterpret_cast<const uint8_t*>(g.rows8);
    const int dlast = g.ld8 - 16 - Q8_PER;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int d = d0 + Q8_SPAN * it;
        const int dc = d < dlast ? d : dlast;
#pragma unroll
        for (int p = 0; p < 4; ++p) L.bb[it][p] = *reinterpret_cast<const i32x4*>(rows + (size_t)L.ids[p] * g.ld8 + dc);
    }
}
// (the 8 lanes of a row read the same word: one fetch, and no lane stands aside)
__device__ __forceinline__ void q8_load_norms(Q8Loads& L, const HnswDeviceGraph& g) {
    const uint8_t* rows = reinterpret_cast<const uint8_t*>(g.rows8);
#pragma unroll
    for (int p = 0; p < 4; ++p) L.xn[p] = *reinterpret_cast<const int*>(rows + (size_t)L.ids[p] * g.ld8 + (g.ld8 - 16));
}
template <int KIND>
__device__ __forceinline__ void q8_consume_step(const Q8Loads& L, const HnswDeviceGraph& g, const Q8Query& qq, int d0,
                                                int acc[4]) {
    const int lc = g.ld8 - 16, dlast = lc - Q8_PER;
#pragma unroll
    for (int it = 0; it < 4; ++it) {
        const int d = d0 + Q8_SPAN * it;
        const bool ok = d < lc;
        const int dc = d < dlast ? d : dlast;
        const i32x4 qv = *reinterpret_cast<const i32x4*>(qq.codes + dc);
#pragma unroll
        for (int p = 0; p < 4; ++p) acc[p] = q8_accum<KIND>(qv, L.bb[it][p], ok, acc[p]);
    }
}

// Keys of the query to the m rows listed in nbr[0..m) -> nd[0..m).
template <int KIND>
__device__ __forceinline__ void q8_distances(const HnswDeviceGraph& g, const Q8Query& qq, const int* nbr, float* nd, int m,
                                             int lane) {
    const int g8 = lane >> 3, sub = lane & 7;
    const int lc = g.ld8 - 16;
    for (int base_i = 0; base_i < m; base_i += 32) {
        Q8Loads L;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            // slots past m re-read the last row (a cache hit) instead of branching
            const int idx = base_i + p * 8 + g8;
            L.ids[p] = nbr[idx < m ? idx : m - 1];
        }
        int acc[4] = {0, 0, 0, 0};
        q8_load_norms(L, g);
        for (int d0 = sub * Q8_PER; d0 < lc; d0 += Q8_STEP) {
            q8_load_step(L, g, d0);
            __builtin_amdgcn_sched_barrier(0);
            q8_consume_step<KIND>(L, g, qq, d0, acc);
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int tot = group8_sum_i(acc[p]);
            const int idx = base_i + p * 8 + g8;
            if (sub == 0 && idx < m) nd[idx] = q8_key<KIND>(tot, L.xn[p], qq);
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// Split-phase form for the pipeline across expansions: issue() requests the first four loads and the slot of the first 32
// rows and returns; finish() consumes them, fetches what is left (longer rows, rows 32..m) and writes nd[0..m).
__device__ __forceinline__ void q8_issue(Q8Loads& L, const HnswDeviceGraph& g, const int* nbr, int m, int lane) {
    const int g8 = lane >> 3, sub = lane & 7;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int idx = p * 8 + g8;
        L.ids[p] = nbr[idx < m ? idx : m - 1];
    }
    q8_load_norms(L, g);
    q8_load_step(L, g, sub * Q8_PER);
    __builtin_amdgcn_sched_barrier(0);
}
template <int KIND>
__device__ __forceinline__ void q8_finish(Q8Loads& L, const HnswDeviceGraph& g, const Q8Query& qq, const int* nbr, float* nd,
                                          int m, int lane) {
    const int g8 = lane >> 3, sub = lane & 7;
    const int lc = g.ld8 - 16;
    int acc[4] = {0, 0, 0, 0};
    for (int d0 = sub * Q8_PER; d0 < lc; d0 += Q8_STEP) {
        if (d0 != sub * Q8_PER) {
            q8_load_step(L, g, d0);
            __builtin_amdgcn_sched_barrier(0);
        }
        q8_consume_step<KIND>(L, g, qq, d0, acc);
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int tot = group8_sum_i(acc[p]);
        const int idx = p * 8 + g8;
        if (sub == 0 && idx < m) nd[idx] = q8_key<KIND>(tot, L.xn[p], qq);
    }
    __builtin_amdgcn_wave_barrier();
    if (m > 32) q8_distances<KIND>(g, qq, nbr + 32, nd + 32, m - 32, lane);
}

// one greedy step on an upper level over a list of any length (greedy_step_any of hnsw_common_dev.hpp on the copy)
template <int KIND>
__device__ __forceinline__ int q8_greedy_step_any(const HnswDeviceGraph& g, const int* list, const Q8Query& qq, int* nbr,
                                                  float* nd, int lane, int& cur, float& curdist, bool& changed) {
    const int cnt = __builtin_amdgcn_readfirstlane(list[0]);
    for (int c0 = 0; c0 < cnt; c0 += 64)
        if (c0 + lane < cnt) nbr[c0 + lane] = list[c0 + lane + 1];
    __builtin_amdgcn_wave_barrier();
    if (cnt > 0) {
        q8_distances<KIND>(g, qq, nbr, nd, cnt, lane);
        u64 key = ~0ull;
        for (int c0 = 0; c0 < cnt; c0 += 64) {
            const int i = c0 + lane;
            if (i < cnt) {
                const u64 k2 = ((u64)f32_ord(nd[i]) << 32) | (uint32_t)i;
                key = k2 < key ? k2 : key;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const u64 other = __shfl_xor(key, o, 64);
            key = other < key ? other : key;
        }
        const float dmin = ord_f32((uint32_t)(key >> 32));
        if (dmin < curdist) {
            curdist = dmin;
            cur = nbr[(uint32_t)key];
            changed = true;
        }
    }
    __builtin_amdgcn_wave_barrier();
    return cnt;
}

// ---- the walk ------------------------------------------------------------------------------------------------------
// LDS as hnsw_make_plan sizes it for the f32 kernel: keys / ids of the sorted array, the query's slot (ldv floats there;
// here its codes, a quarter of it), the frontier arrays, the accepted items, the visited table.
template <int KIND, bool BITSET, int SA_EMAX, bool WIDE>
__device__ __forceinline__ void hnsw_search_q8_body(const HnswArgs& a, char* smem, const int q, uint32_t* const bits) {
    const HnswDeviceGraph& g = a.g;
    const int lane = threadIdx.x;

    float* keys = reinterpret_cast<float*>(smem);                  // [capa]
    int* idu = reinterpret_cast<int*>(keys + a.capa);              // [capa]  id | used<<31
    uint8_t* qc = reinterpret_cast<uint8_t*>(idu + a.capa);        // [ld8 - 16] codes, in the f32 kernel's [ldv] floats
    const int nbcap = WIDE ? a.nbcap : 64;
    int* nbr = reinterpret_cast<int*>(qc + (size_t)g.ldv * 4);     // [nbcap]
    float* nd = reinterpret_cast<float*>(nbr + nbcap);             // [nbcap]
    float* sk = nd + nbcap;                                        // [64] accepted keys, sorted
    int* si = reinterpret_cast<int*>(sk + 64);                     // [64] accepted ids
    uint32_t* table = reinterpret_cast<uint32_t*>(si + 64);        // [table_size]

    // ---- the query's codes: once, in LDS ----
    // l2, l1: the index's unit, clamped (a query far outside the data saturates).  Dot kinds: only the order of q.x matters,
    // so the query -- normalised first where the f32 kernels normalise it, with their operations -- takes a unit of its own
    // that puts its largest |element| into [64, 128).
    Q8Query qq;
    qq.codes = qc;
    qq.cosnorm = g.space == SP_COSINE || g.space == SP_ANGULAR;
    {
        const float* src = reinterpret_cast<const float*>(a.queries) + (size_t)q * g.dim;
        const int lc = g.ld8 - 16;
        float ss = 0.f, mx = 0.f;
        for (int d = lane; d < g.dim; d += 64) {
            const float v = src[d];
            ss = fmaf(v, v, ss);
            mx = fmaxf(mx, fabsf(v));
        }
        float inv = 1.0f;
        if (g.normalize_query) {
            ss = wave_sum(ss);
            if (ss != 0.0f) inv = 1.0f / sqrtf(ss);
        }
        float mult;
        if constexpr (KIND == Q8_DOT) {
            // (rounding is monotone: the largest |v * inv| is the largest |v| times inv)
            const float qmax = wave_max(mx) * inv;
            int ex = 0;
            const bool fin = qmax > 0.f && qmax < INFINITY;
            if (fin) (void)frexpf(qmax, &ex);
            const int e = 7 - ex;
            mult = fin ? ldexpf(1.0f, e < -100 ? -100 : (e > 100 ? 100 : e)) : 1.0f;
        } else {
            mult = ldexpf(1.0f, -g.scale8_exp);
        }
        int qn = 0;
        for (int d = lane; d < lc; d += 64) {
            int c = 0;
            if (d < g.dim) {
                float v = src[d];
                if (g.normalize_query) v *= inv;
                c = q8pack::code(v * mult);
            }
            qn += c * c;
            qc[d] = (uint8_t)(KIND == Q8_L1 ? (c + 128) : c);
        }
        qq.qn = KIND == Q8_L2 ? wave_sum_i(qn) : 0;
    }
    if constexpr (!BITSET) {
        for (int i = lane; i < a.table_size; i += 64) table[i] = HT_EMPTY;
    }
    __builtin_amdgcn_wave_barrier();

    int ndc = 0, hops = 0, hops_up = 0, nvisited = 0;
    bool overflow = false;

    // visited test-and-set: true when id was NOT visited before (exact)
    auto visit = [&](uint32_t id) -> bool {
        if constexpr (BITSET) {
            const uint32_t bit = 1u << (id & 31);
            const uint32_t old = atomicOr(&bits[id >> 5], bit);
            return (old & bit) == 0;
        } else {
            uint32_t hsh = (id * 2654435761u) >> a.table_shift;
            const uint32_t mask = (uint32_t)a.table_size - 1u;
            for (int probe = 0; probe < a.table_size; ++probe) {
                const uint32_t old = atomicCAS(&table[hsh], HT_EMPTY, id);
                if (old == HT_EMPTY) return true;
                if (old == id) return false;
                hsh = (hsh + 1) & mask;
            }
            return false;
        }
    };

    if (g.n == 0) {
        if (lane == 0) {
            a.out_cnt[q] = 0;
            if (a.out_ndc) a.out_ndc[q] = 0;
            if (a.out_hops) a.out_hops[q] = 0;
            if (a.out_hops_up) a.out_hops_up[q] = 0;
            if (a.status) a.status[q] = 0;
        }
        return;
    }

    // ---- entry point + greedy descent (hnsw_distfunc_opt.cc:168-198), on the copy ----
    int cur = g.enterpoint;
    if (lane == 0) nbr[0] = cur;
    __builtin_amdgcn_wave_barrier();
    q8_distances<KIND>(g, qq, nbr, nd, 1, lane);
    float curdist = nd[0];
    ndc += 1;
    for (int lvl = g.maxlevel; lvl > 0; --lvl) {
        bool changed = true;
        while (changed) {
            changed = false;
            const int64_t off = g.up_off[cur] + (int64_t)(lvl - 1) * (g.maxM + 1);
            if (WIDE && g.maxM > 62) {   // upper-level lists longer than one word per lane
                hops_up++;
                ndc += q8_greedy_step_any<KIND>(g, g.up_links + off, qq, nbr, nd, lane, cur, curdist, changed);
                continue;
            }
            const int v = (lane <= g.maxM) ? g.up_links[off + lane] : 0;
            const int cntl = __builtin_amdgcn_readfirstlane(v);
            const int nb = __shfl(v, lane + 1, 64);
            if (lane < cntl) nbr[lane] = nb;
            __builtin_amdgcn_wave_barrier();
            hops_up++;
            if (cntl > 0) {
                q8_distances<KIND>(g, qq, nbr, nd, cntl, lane);
                ndc += cntl;
                // sequential "if (d < curdist)" scan == first index attaining the minimum
                u64 key = ~0ull;
                if (lane < cntl) key = ((u64)f32_ord(nd[lane]) << 32) | (uint32_t)lane;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const u64 other = __shfl_xor(key, o, 64);
                    key = other < key ? other : key;
                }
                const float dmin = ord_f32((uint32_t)(key >> 32));
                if (dmin < curdist) {
                    curdist = dmin;
                    cur = nbr[(uint32_t)key];
                    changed = true;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }

    // ---- level 0 (hnsw_distfunc_opt.cc:200-274) ----
    int n = 1;
    if (lane == 0) {
        keys[0] = curdist;
        idu[0] = cur;
        (void)visit((uint32_t)cur);
    }
    nvisited = 1;
    __builtin_amdgcn_wave_barrier();

    // adjacency word `lane` of node c ([count][ids...])
    auto load_adj = [&](int c) -> int { return (lane <= g.maxM0) ? g.links0[(size_t)c * (g.maxM0 + 1) + lane] : 0; };
    // cursor: every item before it is used (the reference's currElem).  pre_*: adjacency of the item that will most likely be
    // expanded next, requested one expansion early.  pipe_*: the next expansion where it is certain before this one's
    // accepted items are merged in: its visited filter has run and its rows are in flight while the merge executes.
    int cursor = 0;
    int pre_node = -1, pre_v = 0, pre2_node = -1, pre2_v = 0;
    float pre_key = INFINITY;
    bool pre_ok = false;
    int pipe_node = -1, pipe_m = 0;
    Q8Loads fl;
    while (true) {
        const int lim = n < a.ef ? n : a.ef;
        // first unused item at or after cursor
        int fu = n;
        for (int base = cursor; base < n && fu == n; base += 64) {
            const int i = base + lane;
            const u64 mk = __ballot(i < n && idu[i] >= 0);
            if (mk) fu = base + (__ffsll((long long)mk) - 1);
        }
        if (fu >= lim) break;
        const int c = idu[fu] & 0x7FFFFFFF;
        if (lane == 0) idu[fu] |= (int)0x80000000;
        cursor = fu + 1;
        hops++;
        const float topKey = keys[n - 1];
        const int size0 = n;

        int m;
        if (c == pipe_node) {
            m = pipe_m;
            pipe_node = -1;
        } else {
            int v;
            if (c == pre_node) v = pre_v;
            else if (c == pre2_node) v = pre2_v;
            else v = load_adj(c);
            const int cntn = __builtin_amdgcn_readfirstlane(v);
            const int nb = __shfl(v, lane + 1, 64);   // neighbours 0..62 (list words 1..63)
            bool isn = false;
            if (lane < cntn && (!WIDE || lane < 63)) isn = visit((uint32_t)nb);
            const u64 nmask = __ballot(isn);
            m = __popcll(nmask);
            if (isn) nbr[__popcll(nmask & ((1ull << lane) - 1ull))] = nb;
            if (WIDE) {
                // neighbours 63.. are list words 64.., read in chunks of 64 (as many as the frontier arrays hold: a.nbcap)
                const int32_t* Lc = g.links0 + (size_t)c * (g.maxM0 + 1);
                for (int c0 = 63; c0 < cntn; c0 += 64) {
                    int nb2 = 0;
                    if (c0 + 1 + lane <= g.maxM0) nb2 = Lc[c0 + 1 + lane];
                    bool isn2 = false;
                    if (c0 + lane < cntn) isn2 = visit((uint32_t)nb2);
                    const u64 nmask2 = __ballot(isn2);
                    if (isn2) nbr[m + __popcll(nmask2 & ((1ull << lane) - 1ull))] = nb2;
                    m += __popcll(nmask2);
                }
            }
            nvisited += m;
            if (!BITSET && nvisited > (a.table_size - (a.table_size >> 3))) {
                overflow = true;  // visited table nearly full: give up, the bitset variant re-runs the query
                break;
            }
            __builtin_amdgcn_wave_barrier();
            // guess (A) for the next expansion: the next unused item of the array
            {
                int fu2 = n;
                for (int base = cursor; base < n && fu2 == n; base += 64) {
                    const int i = base + lane;
                    const u64 mk = __ballot(i < n && idu[i] >= 0);
                    if (mk) fu2 = base + (__ffsll((long long)mk) - 1);
                }
                if (fu2 < lim) {
                    pre_node = idu[fu2] & 0x7FFFFFFF;
                    pre_key = keys[fu2];
                    pre_v = load_adj(pre_node);
                    pre_ok = true;
                } else {
                    pre_node = -1;
                    pre_key = INFINITY;
                    pre_ok = false;
                }
                pre2_node = -1;
            }
            if (m > 0) q8_issue(fl, g, nbr, m, lane);
        }
        if (m == 0) continue;
        ndc += m;
        q8_finish<KIND>(fl, g, qq, nbr, nd, m, lane);

        for (int r0 = 0; r0 < (WIDE ? m : 1); r0 += 64) {  // one trip unless the lists are wide
            // accept d < topKey || size < ef   (:240)
            float dj = INFINITY;
            int idj = -1;
            bool acc = false;
            if (r0 + lane < m) {
                dj = nd[r0 + lane];
                idj = nbr[r0 + lane];
                acc = (dj < topKey) || (size0 < a.ef);
            }
            const u64 amask = __ballot(acc);
            const int m2 = __popcll(amask);
            if (m2 == 0) continue;
            // ascending order of the accepted items (std::sort, :251); ties keep list order
            int rank = 0;
            for (u64 mm = amask; mm;) {
                const int j = __ffsll((long long)mm) - 1;
                mm &= mm - 1;
                const float dother = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dj), j));
                rank += (dother < dj || (dother == dj && j < lane)) ? 1 : 0;
            }
            __builtin_amdgcn_wave_barrier();
            if (acc) {
                sk[rank] = dj;
                si[rank] = idj;
            }
            __builtin_amdgcn_wave_barrier();

            if (sk[0] <= pre_key) {  // guess (B): the best newly accepted item
                pre2_node = si[0];
                pre2_v = load_adj(pre2_node);
            } else if (!WIDE && pre_ok && !a.no_pipe) {
                // every accepted key is larger than the key of the array's next unused item: that item IS the next
                // expansion.  Its visited filter runs now and its rows are requested; the merge overlaps the gather.
                const int cntp = __builtin_amdgcn_readfirstlane(pre_v);
                const int nbp = __shfl(pre_v, lane + 1, 64);
                bool isp = false;
                if (lane < cntp) isp = visit((uint32_t)nbp);
                const u64 pmask = __ballot(isp);
                const int mp = __popcll(pmask);
                __builtin_amdgcn_wave_barrier();  // (nbr/nd of this expansion were consumed into registers above)
                if (isp) nbr[__popcll(pmask & ((1ull << lane) - 1ull))] = nbp;
                nvisited += mp;
                if (!BITSET && nvisited > (a.table_size - (a.table_size >> 3))) {
                    overflow = true;
                    break;
                }
                __builtin_amdgcn_wave_barrier();
                pipe_node = pre_node;
                pipe_m = mp;
                // guess for the expansion after that: the second unused item of the array, or the best accepted key
                int second = n;
                {
                    int seen = 0;
                    for (int base = cursor; base < n && second == n; base += 64) {
                        const int i = base + lane;
                        u64 mk = __ballot(i < n && idu[i] >= 0);
                        if (seen == 0 && mk) {
                            mk &= mk - 1;
                            seen = 1;
                        }
                        if (mk) second = base + (__ffsll((long long)mk) - 1);
                    }
                }
                const float k2 = second < n ? keys[second] : INFINITY;
                if (second < n && second < a.ef && k2 < sk[0]) {
                    pre_node = idu[second] & 0x7FFFFFFF;
                    pre_key = k2;
                    pre_ok = true;
                    pre_v = load_adj(pre_node);
                } else if (sk[0] < k2) {
                    pre_node = si[0];
                    pre_key = sk[0];
                    pre_ok = false;
                    pre_v = load_adj(pre_node);
                } else {
                    pre_node = -1;
                    pre_key = INFINITY;
                    pre_ok = false;
                }
                pre2_node = -1;
                if (mp > 0) q8_issue(fl, g, nbr, mp, lane);
            }
            // All accepted items at once when no two keys involved are equal: the merge of the two sorted sequences cut at
            // the capacity.  Equal keys -- the rule here, with integer keys -- take the sequential replay below.
            bool tie = false;
            float kreg[SA_EMAX];
            int cntv[SA_EMAX];
#pragma unroll
            for (int e = 0; e < SA_EMAX; ++e) {
                const int i = lane + 64 * e;
                kreg[e] = (e * 64 < n && i < n) ? keys[i] : INFINITY;
                cntv[e] = 0;
            }
            const float mykey = lane < m2 ? sk[lane] : INFINITY;
            const int myid = lane < m2 ? si[lane] : -1;
            int myless = 0;
            for (int t = 0; t < m2; ++t) {
                const float skt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mykey), t));
                int less = 0;
#pragma unroll
                for (int e = 0; e < SA_EMAX; ++e) {
                    if (e * 64 < n) {
                        less += __popcll(__ballot(kreg[e] < skt));
                        cntv[e] += (skt < kreg[e]) ? 1 : 0;
                        tie |= (skt == kreg[e]);
                    }
                }
                if (lane == t) myless = less;
            }
            // (the shuffle runs in ALL lanes: under a short-circuit it would sit in a divergent branch)
            const float next_key = __shfl_down(mykey, 1, 64);
            tie |= (lane + 1 < m2) & (mykey == next_key);
            if (!__any(tie)) {
                int ireg[SA_EMAX];
#pragma unroll
                for (int e = 0; e < SA_EMAX; ++e) {
                    const int i = lane + 64 * e;
                    ireg[e] = (e * 64 < n && i < n) ? idu[i] : 0;
                }
                const int newn = n + m2 < a.cap ? n + m2 : a.cap;
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int e = 0; e < SA_EMAX; ++e) {
                    const int i = lane + 64 * e;
                    if (e * 64 < n && i < n && cntv[e] > 0) {
                        const int np = i + cntv[e];
                        if (np < newn) {
                            keys[np] = kreg[e];
                            idu[np] = ireg[e];
                        }
                    }
                }
                if (lane < m2) {
                    const int np = myless + lane;
                    if (np < newn) {
                        keys[np] = mykey;
                        idu[np] = myid;
                    }
                }
                const int first = __builtin_amdgcn_readlane(myless, 0);
                if (first < cursor) cursor = first;
                n = newn;
                __builtin_amdgcn_wave_barrier();
            } else {
                // SortArrBI::push_or_replace_non_empty_exp for each, in order (sort_arr_bi.h:159-199)
                for (int t = 0; t < m2; ++t) {
                    const float key = sk[t];
                    const int id = si[t];
                    const float lastk = keys[n - 1];
                    if (lastk <= key) {
                        if (n < a.cap) {
                            if (lane == 0) {
                                keys[n] = key;
                                idu[n] = id;
                            }
                            n++;
                        }
                    } else {
                        // insertion index: the number of smaller keys, or, with keys equal to the new one in the array,
                        // the reference's exponential probe + lower_bound replayed (sort_arr_bi.h:172-186)
                        int less = 0, leq = 0;
#pragma unroll
                        for (int e = 0; e < SA_EMAX; ++e) {
                            if (e * 64 < n) {
                                const int i = lane + 64 * e;
                                const float kv = i < n ? keys[i] : INFINITY;
                                less += __popcll(__ballot(kv < key));
                                leq += __popcll(__ballot(kv <= key));
                            }
                        }
                        int p = less;
                        if (leq != less) {
                            int curr = n - 1, prev = curr, dstep = 1;
                            while (curr > 0 && keys[curr] > key) {
                                prev = curr;
                                curr -= dstep;
                                dstep *= 2;
                                if (dstep > curr) dstep = curr;
                            }
                            p = curr;
                            for (int i = curr; i < prev && keys[i] < key; ++i) p = i + 1;
                        }
                        const int newn = n < a.cap ? n + 1 : a.cap;
                        float rk[SA_EMAX];
                        int ri[SA_EMAX];
#pragma unroll
                        for (int e = 0; e < SA_EMAX; ++e) {
                            if (e * 64 < newn) {
                                const int i = lane + 64 * e;
                                if (i > p && i < newn) {
                                    rk[e] = keys[i - 1];
                                    ri[e] = idu[i - 1];
                                }
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
#pragma unroll
                        for (int e = 0; e < SA_EMAX; ++e) {
                            if (e * 64 < newn) {
                                const int i = lane + 64 * e;
                                if (i > p && i < newn) {
                                    keys[i] = rk[e];
                                    idu[i] = ri[e];
                                }
                            }
                        }
                        if (lane == 0) {
                            keys[p] = key;
                            idu[p] = id;
                        }
                        n = newn;
                        if (p < cursor) cursor = p;  // :261-266
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        if (overflow) break;  // (set inside the round loop by the pipelined visited filter)
    }

    // ---- the sorted array as it stands, for the re-rank: array order, internal positions (a.k = a.cap) ----
    const int kk = overflow ? 0 : (a.k < n ? a.k : n);
    for (int i = lane; i < kk; i += 64) {
        a.out_ids[(size_t)q * a.k + i] = idu[i] & 0x7FFFFFFF;
        a.out_dists[(size_t)q * a.k + i] = keys[i];
    }
    if (lane == 0) {
        a.out_cnt[q] = kk;
        if (a.out_ndc) a.out_ndc[q] = ndc;
        if (a.out_hops) a.out_hops[q] = hops;
        if (a.out_hops_up) a.out_hops_up[q] = hops_up;
        if (a.status) a.status[q] = overflow ? 1 : 0;
        if (!BITSET && overflow && a.fix_list) a.fix_list[atomicAdd(a.fix_count, 1)] = q;
    }
}

template <int KIND, bool BITSET, int EMAX, bool WIDE>
__global__ __launch_bounds__(64) void hnsw_search_q8_kernel(HnswArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if constexpr (BITSET) {
        if (a.fix_mode) {
            // queries whose LDS visited table filled up in the previous launch, re-run on HBM bitsets: workgroup b owns
            // bitset slot b and clears it before every query it takes from the list
            const int cnt = *a.fix_count;
            uint32_t* bits = a.bitset + (size_t)blockIdx.x * a.bitset_words;
            for (int slot = blockIdx.x; slot < cnt; slot += gridDim.x) {
                for (size_t i = threadIdx.x; i < a.bitset_words; i += 64) bits[i] = 0u;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                hnsw_search_q8_body<KIND, true, EMAX, WIDE>(a, smem, a.fix_list[slot], bits);
                __builtin_amdgcn_wave_barrier();
            }
            return;
        }
        hnsw_search_q8_body<KIND, true, EMAX, WIDE>(a, smem, blockIdx.x, a.bitset + (size_t)blockIdx.x * a.bitset_words);
    } else {
        hnsw_search_q8_body<KIND, false, EMAX, WIDE>(a, smem, blockIdx.x, nullptr);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------
template <int KIND, int EMAX, bool WIDE>
static hipError_t launch_q8_w(const HnswArgs& a, const HnswSearchPlan& p, hipStream_t s) {
    auto go = [&](auto kern, int grid) -> hipError_t {
        // (the dynamic LDS is named to the runtime: plans beyond the default 64 KiB exist for long rows)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds_bytes);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64), p.lds_bytes, s, a);
        return hipGetLastError();
    };
    if (p.table_size == 0) return go(hnsw_search_q8_kernel<KIND, true, EMAX, WIDE>, a.fix_mode ? a.fix_mode : a.nq);
    return go(hnsw_search_q8_kernel<KIND, false, EMAX, WIDE>, a.nq);
}

template <int KIND>
static hipError_t launch_q8_kind(const HnswArgs& a, const HnswSearchPlan& p, hipStream_t s) {
    const bool wide = hnsw_wide(a.g);
    switch (hnsw_emax(p.cap)) {
        case 2: return wide ? launch_q8_w<KIND, 2, true>(a, p, s) : launch_q8_w<KIND, 2, false>(a, p, s);
        case 4: return wide ? launch_q8_w<KIND, 4, true>(a, p, s) : launch_q8_w<KIND, 4, false>(a, p, s);
        default: return wide ? launch_q8_w<KIND, 16, true>(a, p, s) : launch_q8_w<KIND, 16, false>(a, p, s);
    }
}

hipError_t launch_hnsw_search_q8(const HnswDeviceGraph& g, const HnswSearchPlan& p, const HnswQueries& q, uint32_t* bitset,
                                 const HnswOverflow& fix, const HnswOut& out, hipStream_t s) {
    if (p.nq == 0) return hipSuccess;
    // the limits of launch_hnsw_search, and what is this kernel's own: a copy of these rows, external queries, the whole
    // array asked for, the codes within the query's slot
    if (p.cap > 64 * 16 || hnsw_nbcap(g) > HNSW_NBCAP_LDS || p.lds_bytes > HNSW_LDS_LIMIT) return hipErrorInvalidValue;
    if (!g.rows8 || g.ld8 != (int)q8pack::row_stride((size_t)g.dim) || g.ld8 - 16 > g.ldv * 4) return hipErrorInvalidValue;
    if (!q.queries || q.query_rows || q.start_nodes || q.level != 0 || p.k != p.cap) return hipErrorInvalidValue;
    if (p.table_size == 0 && !bitset) return hipErrorInvalidValue;
    HnswArgs a{};
    a.g = g;
    a.nbcap = hnsw_nbcap(g);
    a.queries = q.queries;
    a.bitset = bitset;
    a.bitset_words = p.bitset_words;
    a.out_ids = out.ids;
    a.out_dists = out.dists;
    a.out_cnt = out.cnt;
    a.out_ndc = out.ndc;
    a.out_hops = out.hops;
    a.out_hops_up = out.hops_up;
    a.status = out.status;
    a.nq = p.nq;
    a.k = p.k;
    a.ef = p.ef;
    a.cap = p.cap;
    a.capa = (p.cap + 3) & ~3;
    a.table_size = p.table_size;
    a.table_shift = p.table_shift;
    a.fix_list = fix.fix_list;
    a.fix_count = fix.fix_count;
    a.fix_mode = (p.table_size == 0) ? fix.fix_slots : 0;
    a.no_pipe = getenv("NMSLIB_HNSW_PIPE") ? atoi(getenv("NMSLIB_HNSW_PIPE")) == 0 : 0;
    switch (g.space) {
        case SP_L2:
        case SP_L2SQR: return launch_q8_kind<Q8_L2>(a, p, s);
        case SP_L1: return launch_q8_kind<Q8_L1>(a, p, s);
        case SP_NORMCOS:
        case SP_COSINE:
        case SP_ANGULAR:
        case SP_NEGDOT: return launch_q8_kind<Q8_DOT>(a, p, s);
        default: return hipErrorInvalidValue;  // linf, l2sqr_sift: not served
    }
}

}  // namespace gfxknn
