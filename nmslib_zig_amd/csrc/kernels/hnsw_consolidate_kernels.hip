// Consolidating an HNSW graph with deleted rows (nmslib_gpu_consolidate): the adjacency lists around the
// deleted nodes are repaired in place, then rows, ids and lists are moved to the live rows' new positions.
//
//   1. worklist   - one wave per live node: every (node, level) list that holds a deleted entry goes into a worklist
//                   (the order comes from an atomic counter: the repairs do not depend on each other);
//   2. repair     - one wave per worklist entry, FreshDiskANN's one-hop rule with this project's selection test: the
//                   live entries stay, candidates are the live neighbours of the deleted entries, the closest P of them
//                   are walked in (distance, position) order until the list has its old length again;
//   3. compaction - scatter kernels: a live row, id, norm or list goes to its rank among the live rows, list entries
//                   are renumbered.
//
// The repair is race-free in place: a repair of (u, l) reads u's own list and the lists of DELETED nodes, and writes u's
// own list only.  Deleted nodes are never repaired, so no list that one wave reads is written by another, and nobody
// waits for another workgroup.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>

#include "hnsw_select_dev.hpp"
#include "kernels.hpp"

namespace gfxknn {

struct ConsArgs {
    HnswDeviceGraph g;
    int32_t* links0;
    int32_t* up_links;
    const uint32_t* tomb;     // bit = position, [ceil(n / 32)] words
    const int32_t* levels;    // [n]
    int32_t* work;            // [work_cap][2]: node, level
    int32_t* nwork;
    int work_cap;
    int delaunay, P, LW;      // pool size; entries of the list arrays in LDS (a multiple of 64 >= the longest list)
    u64* ndist;               // optional: distance evaluations of the launch (one atomic per wave)
};

__device__ __forceinline__ bool cons_dead(const uint32_t* tomb, int pos) { return (tomb[pos >> 5] >> (pos & 31)) & 1u; }

__device__ __forceinline__ int32_t* cons_list(const ConsArgs& a, int node, int level) {
    if (level == 0) return a.links0 + (size_t)node * (a.g.maxM0 + 1);
    return a.up_links + a.g.up_off[node] + (int64_t)(level - 1) * (a.g.maxM + 1);
}

// levels of `node` that have a list: its level, unless the offsets say it has no upper block
__device__ __forceinline__ int cons_top(const ConsArgs& a, int node) {
    int lv = a.levels[node];
    lv = lv < 0 ? 0 : (lv < a.g.maxlevel ? lv : a.g.maxlevel);
    return a.g.up_off[node] < 0 ? 0 : lv;
}

__global__ __launch_bounds__(256) void hnsw_cons_worklist_kernel(ConsArgs a) {
    const int lane = threadIdx.x & 63;
    const int u = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n = a.g.n;
    if (u >= n || cons_dead(a.tomb, u)) return;   // (wave-uniform)
    const int top = cons_top(a, u);
    for (int l = 0; l <= top; ++l) {
        const int32_t* L = cons_list(a, u, l);
        const int maxsz = l > 0 ? a.g.maxM : a.g.maxM0;
        int cnt = L[0];
        cnt = cnt < 0 ? 0 : (cnt < maxsz ? cnt : maxsz);
        bool flag = false;
        for (int i = lane; i < cnt; i += 64) {
            const int v = L[1 + i];
            flag |= (unsigned)v < (unsigned)n && cons_dead(a.tomb, v);
        }
        if (__any(flag) && lane == 0) {
            const int slot = atomicAdd(a.nwork, 1);
            if (slot < a.work_cap) {
                a.work[2 * (size_t)slot] = u;
                a.work[2 * (size_t)slot + 1] = l;
            }
        }
    }
}

__device__ __forceinline__ bool cons_less(float d1, int id1, float d2, int id2) {
    return d1 < d2 || (d1 == d2 && id1 < id2);
}

// One wave per worklist entry (u, l).  LDS: u's row (later a candidate's), the list arrays and the pool.
template <int SPACE>
__global__ __launch_bounds__(64) void hnsw_cons_repair_kernel(ConsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const HnswDeviceGraph& g = a.g;
    const int lane = threadIdx.x, n = g.n;
    const int qfloats = DistTraits<SPACE>::kU8 ? 32 : g.ldv;
    const int LW = a.LW, P = a.P, PC = (P + 3) / 4 * 4 + 64;
    float* qv = reinterpret_cast<float*>(smem);                 // [ldv]
    float* nd = qv + qfloats;                                   // [LW] distances of a candidate to the kept entries
    int* keep = reinterpret_cast<int*>(nd + LW);                // [LW] the new list
    int* dl = keep + LW;                                        // [LW] u's deleted entries
    int* cb_id = dl + LW;                                       // [128] candidates waiting for their distances
    float* cb_d = reinterpret_cast<float*>(cb_id + 128);        // [64]
    int* pool_id = reinterpret_cast<int*>(cb_d + 64);           // [PC] the P closest candidates, ascending (distance, position)
    float* pool_d = reinterpret_cast<float*>(pool_id + PC);     // [PC]
    int* tmp_id = reinterpret_cast<int*>(pool_d + PC);          // [PC] the merge's other side
    float* tmp_d = reinterpret_cast<float*>(tmp_id + PC);       // [PC]
    const u64 below = (1ull << lane) - 1ull;

    const int u = a.work[2 * (size_t)blockIdx.x], l = a.work[2 * (size_t)blockIdx.x + 1];
    int32_t* L = cons_list(a, u, l);
    const int maxsz = l > 0 ? g.maxM : g.maxM0;
    int cnt = L[0];
    cnt = cnt < 0 ? 0 : (cnt < maxsz ? cnt : maxsz);
    const int target = cnt;   // the old length: a list never grows

    // keep = the live entries in list order, dl = the deleted ones
    int nk = 0, ndl = 0;
    for (int base = 0; base < cnt; base += 64) {
        const int i = base + lane;
        const int v = i < cnt ? L[1 + i] : -1;
        const bool ok = (unsigned)v < (unsigned)n;
        const bool dead = ok && cons_dead(a.tomb, v), live = ok && !dead;
        const u64 lm = __ballot(live), dm = __ballot(dead);
        if (live) keep[nk + __popcll(lm & below)] = v;
        if (dead) dl[ndl + __popcll(dm & below)] = v;
        nk += __popcll(lm);
        ndl += __popcll(dm);
    }
    __builtin_amdgcn_wave_barrier();
    const int nk0 = nk;

    int qnorm;
    stage_row<SPACE>(g, u, qv, qnorm, lane);

    // distances of the first m waiting candidates, then their merge into the sorted pool (ranks by ballot-free counting:
    // a new entry lands at its lower bound in the pool plus its rank among the new ones, a pool entry moves up by the
    // number of new entries before it); what falls beyond P is dropped
    int np = 0, nc = 0;
    u64 evals = 0;   // (wave-uniform)
    auto flush = [&](int m) {
        evals += (u64)m;
        frontier_distances<SPACE>(g, qv, reinterpret_cast<const uint8_t*>(qv), qnorm, cb_id, cb_d, m, lane);
        float md = lane < m ? cb_d[lane] : INFINITY;
        if (!(md == md)) md = INFINITY;   // (a NaN would break the order the merge relies on)
        if (lane < m) cb_d[lane] = md;
        __builtin_amdgcn_wave_barrier();
        const int mi = lane < m ? cb_id[lane] : INT_MAX;
        int r = 0;
        for (int j = 0; j < m; ++j) r += cons_less(cb_d[j], cb_id[j], md, mi) ? 1 : 0;
        int lo = 0, hi = np;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cons_less(pool_d[mid], pool_id[mid], md, mi)) lo = mid + 1;
            else hi = mid;
        }
        if (lane < m && lo + r < P) {
            tmp_id[lo + r] = mi;
            tmp_d[lo + r] = md;
        }
        for (int i = lane; i < np; i += 64) {
            const float pd = pool_d[i];
            const int pi = pool_id[i];
            int c = 0;
            for (int j = 0; j < m; ++j) c += cons_less(cb_d[j], cb_id[j], pd, pi) ? 1 : 0;
            if (i + c < P) {
                tmp_id[i + c] = pi;
                tmp_d[i + c] = pd;
            }
        }
        np = np + m < P ? np + m : P;
        __builtin_amdgcn_wave_barrier();
        int* ti = pool_id;
        pool_id = tmp_id;
        tmp_id = ti;
        float* td = pool_d;
        pool_d = tmp_d;
        tmp_d = td;
        // the candidates behind the first m move to the front
        const int rest = nc - m;
        const int mv = lane < rest ? cb_id[m + lane] : 0;
        __builtin_amdgcn_wave_barrier();
        if (lane < rest) cb_id[lane] = mv;
        nc = rest;
        __builtin_amdgcn_wave_barrier();
    };

    // pool = live nodes w != u, not in keep, found in the lists of u's deleted entries (one hop), without duplicates
    for (int t = 0; t < ndl; ++t) {
        const int d = dl[t];
        if (l > cons_top(a, d)) continue;   // (a node listed on a level it does not have: nothing to follow)
        const int32_t* D = cons_list(a, d, l);
        int cd = D[0];
        cd = cd < 0 ? 0 : (cd < maxsz ? cd : maxsz);
        for (int base = 0; base < cd; base += 64) {
            const int i = base + lane;
            const int w = i < cd ? D[1 + i] : -1;
            bool ok = (unsigned)w < (unsigned)n && w != u && !cons_dead(a.tomb, w);
            for (int j = 0; j < nk0; ++j) ok &= keep[j] != w;
            for (int j = 0; j < np; ++j) ok &= pool_id[j] != w;
            for (int j = 0; j < nc; ++j) ok &= cb_id[j] != w;
            bool dup = false;   // an earlier lane of this chunk with the same node
            for (int j = 0; j < 63; ++j) {
                const int wj = __shfl(w, j, 64);
                const int okj = __shfl((int)ok, j, 64);
                dup |= j < lane && okj && wj == w;
            }
            ok &= !dup;
            const u64 am = __ballot(ok);
            if (ok) cb_id[nc + __popcll(am & below)] = w;
            nc += __popcll(am);
            __builtin_amdgcn_wave_barrier();
            if (nc >= 64) flush(64);
        }
    }
    if (nc > 0) flush(nc);

    // walk the pool while the list is shorter than it was
    if (a.delaunay == 0) {
        const int take = target - nk < np ? target - nk : np;
        for (int i = lane; i < take; i += 64) keep[nk + i] = pool_id[i];
        nk += take > 0 ? take : 0;
    } else {
        for (int i = 0; i < np && nk < target; ++i) {
            const int c = pool_id[i];
            const float dc = pool_d[i];
            bool good = true;
            if (nk > 0) {   // some kept node strictly closer to c than u is: rejected
                int cnorm;
                stage_row<SPACE>(g, c, qv, cnorm, lane);
                evals += (u64)nk;
                frontier_distances<SPACE>(g, qv, reinterpret_cast<const uint8_t*>(qv), cnorm, keep, nd, nk, lane);
                bool bad = false;
                for (int j = lane; j < nk; j += 64) bad |= nd[j] < dc;
                good = !__any(bad);
            }
            if (good) {
                if (lane == 0) {
                    keep[nk] = c;
                    pool_id[i] = ~c;   // accepted
                }
                nk++;
            }
            __builtin_amdgcn_wave_barrier();
        }
        if (a.delaunay == 1 && nk < target) {   // heuristic 1: the closest rejected candidates fill the list up
            for (int base = 0; base < np && nk < target; base += 64) {
                const int i = base + lane;
                const int c = i < np ? pool_id[i] : -1;
                const bool isr = i < np && c >= 0;
                const u64 rm = __ballot(isr);
                const int slot = nk + __popcll(rm & below);
                if (isr && slot < target) keep[slot] = c;
                nk = nk + __popcll(rm) < target ? nk + __popcll(rm) : target;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) L[0] = nk;
    for (int i = lane; i < maxsz; i += 64) L[1 + i] = i < nk ? keep[i] : 0;
    if (a.ndist && lane == 0) atomicAdd(a.ndist, evals);
}

// ---- compaction: row `r` of a live node goes to row newpos[r] ----------------------------------------------------------
template <typename V>
__global__ void hnsw_cons_scatter_kernel(const V* __restrict__ src, V* __restrict__ dst, size_t vecs, size_t total,
                                         const uint32_t* __restrict__ tomb, const int32_t* __restrict__ newpos) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t row = i / vecs;
    if (cons_dead(tomb, (int)row)) return;
    dst[(size_t)newpos[row] * vecs + (i - row * vecs)] = src[i];
}

// level-0 lists: count, the entries renumbered, unused slots 0
__global__ void hnsw_cons_links0_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int stride, int n,
                                        size_t total, const uint32_t* __restrict__ tomb,
                                        const int32_t* __restrict__ newpos) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t node = i / (size_t)stride;
    if (cons_dead(tomb, (int)node)) return;
    const int j = (int)(i - node * (size_t)stride);
    const int32_t* S = src + node * (size_t)stride;
    int cnt = S[0];
    cnt = cnt < 0 ? 0 : (cnt < stride - 1 ? cnt : stride - 1);
    int v = 0;
    if (j == 0) v = cnt;
    else if (j <= cnt) {
        const int e = S[j];
        v = (unsigned)e < (unsigned)n ? newpos[e] : 0;
    }
    dst[(size_t)newpos[node] * stride + j] = v;
}

// upper-level blocks: one wave per live node with upper levels (up_nodes: their old positions)
__global__ __launch_bounds__(64) void hnsw_cons_up_links_kernel(const int32_t* __restrict__ src,
                                                                const int64_t* __restrict__ old_off,
                                                                const int32_t* __restrict__ levels, int32_t* __restrict__ dst,
                                                                const int64_t* __restrict__ new_off,
                                                                const int32_t* __restrict__ up_nodes, int maxM, int n,
                                                                const int32_t* __restrict__ newpos) {
    const int u = up_nodes[blockIdx.x], lane = threadIdx.x;
    const int stride = maxM + 1, ints = levels[u] * stride;
    const int32_t* S = src + old_off[u];
    int32_t* O = dst + new_off[newpos[u]];
    for (int i = lane; i < ints; i += 64) {
        const int j = i % stride;
        int cnt = S[i - j];
        cnt = cnt < 0 ? 0 : (cnt < maxM ? cnt : maxM);
        int v = 0;
        if (j == 0) v = cnt;
        else if (j <= cnt) {
            const int e = S[i];
            v = (unsigned)e < (unsigned)n ? newpos[e] : 0;
        }
        O[i] = v;
    }
}

// ---------------------------------------------------------------------------------------
static ConsArgs cons_args(const HnswConsolidate& c) {
    ConsArgs a{};
    a.g = c.g;
    a.links0 = c.links0;
    a.up_links = c.up_links;
    a.tomb = c.tomb;
    a.levels = c.levels;
    a.delaunay = c.delaunay;
    a.P = c.P;
    a.ndist = c.ndist;
    const int longest = c.g.maxM0 > c.g.maxM ? c.g.maxM0 : c.g.maxM;
    a.LW = (longest + 63) / 64 * 64;
    return a;
}

hipError_t launch_hnsw_cons_worklist(const HnswConsolidate& c, int32_t* work, int work_cap, int32_t* nwork, hipStream_t s) {
    if (c.g.n <= 0) return hipSuccess;
    if (!c.tomb || !c.levels || !work || !nwork) return hipErrorInvalidValue;
    ConsArgs a = cons_args(c);
    a.work = work;
    a.work_cap = work_cap;
    a.nwork = nwork;
    hipLaunchKernelGGL(hnsw_cons_worklist_kernel, dim3((c.g.n + 3) / 4), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_hnsw_cons_repair(const HnswConsolidate& c, const int32_t* work, int nwork, hipStream_t s) {
    if (nwork <= 0) return hipSuccess;
    if (!c.tomb || !c.levels || !work || c.P < 1 || c.P > 1024 || c.g.maxM > 254 || c.g.maxM0 > 254 || c.delaunay < 0 ||
        c.delaunay > 2)
        return hipErrorInvalidValue;
    ConsArgs a = cons_args(c);
    a.work = const_cast<int32_t*>(work);
    const size_t qbytes = c.g.space == SP_L2SQR_SIFT ? 128 : (size_t)c.g.ldv * 4;
    const size_t PC = (size_t)(c.P + 3) / 4 * 4 + 64;
    const size_t lds = qbytes + (3 * (size_t)a.LW + 128 + 64 + 4 * PC) * 4 + 16;
    return hnsw_dispatch_space(c.g.space, [&](auto sp) {
        auto kern = hnsw_cons_repair_kernel<sp.value>;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(kern, dim3(nwork), dim3(64), lds, s, a);
        return hipGetLastError();
    });
}

hipError_t launch_hnsw_cons_scatter_rows(const void* src, void* dst, size_t row_bytes, int n, const uint32_t* tomb,
                                         const int32_t* newpos, hipStream_t s) {
    if (n <= 0 || row_bytes == 0) return hipSuccess;
    if (row_bytes % 4 || !tomb || !newpos) return hipErrorInvalidValue;
    if (row_bytes % 16 == 0) {
        const size_t vecs = row_bytes / 16, total = vecs * (size_t)n;
        hipLaunchKernelGGL(hnsw_cons_scatter_kernel<uint4>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                           static_cast<const uint4*>(src), static_cast<uint4*>(dst), vecs, total, tomb, newpos);
    } else {
        const size_t vecs = row_bytes / 4, total = vecs * (size_t)n;
        hipLaunchKernelGGL(hnsw_cons_scatter_kernel<uint32_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                           static_cast<const uint32_t*>(src), static_cast<uint32_t*>(dst), vecs, total, tomb, newpos);
    }
    return hipGetLastError();
}

hipError_t launch_hnsw_cons_links0(const int32_t* src, int32_t* dst, int stride, int n, const uint32_t* tomb,
                                   const int32_t* newpos, hipStream_t s) {
    const size_t total = (size_t)n * (size_t)stride;
    if (n <= 0) return hipSuccess;
    if (stride < 1 || !tomb || !newpos) return hipErrorInvalidValue;
    hipLaunchKernelGGL(hnsw_cons_links0_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, stride, n,
                       total, tomb, newpos);
    return hipGetLastError();
}

hipError_t launch_hnsw_cons_up_links(const int32_t* src, const int64_t* old_off, const int32_t* levels, int32_t* dst,
                                     const int64_t* new_off, const int32_t* up_nodes, int nup, int maxM, int n,
                                     const int32_t* newpos, hipStream_t s) {
    if (nup <= 0) return hipSuccess;
    hipLaunchKernelGGL(hnsw_cons_up_links_kernel, dim3(nup), dim3(64), 0, s, src, old_off, levels, dst, new_off, up_nodes,
                       maxM, n, newpos);
    return hipGetLastError();
}

}  // namespace gfxknn
