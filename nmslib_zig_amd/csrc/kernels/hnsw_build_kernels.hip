// HNSW construction on the GPU: batched insertion.
//
// Restates Hnsw::add (src/method/hnsw.cc:534-609) for a whole batch of new nodes at once.  Per
// level, top down, three launches:
//   1. search    - kSearchElementsWithAttemptsLevel (hnsw.cc:611-708) for every new node of the
//                  batch = the search kernel in construction mode (hnsw_kernels.hip): the query is
//                  a stored row, ef = efConstruction, the whole result set is returned;
//   2. select    - HnswNode::getNeighborsByHeuristic2 (include/method/hnsw.h:129-169) on each result
//                  set -> the new node's forward list, plus one queued reverse-link request per
//                  selected neighbour;
//   3. link      - HnswNode::addFriendlevel (hnsw.h:258-314) target by target: append, or shrink
//                  with the same heuristic when the list is full.
// The nodes of one batch do not see each other while searching (like the reference's concurrent
// inserts, which lock one node at a time).  Reverse-link requests are written to fixed slots (new node x M),
// sorted by (target, new node) with one device radix sort, and applied per target in that order: any
// number of requests per target, no atomics, no dependence on scheduling -> the construction is
// deterministic.  One wavefront per node/target; no workgroup ever waits for another inside a launch.
//
// List width: the select and link kernels are instantiated for W = 128 (M, maxM <= 62, maxM0 <= 126: a list and the
// node that joins it are two items per lane) and W = 256 (M, maxM <= 127, maxM0 <= 254: four items per lane).  The
// W = 256 form also carries getNeighborsByHeuristic1 (delaunay_type = 1), so the narrow kernels stay as they were.
// Post-processing (hnsw.cc:251-330): hnsw_build_post_kernel, one wave per node, over the level-0 lists of two graphs.
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>

#include "hnsw_select_dev.hpp"
#include "kernels.hpp"

namespace gfxknn {

struct BuildArgs {
    HnswDeviceGraph g;
    int32_t* links0;
    int32_t* up_links;
    int M, delaunay, level;
    const int32_t* pts;
    int npts;
    const int32_t* cand_ids;
    const float* cand_d;
    const int32_t* cand_n;
    int stride;
    u64* req_key;        // select: [npts][M] slots, key = target << 32 | new node (pad = ~0); link: the sorted keys
    float* req_dist;     // distance(target, new node), same order as req_key
    int req_total;       // link: number of slots (valid entries sort to the front)
    int32_t* active;     // link: index of the first request of each target
    int32_t* nactive;
    // batch-mates (hnsw_build_mates_kernel): per new node up to XCAP earlier nodes of the same batch that are closer
    // than its worst candidate, ascending by distance
    int32_t* extra_ids;
    float* extra_d;
    int32_t* extra_n;
};

constexpr int XCAP = 64;

__device__ __forceinline__ int32_t* adj_list(const BuildArgs& a, int node) {
    if (a.level == 0) return a.links0 + (size_t)node * (a.g.maxM0 + 1);
    return a.up_links + a.g.up_off[node] + (int64_t)(a.level - 1) * (a.g.maxM + 1);
}

template <int SPACE, int W>
__global__ __launch_bounds__(64) void hnsw_build_select_kernel(BuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const HnswDeviceGraph& g = a.g;
    const int q = blockIdx.x, lane = threadIdx.x;
    const int qfloats = DistTraits<SPACE>::kU8 ? 32 : g.ldv;
    float* qv = reinterpret_cast<float*>(smem);                 // [ldv]
    constexpr int KW = W / 2;                                   // the new node's list: M <= 62 (W = 128) or <= 127
    float* nd = qv + qfloats;                                   // [KW]
    int* kept_id = reinterpret_cast<int*>(nd + KW);             // [KW]
    float* kept_d = reinterpret_cast<float*>(kept_id + KW);     // [KW]
    int* lc_id = reinterpret_cast<int*>(kept_d + KW);           // [stride]
    float* lc_d = reinterpret_cast<float*>(lc_id + a.stride);   // [stride]

    const int p = a.pts[q];
    int nc = a.cand_n[q];
    const int nx = a.extra_n ? a.extra_n[q] : 0;
    if (nx == 0) {
        for (int i = lane; i < nc; i += 64) {
            lc_id[i] = a.cand_ids[(size_t)q * a.stride + i];
            lc_d[i] = a.cand_d[(size_t)q * a.stride + i];
        }
    } else {
        // merge the graph-search results with the close batch-mates (both ascending; equal distances: graph
        // results first), keep the `stride` (= efConstruction) closest: what kSearchElementsWithAttemptsLevel would
        // have returned had the earlier nodes of this batch already been linked (hnsw.cc:611-708)
        const float xd = lane < nx ? a.extra_d[(size_t)q * XCAP + lane] : INFINITY;
        const int xi = lane < nx ? a.extra_ids[(size_t)q * XCAP + lane] : -1;
        int below = 0;  // graph candidates <= xd
        for (int base = 0; base < nc; base += 64) {
            const int i = base + lane;
            const float cd = i < nc ? a.cand_d[(size_t)q * a.stride + i] : INFINITY;
            for (int t = 0; t < nx; ++t) {
                const float xt = __shfl(xd, t, 64);
                const int c = __popcll(__ballot(i < nc && cd <= xt));
                if (lane == t) below += c;
            }
        }
        for (int base = 0; base < nc; base += 64) {
            const int i = base + lane;
            const float cd = i < nc ? a.cand_d[(size_t)q * a.stride + i] : INFINITY;
            const int cid = i < nc ? a.cand_ids[(size_t)q * a.stride + i] : -1;
            int sh = 0;  // batch-mates strictly closer than this candidate (uniform loop: shuffles need every lane)
            for (int t = 0; t < nx; ++t) sh += (__shfl(xd, t, 64) < cd) ? 1 : 0;
            if (i < nc && i + sh < a.stride) {
                lc_id[i + sh] = cid;
                lc_d[i + sh] = cd;
            }
        }
        if (lane < nx && below + lane < a.stride) {
            lc_id[below + lane] = xi;
            lc_d[below + lane] = xd;
        }
        nc = nc + nx < a.stride ? nc + nx : a.stride;
    }
    __builtin_amdgcn_wave_barrier();
    const int nk = select_neighbours<SPACE, W>(g, lc_id, lc_d, nc, a.M, a.delaunay, qv, nd, kept_id, kept_d, lane);

    // forward list of the new node: link() is called farthest first (hnsw.cc:597-601)
    int32_t* L = adj_list(a, p);
    if (lane == 0) L[0] = nk;
    // + one reverse-link request per selected neighbour, in this node's own slots
    for (int i = lane; i < nk; i += 64) {
        L[1 + i] = kept_id[nk - 1 - i];
        a.req_key[(size_t)q * a.M + i] = ((u64)(uint32_t)kept_id[i] << 32) | (uint32_t)p;
        a.req_dist[(size_t)q * a.M + i] = kept_d[i];
    }
}

// Batch-mates: the nodes of one batch are searched against the graph as it was BEFORE the batch, so a node never meets
// the earlier nodes of its own batch -- harmless for shuffled data, fatal for data whose insertion order has locality
// (near-duplicates arriving together end up linked only to their common old neighbours).  This kernel gives node j what
// sequential insertion gives it: every EARLIER node of the batch (same level slice) that is closer than its worst
// graph-search candidate, by exhaustive distance evaluation (one wave per node, 32 rows per gather; the batch's rows
// are L2 / Infinity-Cache resident).  The select kernel merges them into the candidate list.
template <int SPACE>
__global__ __launch_bounds__(64) void hnsw_build_mates_kernel(BuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const HnswDeviceGraph& g = a.g;
    const int q = blockIdx.x, lane = threadIdx.x;
    const int qfloats = DistTraits<SPACE>::kU8 ? 32 : g.ldv;
    float* qv = reinterpret_cast<float*>(smem);                 // [ldv]
    int* nbr = reinterpret_cast<int*>(qv + qfloats);            // [32]
    float* nd = reinterpret_cast<float*>(nbr + 32);             // [32]
    int* xid = reinterpret_cast<int*>(nd + 32);                 // [XCAP + 32] kept + newly accepted
    float* xdv = reinterpret_cast<float*>(xid + XCAP + 32);     // [XCAP + 32]
    int* tid_ = reinterpret_cast<int*>(xdv + XCAP + 32);        // [XCAP + 32] rank-sort scratch
    float* tdv = reinterpret_cast<float*>(tid_ + XCAP + 32);    // [XCAP + 32]

    int nx = 0;
    if (q > 0) {
        const int p = a.pts[q];
        const int nc = a.cand_n[q];
        float thr = nc >= a.stride ? a.cand_d[(size_t)q * a.stride + nc - 1] : INFINITY;  // full list: must beat its worst
        int qnorm;
        stage_row<SPACE>(g, p, qv, qnorm, lane);
        for (int base = 0; base < q; base += 32) {
            const int m = min(32, q - base);
            if (lane < m) nbr[lane] = a.pts[base + lane];
            __builtin_amdgcn_wave_barrier();
            frontier_distances<SPACE>(g, qv, reinterpret_cast<const uint8_t*>(qv), qnorm, nbr, nd, m, lane);
            const float d = lane < m ? nd[lane] : INFINITY;
            const bool acc = lane < m && d < thr;
            const u64 am = __ballot(acc);
            if (am == 0) continue;
            const int na = __popcll(am);
            if (acc) {
                const int slot = nx + __popcll(am & ((1ull << lane) - 1ull));
                xid[slot] = nbr[lane];
                xdv[slot] = d;
            }
            __builtin_amdgcn_wave_barrier();
            // rank-sort the nx + na entries (distance, then arrival order), keep the XCAP closest
            const int tot = nx + na;
            for (int i = lane; i < tot; i += 64) {
                tid_[i] = xid[i];
                tdv[i] = xdv[i];
            }
            __builtin_amdgcn_wave_barrier();
            for (int i = lane; i < tot; i += 64) {
                const float di = tdv[i];
                int r = 0;
                for (int j = 0; j < tot; ++j) {
                    const float dj = tdv[j];
                    r += (dj < di || (dj == di && j < i)) ? 1 : 0;
                }
                if (r < XCAP) {
                    xid[r] = tid_[i];
                    xdv[r] = di;
                }
            }
            nx = tot < XCAP ? tot : XCAP;
            __builtin_amdgcn_wave_barrier();
            if (nx == XCAP) thr = fminf(thr, xdv[XCAP - 1]);
        }
    }
    if (lane == 0) a.extra_n[q] = nx;
    if (lane < nx) {
        a.extra_ids[(size_t)q * XCAP + lane] = xid[lane];
        a.extra_d[(size_t)q * XCAP + lane] = xdv[lane];
    }
}

// first request of every target in the sorted list -> active[]
__global__ void hnsw_build_heads_kernel(const u64* keys, int total, int32_t* active, int32_t* nactive) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const u64 k = keys[i];
    if (k == ~0ull) return;
    if (i == 0 || (uint32_t)(keys[i - 1] >> 32) != (uint32_t)(k >> 32)) active[atomicAdd(nactive, 1)] = i;
}

template <int SPACE, int W>   // W: list width = maxM0 friends + the new node (128: maxM0 <= 126; 256: maxM0 <= 254)
__global__ __launch_bounds__(64) void hnsw_build_link_kernel(BuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const HnswDeviceGraph& g = a.g;
    const int lane = threadIdx.x;
    if ((int)blockIdx.x >= *a.nactive) return;
    const int qfloats = DistTraits<SPACE>::kU8 ? 32 : g.ldv;
    float* qv = reinterpret_cast<float*>(smem);                 // [ldv]
    float* nd = qv + qfloats;                                   // [W]
    int* kept_id = reinterpret_cast<int*>(nd + W);              // [W]
    float* kept_d = reinterpret_cast<float*>(kept_id + W);      // [W]
    int* fl = reinterpret_cast<int*>(kept_d + W);               // [W] current friends
    int* sc_id = fl + W;                                        // [W] friends + new node, sorted
    float* sc_d = reinterpret_cast<float*>(sc_id + W);          // [W]
    float* td = sc_d + W;                                       // [W] unsorted distances of the same

    const int first = a.active[blockIdx.x];
    const int t = (int)(uint32_t)(a.req_key[first] >> 32);
    int32_t* L = adj_list(a, t);
    const int maxsz = a.level > 0 ? g.maxM : g.maxM0;
    int cnt = L[0];
    for (int i = lane; i < cnt; i += 64) fl[i] = L[1 + i];
    __builtin_amdgcn_wave_barrier();

    // this target's requests: consecutive in the sorted list, ascending new-node id
    for (int r = first; r < a.req_total; ++r) {
        const u64 rk = a.req_key[r];
        if ((int)(uint32_t)(rk >> 32) != t || rk == ~0ull) break;
        const int p = (int)(uint32_t)rk;
        const float dp = a.req_dist[r];
        if (cnt < maxsz) {
            if (lane == 0) fl[cnt] = p;
            cnt++;
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        // full: distances of the centre t to its friends, the new node joins, heuristic over cnt+1
        int qnorm;
        stage_row<SPACE>(g, t, qv, qnorm, lane);
        frontier_distances<SPACE>(g, qv, reinterpret_cast<const uint8_t*>(qv), qnorm, fl, nd, cnt, lane);
        const int n1 = cnt + 1;
        for (int i = lane; i < cnt; i += 64) td[i] = nd[i];
        if (lane == 0) {
            td[cnt] = dp;
            fl[cnt] = p;   // (slot cnt <= W - 2 is free: the list is rebuilt below)
        }
        __builtin_amdgcn_wave_barrier();
        // rank sort by (distance, list position), up to W / 64 items per lane
        constexpr int E = W / 64;
        float dv[E];
        int rank[E];
#pragma unroll
        for (int e = 0; e < E; ++e) {
            dv[e] = lane + 64 * e < n1 ? td[lane + 64 * e] : INFINITY;
            rank[e] = 0;
        }
        for (int j = 0; j < n1; ++j) {
            const float dj = td[j];
#pragma unroll
            for (int e = 0; e < E; ++e) rank[e] += (dj < dv[e] || (dj == dv[e] && j < lane + 64 * e)) ? 1 : 0;
        }
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (lane + 64 * e < n1) {
                sc_id[rank[e]] = fl[lane + 64 * e];
                sc_d[rank[e]] = dv[e];
            }
        __builtin_amdgcn_wave_barrier();
        const int nk = select_neighbours<SPACE, W>(g, sc_id, sc_d, n1, n1 - 1, a.delaunay, qv, nd, kept_id, kept_d, lane);
        // refilled farthest first (hnsw.h:295-300)
        for (int i = lane; i < nk; i += 64) fl[i] = kept_id[nk - 1 - i];
        cnt = nk;
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0) L[0] = cnt;
    for (int i = lane; i < maxsz; i += 64) L[1 + i] = i < cnt ? fl[i] : 0;
}

// ---- post-processing (hnsw.cc:251-330) ------------------------------------------------------------------------------
// Two graphs over the same rows: `first` built in insertion order, `second` in reverse order.  Every node but node 0
// gets new level-0 friends from the union of its two lists (the second graph's entries, then the first graph's that
// are not among them): post = 1 keeps the union whole, post = 2 ranks it again by (distance, position) and selects
// maxM0 of it (delaunay_type 0: the closest; 1 and 2: heuristic 1), farthest first in the list.  One wave per node.
struct PostArgs {
    HnswDeviceGraph g;        // rows and distance
    const int32_t* second;    // [n][maxM0 + 1]
    const int32_t* first;     // [n][maxM0 + 1]
    int32_t* out;             // [n][out_stride], cleared by the caller
    int out_stride, maxM0, mode, delaunay;
    int32_t* max_len;         // longest list written (post = 1 widens maxM0 to it), or NULL
};

constexpr int PW = 512;       // union of two lists of up to 254

template <int SPACE>
__global__ __launch_bounds__(64) void hnsw_build_post_kernel(PostArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const HnswDeviceGraph& g = a.g;
    const int id = blockIdx.x, lane = threadIdx.x;
    const int qfloats = DistTraits<SPACE>::kU8 ? 32 : g.ldv;
    float* qv = reinterpret_cast<float*>(smem);                 // [ldv]
    float* nd = qv + qfloats;                                   // [PW]
    int* u_id = reinterpret_cast<int*>(nd + PW);                // [PW] the union
    int* s_id = u_id + PW;                                      // [PW] the union, sorted
    float* s_d = reinterpret_cast<float*>(s_id + PW);           // [PW]
    int* kept_id = reinterpret_cast<int*>(s_d + PW);            // [PW / 2]
    float* kept_d = reinterpret_cast<float*>(kept_id + PW / 2); // [PW / 2]

    const int32_t* A = a.second + (size_t)id * (a.maxM0 + 1);
    const int32_t* B = a.first + (size_t)id * (a.maxM0 + 1);
    int32_t* O = a.out + (size_t)id * a.out_stride;
    const u64 below = (1ull << lane) - 1ull;
    const int na = A[0];
    for (int i = lane; i < na; i += 64) u_id[i] = A[1 + i];
    __builtin_amdgcn_wave_barrier();
    int nu = na;
    if (id != 0) {   // (node 0 keeps the second graph's list, hnsw.cc:281)
        const int nb = B[0];
        for (int base = 0; base < nb; base += 64) {
            const int i = base + lane;
            const int v = i < nb ? B[1 + i] : -1;
            bool fresh = i < nb;
            for (int j = 0; j < na; ++j) fresh &= u_id[j] != v;
            const u64 fm = __ballot(fresh);
            if (fresh) u_id[nu + __popcll(fm & below)] = v;
            nu += __popcll(fm);
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (a.mode == 1 || id == 0 || nu == 0) {
        if (lane == 0) {
            O[0] = nu;
            if (a.max_len) atomicMax(a.max_len, nu);
        }
        for (int i = lane; i < nu; i += 64) O[1 + i] = u_id[i];
        return;
    }
    int qnorm;
    stage_row<SPACE>(g, id, qv, qnorm, lane);
    frontier_distances<SPACE>(g, qv, reinterpret_cast<const uint8_t*>(qv), qnorm, u_id, nd, nu, lane);
    __builtin_amdgcn_wave_barrier();
    // rank sort by (distance, position in the union), up to PW / 64 items per lane
    constexpr int E = PW / 64;
    float dv[E];
    int rk[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        dv[e] = lane + 64 * e < nu ? nd[lane + 64 * e] : INFINITY;
        rk[e] = 0;
    }
    for (int j = 0; j < nu; ++j) {
        const float dj = nd[j];
#pragma unroll
        for (int e = 0; e < E; ++e) rk[e] += (dj < dv[e] || (dj == dv[e] && j < lane + 64 * e)) ? 1 : 0;
    }
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (lane + 64 * e < nu) {
            s_id[rk[e]] = u_id[lane + 64 * e];
            s_d[rk[e]] = dv[e];
        }
    __builtin_amdgcn_wave_barrier();
    const int NN = a.maxM0;
    int nk;
    const int* res = s_id;
    if (a.delaunay == 0 || nu < NN) {
        nk = nu < NN ? nu : NN;
    } else {
        nk = heuristic1<SPACE>(g, s_id, s_d, nu, NN, qv, nd, kept_id, kept_d, lane);
        res = kept_id;
    }
    if (lane == 0) O[0] = nk;
    for (int i = lane; i < nk; i += 64) O[1 + i] = res[nk - 1 - i];
}

// lists of stride sstride -> lists of stride dstride (post = 1: maxM0 becomes the longest union)
__global__ void hnsw_build_repack_kernel(const int32_t* src, int sstride, int32_t* dst, int dstride, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const size_t node = i / (size_t)dstride;
    const int j = (int)(i - node * (size_t)dstride);
    const int32_t* S = src + node * (size_t)sstride;
    dst[i] = (j < sstride && j <= S[0]) ? S[j] : 0;
}

// start node of each (node, level) search = closest result of the same node's search one level up
__global__ void hnsw_build_starts_kernel(const int32_t* src, const int32_t* cand_ids, const int32_t* cand_n,
                                         int stride, int32_t* starts, int m) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const int sp = src[i];
    starts[i] = (sp >= 0 && cand_n[sp] > 0) ? cand_ids[(size_t)sp * stride] : -1;
}

hipError_t launch_hnsw_build_starts(const int32_t* src, const int32_t* cand_ids, const int32_t* cand_n, int stride,
                                    int32_t* starts, int m, hipStream_t s) {
    if (m <= 0) return hipSuccess;
    hipLaunchKernelGGL(hnsw_build_starts_kernel, dim3((m + 255) / 256), dim3(256), 0, s, src, cand_ids, cand_n,
                       stride, starts, m);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------
template <typename Kern, typename Args>
static hipError_t launch_build(Kern kern, const Args& a, int grid, size_t lds, hipStream_t s) {
    if (grid <= 0) return hipSuccess;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64), lds, s, a);
    return hipGetLastError();
}

// the W = 256 kernels: lists beyond two items per lane, and heuristic 1
static bool wide_lists(const HnswBuildGraph& bg) {
    return bg.M > 62 || bg.g.maxM > 62 || bg.g.maxM0 > 126 || bg.delaunay == 1;
}

static BuildArgs base_args(const HnswBuildGraph& bg, int level) {
    BuildArgs a{};
    a.g = bg.g;
    a.links0 = bg.links0;
    a.up_links = bg.up_links;
    a.M = bg.M;
    a.delaunay = bg.delaunay;
    a.level = level;
    return a;
}

hipError_t launch_hnsw_build_select(const HnswBuildGraph& bg, int level, const int32_t* pts, int npts,
                                    const int32_t* cand_ids, const float* cand_d, const int32_t* cand_n,
                                    int stride, const int32_t* extra_ids, const float* extra_d,
                                    const int32_t* extra_n, unsigned long long* req_key, float* req_dist,
                                    hipStream_t s) {
    if (npts <= 0) return hipSuccess;
    // unused slots keep the pad key ~0 and sort behind every real request
    hipError_t e = hipMemsetAsync(req_key, 0xFF, (size_t)npts * bg.M * 8, s);
    if (e != hipSuccess) return e;
    BuildArgs a = base_args(bg, level);
    a.pts = pts;
    a.npts = npts;
    a.cand_ids = cand_ids;
    a.cand_d = cand_d;
    a.cand_n = cand_n;
    a.stride = stride;
    a.req_key = req_key;
    a.req_dist = req_dist;
    a.extra_ids = const_cast<int32_t*>(extra_ids);
    a.extra_d = const_cast<float*>(extra_d);
    a.extra_n = const_cast<int32_t*>(extra_n);
    const size_t qbytes = bg.g.space == SP_L2SQR_SIFT ? 128 : (size_t)bg.g.ldv * 4;
    if (bg.M > 127) return hipErrorInvalidValue;
    if (wide_lists(bg)) {
        const size_t lds = qbytes + 3 * 128 * 4 + (size_t)stride * 8 + 16;
        return hnsw_dispatch_space(bg.g.space, [&](auto sp) {
            return launch_build(hnsw_build_select_kernel<sp.value, 256>, a, npts, lds, s);
        });
    }
    const size_t lds = qbytes + 3 * 64 * 4 + (size_t)stride * 8 + 16;
    return hnsw_dispatch_space(bg.g.space, [&](auto sp) {
        return launch_build(hnsw_build_select_kernel<sp.value, 128>, a, npts, lds, s);
    });
}

hipError_t launch_hnsw_build_mates(const HnswBuildGraph& bg, int level, const int32_t* pts, int npts,
                                   const float* cand_d, const int32_t* cand_n, int stride, int32_t* extra_ids,
                                   float* extra_d, int32_t* extra_n, hipStream_t s) {
    if (npts <= 0) return hipSuccess;
    BuildArgs a = base_args(bg, level);
    a.pts = pts;
    a.npts = npts;
    a.cand_d = cand_d;
    a.cand_n = cand_n;
    a.stride = stride;
    a.extra_ids = extra_ids;
    a.extra_d = extra_d;
    a.extra_n = extra_n;
    const size_t qbytes = bg.g.space == SP_L2SQR_SIFT ? 128 : (size_t)bg.g.ldv * 4;
    const size_t lds = qbytes + 2 * 32 * 4 + 4 * (size_t)(XCAP + 32) * 4 + 16;
    return hnsw_dispatch_space(bg.g.space, [&](auto sp) {
        return launch_build(hnsw_build_mates_kernel<sp.value>, a, npts, lds, s);
    });
}

size_t hnsw_build_sort_temp_bytes(int max_requests, int n) {
    size_t tmp = 0;
    int bits = 32;
    while (bits < 64 && (1ull << (bits - 32)) < (unsigned long long)n + 1) ++bits;
    (void)rocprim::radix_sort_pairs(nullptr, tmp, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                    (float*)nullptr, (float*)nullptr, (size_t)max_requests, 0, 64, nullptr, false);
    (void)bits;
    return tmp + 256;
}

// (target, new node) order of the requests of one level + the first request of every target
hipError_t launch_hnsw_build_sort_requests(const unsigned long long* req_key, const float* req_dist, int total,
                                           unsigned long long* key_sorted, float* dist_sorted, void* temp,
                                           size_t temp_bytes, int32_t* active, int32_t* nactive, hipStream_t s) {
    if (total <= 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(nactive, 0, 4, s);
    if (e != hipSuccess) return e;
    e = rocprim::radix_sort_pairs(temp, temp_bytes, req_key, key_sorted, req_dist, dist_sorted, (size_t)total, 0, 64, s,
                                  false);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hnsw_build_heads_kernel, dim3((total + 255) / 256), dim3(256), 0, s, key_sorted, total, active,
                       nactive);
    return hipGetLastError();
}

hipError_t launch_hnsw_build_link(const HnswBuildGraph& bg, int level, const int32_t* active,
                                  const int32_t* nactive, int max_active, const unsigned long long* key_sorted,
                                  const float* dist_sorted, int total, hipStream_t s) {
    BuildArgs a = base_args(bg, level);
    a.active = const_cast<int32_t*>(active);
    a.nactive = const_cast<int32_t*>(nactive);
    a.req_key = const_cast<u64*>(key_sorted);
    a.req_dist = const_cast<float*>(dist_sorted);
    a.req_total = total;
    const size_t qbytes = bg.g.space == SP_L2SQR_SIFT ? 128 : (size_t)bg.g.ldv * 4;
    if (bg.g.maxM > 254 || bg.g.maxM0 > 254) return hipErrorInvalidValue;
    if (wide_lists(bg)) {
        const size_t lds = qbytes + 7 * 256 * 4 + 16;
        return hnsw_dispatch_space(bg.g.space, [&](auto sp) {
            return launch_build(hnsw_build_link_kernel<sp.value, 256>, a, max_active, lds, s);
        });
    }
    const size_t lds = qbytes + 7 * 128 * 4 + 16;
    return hnsw_dispatch_space(bg.g.space, [&](auto sp) {
        return launch_build(hnsw_build_link_kernel<sp.value, 128>, a, max_active, lds, s);
    });
}

hipError_t launch_hnsw_build_post(const HnswDeviceGraph& g, const int32_t* second, const int32_t* first, int maxM0,
                                  int mode, int delaunay, int32_t* out, int out_stride, int32_t* max_len,
                                  hipStream_t s) {
    if (g.n <= 0) return hipSuccess;
    if (maxM0 > 254 || out_stride < (mode == 1 ? 2 * maxM0 : maxM0) + 1) return hipErrorInvalidValue;
    PostArgs a{};
    a.g = g;
    a.second = second;
    a.first = first;
    a.out = out;
    a.out_stride = out_stride;
    a.maxM0 = maxM0;
    a.mode = mode;
    a.delaunay = delaunay;
    a.max_len = max_len;
    const size_t qbytes = g.space == SP_L2SQR_SIFT ? 128 : (size_t)g.ldv * 4;
    const size_t lds = qbytes + 5 * (size_t)PW * 4 + 16;
    return hnsw_dispatch_space(g.space, [&](auto sp) {
        return launch_build(hnsw_build_post_kernel<sp.value>, a, g.n, lds, s);
    });
}

hipError_t launch_hnsw_build_repack(const int32_t* src, int sstride, int32_t* dst, int dstride, int n, hipStream_t s) {
    const size_t total = (size_t)n * (size_t)dstride;
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(hnsw_build_repack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, sstride, dst,
                       dstride, total);
    return hipGetLastError();
}

}  // namespace gfxknn
