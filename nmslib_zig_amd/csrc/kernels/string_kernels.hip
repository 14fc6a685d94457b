// Exact k-NN, range and pair distances over the string spaces (data type 3): leven and bit_hamming.
//
// leven: unit-cost edit distance over bytes (levenshtein, src/distcomp_edist.cc).  It is evaluated by the
// bit-parallel recurrence of Myers (1999) in the block form of Hyyro (2001): the query is the pattern, split in
// 64-row blocks, and Peq[block][symbol] marks the pattern positions equal to the symbol; the row is the text, one
// byte per step.  Each block keeps its vertical deltas (Pv, Mv) and passes its horizontal delta at the bottom row
// (hout, -1/0/+1) to the next block as hin; block 0 starts with hin = +1 (D[0][j] = j).  The distance is m plus the
// sum of the last block's hout over the text.  Bits above the pattern's last row only ever carry upwards, so the
// last block's unused high bits never reach the bit that is read.  The distance is symmetric, so taking the query
// as the pattern gives the reference's value whichever string it makes the column.
// bit_hamming: popcount of XOR over the packed words (BitHamming, include/distcomp.h:241-250); the trailing count
// word is not stored on the device.
//
// Storage: leven rows are CSR bytes (row_ptr int64 [n+1], data uint8); bit_hamming rows are W uint32 words each,
// row-major.  Queries of a batch: leven as Peq tables (q_off int64 [nq+1] in u64 units, [nw][256] per query) plus
// their lengths; bit_hamming as W words per query.
//   leven_knn_kernel<TQ, MW> : grid (splits, query tiles).  A workgroup scans a row range for TQ queries.  256 rows
//                              at a time: their bytes are copied into LDS (coalesced dwords) when they fit kStrRowStage,
//                              else read from HBM; each lane takes one row and advances all TQ queries of the tile
//                              over it, byte by byte, so a row is read once per tile.  MW = false: every query of
//                              the tile fits one 64-bit block, state in registers, TQ = 8.  MW = true: TQ = 1, the
//                              blocks' (Pv, Mv) live in LDS (nw <= kStrMwLds) or in a per-lane HBM workspace.
//   ham_knn_kernel<TQ>       : grid (splits, query tiles); each lane streams one row (16-byte loads when W % 4 == 0)
//                              and XORs it against the tile's queries, staged in LDS.
//   Selection: the best kl keys (distance, position) of the range in LDS (SplitTopK, split_topk_dev.hpp); the
//   per-split lists are merged by launch_merge_topk_ex.  Integer distances are exact in float.
//   *_dist_kernel: distance of every row to one query (range search); *_pair_kernel: nmslib_get_distance.
#include <algorithm>

#include "kernels.hpp"
#include "split_topk_dev.hpp"

namespace gfxknn {

namespace {

// ---- the distances ---------------------------------------------------------------------------

// One 64-row block advanced by one text symbol (eq = Peq[block][symbol]); hin / the return value are the horizontal
// deltas entering at the top and leaving at row `high` of the block.
__device__ __forceinline__ int leven_block(u64 eq, u64& pv, u64& mv, int hin, u64 high) {
    const u64 xv = eq | mv;
    if (hin < 0) eq |= 1ull;
    const u64 xh = (((eq & pv) + pv) ^ pv) | eq;
    u64 ph = mv | ~(xh | pv);
    u64 mh = pv & xh;
    const int hout = (ph & high) ? 1 : ((mh & high) ? -1 : 0);
    ph <<= 1;
    mh <<= 1;
    if (hin < 0) mh |= 1ull;
    else if (hin > 0) ph |= 1ull;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
    return hout;
}

// Pattern of m <= 64 symbols (peq: 256 words) against text[0..n): the edit distance.
__device__ __forceinline__ int leven_1w(const u64* peq, int m, const uint8_t* text, int n) {
    u64 pv = ~0ull, mv = 0;
    const u64 high = 1ull << (m - 1);
    int score = m;
    for (int j = 0; j < n; ++j) score += leven_block(peq[text[j]], pv, mv, 1, high);
    return score;
}

// Pattern of any length (nw blocks, peq [nw][256]); the blocks' state at st[b * stride] (Pv) and st[(nw + b) * stride]
// (Mv), private to the caller.
__device__ __forceinline__ int leven_mw(const u64* peq, int m, int nw, const uint8_t* text, int n, u64* st,
                                        int stride) {
    for (int b = 0; b < nw; ++b) {
        st[(size_t)b * stride] = ~0ull;
        st[(size_t)(nw + b) * stride] = 0;
    }
    const u64 high_last = 1ull << ((m - 1) & 63);
    int score = m;
    for (int j = 0; j < n; ++j) {
        const int c = text[j];
        int h = 1;
        for (int b = 0; b < nw; ++b) {
            u64 pv = st[(size_t)b * stride], mv = st[(size_t)(nw + b) * stride];
            h = leven_block(peq[b * 256 + c], pv, mv, h, b == nw - 1 ? high_last : (1ull << 63));
            st[(size_t)b * stride] = pv;
            st[(size_t)(nw + b) * stride] = mv;
        }
        score += h;
    }
    return score;
}

__device__ __forceinline__ int ham_words(const uint32_t* a, const uint32_t* b, int W) {
    int s = 0;
    for (int w = 0; w < W; ++w) s += __popc(a[w] ^ b[w]);
    return s;
}

// A distance d >= 0 is the upper half of its key as it is (the integer orders as its float does)
struct KeyToDist {
    __device__ float operator()(uint32_t hi) const { return (float)hi; }
};

// ---- k-NN scans ---------------------------------------------------------------------------------

template <int TQ, bool MW>
__global__ __launch_bounds__(256) void leven_knn_kernel(const int64_t* __restrict__ row_ptr,
                                                        const uint8_t* __restrict__ data, int n, int rows_per_split,
                                                        const int64_t* __restrict__ q_off, const int32_t* __restrict__ q_len,
                                                        const u64* __restrict__ peq, int nq, int k, int kl, int P,
                                                        int nw_max, u64* __restrict__ mw_ws, float* __restrict__ out_d,
                                                        int32_t* __restrict__ out_pos) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_cnt[TQ];
    const int tid = threadIdx.x, split = blockIdx.x, q_first = blockIdx.y * TQ;
    const int tile_n = min(TQ, nq - q_first);
    SplitTopK<TQ> sel{reinterpret_cast<u64*>(smem), s_cnt, P, kl, tile_n};
    u64* s_peq = reinterpret_cast<u64*>(smem) + (size_t)TQ * P;  // the tile's Peq tables, when staged
    const int64_t p0 = q_off[q_first], p1 = q_off[q_first + tile_n];
    const bool peq_staged = p1 - p0 <= kStrPeqStage / 8;
    if (peq_staged)
        for (int64_t i = tid; i < p1 - p0; i += 256) s_peq[i] = peq[p0 + i];
    uint8_t* s_rows = reinterpret_cast<uint8_t*>(s_peq + (peq_staged ? (p1 - p0) : 0));
    // MW: the blocks' state of this lane, in LDS after the rows or in the lane's slice of the HBM workspace; both are
    // sized by the batch's largest block count nw_max (the launch decides between them the same way)
    const int nw = MW ? (int)((p1 - p0) / 256) : 1;
    u64* s_state = reinterpret_cast<u64*>(s_rows + kStrRowStage);
    const bool state_lds = MW && nw_max <= kStrMwLds;
    u64* st = MW ? (state_lds ? s_state + tid
                              : mw_ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 256 * 2 * nw_max + tid)
                 : nullptr;
    sel.init(tid);
    __syncthreads();
    const int r0 = (int)min((long long)split * rows_per_split, (long long)n);
    const int r1 = min(n, r0 + rows_per_split);
    for (int base = r0; base < r1; base += 256) {
        const int top = min(r1, base + 256);
        const int64_t c0 = row_ptr[base], c1 = row_ptr[top];
        // the chunk's bytes as aligned dwords (the store is padded so the last dword is readable): byte c0 lands at
        // s_rows[c0 & 3]
        const int64_t w0 = c0 >> 2, w1 = (c1 + 3) >> 2;
        const bool rows_staged = (w1 - w0) * 4 <= (int64_t)kStrRowStage;
        if (rows_staged) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(data) + w0;
            uint32_t* dst = reinterpret_cast<uint32_t*>(s_rows);
            for (int64_t i = tid; i < w1 - w0; i += 256) dst[i] = src[i];
        }
        __syncthreads();
        const int r = base + tid;
        if (r < r1) {
            const int64_t a = row_ptr[r];
            const int len = (int)(row_ptr[r + 1] - a);
            const uint8_t* text = rows_staged ? s_rows + (a - (w0 << 2)) : data + a;
            if constexpr (MW) {
                const u64* pq = peq_staged ? s_peq : peq + p0;
                sel.offer(0, (uint32_t)leven_mw(pq, q_len[q_first], nw, text, len, st, 256), r);
            } else {
                // all TQ queries advance over the row together: one byte read per step for the whole tile
                u64 pv[TQ], mv[TQ], high[TQ];
                int score[TQ];
                const u64* pq[TQ];
#pragma unroll
                for (int t = 0; t < TQ; ++t) {
                    const int m = t < tile_n ? q_len[q_first + t] : 1;
                    pv[t] = ~0ull;
                    mv[t] = 0;
                    high[t] = 1ull << (m - 1);
                    score[t] = m;
                    pq[t] = (peq_staged ? s_peq : peq + p0) + (size_t)256 * (t < tile_n ? t : 0);
                }
                for (int j = 0; j < len; ++j) {
                    const int c = text[j];
#pragma unroll
                    for (int t = 0; t < TQ; ++t) score[t] += leven_block(pq[t][c], pv[t], mv[t], 1, high[t]);
                }
#pragma unroll
                for (int t = 0; t < TQ; ++t)
                    if (t < tile_n) sel.offer(t, (uint32_t)score[t], r);
            }
        }
        sel.chunk_done(tid, base + 256 >= r1);  // (its first barrier also keeps s_rows until every lane is done)
    }
    sel.write(tid, split, nq, q_first, k, out_d, out_pos, KeyToDist{});
}

template <int TQ>
__global__ __launch_bounds__(256) void ham_knn_kernel(const uint32_t* __restrict__ rows, int W, int n,
                                                      int rows_per_split, const uint32_t* __restrict__ q, int nq,
                                                      int k, int kl, int P, float* __restrict__ out_d,
                                                      int32_t* __restrict__ out_pos) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_cnt[TQ];
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
    const uint32_t* qb = q_staged ? s_q : q + (size_t)q_first * W;
    sel.init(tid);
    __syncthreads();
    const int r0 = (int)min((long long)split * rows_per_split, (long long)n);
    const int r1 = min(n, r0 + rows_per_split);
    for (int base = r0; base < r1; base += 256) {
        const int r = base + tid;
        if (r < r1) {
            const uint32_t* row = rows + (size_t)r * W;
            int acc[TQ];
#pragma unroll
            for (int t = 0; t < TQ; ++t) acc[t] = 0;
            int w = 0;
            if ((W & 3) == 0) {
                for (; w < W; w += 4) {
                    const uint4 x = *reinterpret_cast<const uint4*>(row + w);
#pragma unroll
                    for (int t = 0; t < TQ; ++t) {
                        const uint32_t* qt = qb + (size_t)(t < tile_n ? t : 0) * W + w;
                        acc[t] += __popc(x.x ^ qt[0]) + __popc(x.y ^ qt[1]) + __popc(x.z ^ qt[2]) + __popc(x.w ^ qt[3]);
                    }
                }
            }
            for (; w < W; ++w) {
                const uint32_t x = row[w];
#pragma unroll
                for (int t = 0; t < TQ; ++t) acc[t] += __popc(x ^ qb[(size_t)(t < tile_n ? t : 0) * W + w]);
            }
#pragma unroll
            for (int t = 0; t < TQ; ++t)
                if (t < tile_n) sel.offer(t, (uint32_t)acc[t], r);
        }
        sel.chunk_done(tid, base + 256 >= r1);
    }
    sel.write(tid, split, nq, q_first, k, out_d, out_pos, KeyToDist{});
}

// ---- range / pair ---------------------------------------------------------------------------------

// every row against one query (m symbols, nw blocks); mw_ws: 2 * nw words per row when nw > 1
__global__ __launch_bounds__(256) void leven_dist_kernel(const int64_t* __restrict__ row_ptr,
                                                         const uint8_t* __restrict__ data, int n,
                                                         const u64* __restrict__ peq, int m, int nw,
                                                         u64* __restrict__ mw_ws, float* __restrict__ d_out) {
    const int stride = gridDim.x * 256;
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += stride) {
        const int64_t a = row_ptr[r];
        const int len = (int)(row_ptr[r + 1] - a);
        const int d = nw == 1 ? leven_1w(peq, m, data + a, len)
                              : leven_mw(peq, m, nw, data + a, len, mw_ws + blockIdx.x * 256 + threadIdx.x, stride);
        d_out[r] = (float)d;
    }
}

__global__ __launch_bounds__(256) void ham_dist_kernel(const uint32_t* __restrict__ rows, int W, int n,
                                                       const uint32_t* __restrict__ q, float* __restrict__ d_out) {
    for (int r = blockIdx.x * 256 + threadIdx.x; r < n; r += gridDim.x * 256)
        d_out[r] = (float)ham_words(rows + (size_t)r * W, q, W);
}

// text = row p2 of the store, the pattern (row p1) given by its Peq table; one lane
__global__ void leven_pair_kernel(const int64_t* __restrict__ row_ptr, const uint8_t* __restrict__ data, int p2,
                                  const u64* __restrict__ peq, int m, int nw, u64* __restrict__ mw_ws, float* out) {
    if (threadIdx.x != 0) return;
    const int64_t a = row_ptr[p2];
    const int len = (int)(row_ptr[p2 + 1] - a);
    *out = (float)(nw == 1 ? leven_1w(peq, m, data + a, len) : leven_mw(peq, m, nw, data + a, len, mw_ws, 1));
}

__global__ void ham_pair_kernel(const uint32_t* __restrict__ rows, int W, int p1, int p2, float* out) {
    if (threadIdx.x != 0) return;
    *out = (float)ham_words(rows + (size_t)p1 * W, rows + (size_t)p2 * W, W);
}


// ---- HNSW search over strings (one wave per query) ---------------------------------------------------------------
// baseSearchAlgorithmV1Merge / baseSearchAlgorithmOld (src/method/hnsw.cc:1078-1290): the greedy descent through the
// upper levels, then the level-0 walk.  Lane 0 keeps the candidate and result sets in the algorithm's order; the
// lanes compute the distances of a list's unvisited neighbours in parallel (the same device functions as the scan).
// Equal distances are ordered by position everywhere (keys (distance << 32) | position), so the walk is defined
// exactly.  Per query, in HBM: a visited bitset, the sorted array (V1Merge: max(ef, k) keys + used flags) or the
// candidate / closest / result heaps (Old), and the multi-block leven state of its 64 lanes.

struct StrQ {  // one query's operand, as the distance functions need it
    const u64* peq;
    int m, nw;
    const uint32_t* words;
};

__device__ __forceinline__ int str_dist(const StringHnswArgs& a, const StrQ& q, int node, u64* st) {
    if (a.space == SP_LEVEN) {
        const int64_t b = a.row_ptr[node];
        const int len = (int)(a.row_ptr[node + 1] - b);
        return q.nw == 1 ? leven_1w(q.peq, q.m, a.data + b, len) : leven_mw(q.peq, q.m, q.nw, a.data + b, len, st, 64);
    }
    return ham_words(a.words + (size_t)node * a.W, q.words, a.W);
}

// binary heaps of u64 keys (min-heap when MIN, else max-heap); h[0..n)
template <bool MIN>
__device__ __forceinline__ bool hbefore(u64 x, u64 y) { return MIN ? x < y : x > y; }
template <bool MIN>
__device__ void heap_push(u64* h, int& n, u64 v) {
    int i = n++;
    while (i > 0) {
        const int p = (i - 1) >> 1;
        if (!hbefore<MIN>(v, h[p])) break;
        h[i] = h[p];
        i = p;
    }
    h[i] = v;
}
template <bool MIN>
__device__ void heap_pop(u64* h, int& n) {
    const u64 v = h[--n];
    int i = 0;
    for (;;) {
        int c = 2 * i + 1;
        if (c >= n) break;
        if (c + 1 < n && hbefore<MIN>(h[c + 1], h[c])) ++c;
        if (!hbefore<MIN>(h[c], v)) break;
        h[i] = h[c];
        i = c;
    }
    if (n > 0) h[i] = v;
}

__device__ __forceinline__ u64 skey(int d, int node) { return ((u64)(uint32_t)d << 32) | (uint32_t)node; }

template <bool OLD>
__global__ __launch_bounds__(64) void string_hnsw_kernel(StringHnswArgs a, int q0, int nq) {
    const int qi = blockIdx.x;  // query of the slice
    if (qi >= nq) return;
    const int q = q0 + qi, lane = threadIdx.x;
    __shared__ int s_d[64];
    __shared__ int s_node, s_cnt, s_go, s_top;
    StrQ Q;
    if (a.space == SP_LEVEN) {
        Q.peq = a.peq + a.q_off[q];
        Q.m = a.q_len[q];
        Q.nw = (int)((a.q_off[q + 1] - a.q_off[q]) / 256);
        Q.words = nullptr;
    } else {
        Q.peq = nullptr;
        Q.m = Q.nw = 0;
        Q.words = a.q_words + (size_t)q * a.W;
    }
    u64* st = a.mw_ws + (size_t)qi * 64 * 2 * a.nw_max + lane;  // this lane's leven block state
    uint32_t* vis = a.visited + (size_t)qi * a.vis_words;
    u64* ws = a.ws + (size_t)qi * a.ws_per_query;
    int ndc = 0, hops = 0, hops_up = 0;

    // greedy descent (hnsw.cc:1090-1117): a list's distances are computed together, then taken in list order
    int cur = a.enterpoint;
    if (lane == 0) s_d[0] = str_dist(a, Q, cur, st);
    __syncthreads();
    int curdist = s_d[0];
    ndc = 1;
    for (int lvl = a.maxlevel; lvl > 0; --lvl) {
        bool changed = true;
        while (changed) {
            changed = false;
            const int32_t* L = a.up_links + a.up_off[cur] + (size_t)(lvl - 1) * (a.maxM + 1);
            const int cnt = L[0];
            ++hops_up;
            for (int c0 = 0; c0 < cnt; c0 += 64) {
                __syncthreads();
                if (c0 + lane < cnt) s_d[lane] = str_dist(a, Q, L[1 + c0 + lane], st);
                __syncthreads();
                const int m = min(64, cnt - c0);
                for (int j = 0; j < m; ++j)
                    if (s_d[j] < curdist) {
                        curdist = s_d[j];
                        cur = L[1 + c0 + j];
                        changed = true;
                    }
                ndc += m;
            }
        }
    }
    if (lane == 0) atomicOr(&vis[cur >> 5], 1u << (cur & 31));

    const int ef = a.ef, k = a.k;
    int nres = 0;
    u64* res_out;  // ascending keys of the result, nres of them
    if constexpr (!OLD) {
        // SortArrBI of capacity max(ef, k): keys ascending, used flags beside them
        const int cap = max(ef, k);
        u64* arr = ws;
        uint32_t* used = reinterpret_cast<uint32_t*>(ws + cap);
        u64* buf = ws + cap + (cap + 1) / 2;  // itemBuff: the accepted neighbours of one expansion
        int size = 1, curElem = 0;
        if (lane == 0) {
            arr[0] = skey(curdist, cur);
            used[0] = 0;
        }
        while (curElem < min(size, ef)) {
            __syncthreads();
            if (lane == 0) {
                used[curElem] = 1;
                s_node = (int)(uint32_t)arr[curElem];
                s_top = (int)(arr[size - 1] >> 32);
            }
            __syncthreads();
            ++curElem;
            ++hops;
            const int node = s_node, topKey = s_top;
            const int32_t* L = a.links0 + (size_t)node * (a.maxM0 + 1);
            const int cnt = L[0];
            int nitem = 0;
            for (int c0 = 0; c0 < cnt; c0 += 64) {
                int d = -1;
                if (c0 + lane < cnt) {
                    const int v = L[1 + c0 + lane];
                    const uint32_t bit = 1u << (v & 31);
                    if (!(atomicOr(&vis[v >> 5], bit) & bit)) d = str_dist(a, Q, v, st);
                }
                __syncthreads();
                s_d[lane] = d;
                __syncthreads();
                if (lane == 0) {
                    const int m = min(64, cnt - c0);
                    for (int j = 0; j < m; ++j) {
                        if (s_d[j] < 0) continue;
                        ++ndc;
                        if (s_d[j] < topKey || size < ef) buf[nitem++] = skey(s_d[j], L[1 + c0 + j]);
                    }
                }
            }
            if (lane == 0) {
                // sort the buffer, then insert each item (push_or_replace_non_empty_exp / merge_with_sorted_items: the
                // same array; the first insertion index is the smallest)
                for (int i = 1; i < nitem; ++i) {
                    const u64 v = buf[i];
                    int j = i - 1;
                    while (j >= 0 && buf[j] > v) {
                        buf[j + 1] = buf[j];
                        --j;
                    }
                    buf[j + 1] = v;
                }
                for (int i = 0; i < nitem; ++i) {
                    const u64 v = buf[i];
                    if (size == cap && v >= arr[size - 1]) continue;
                    int pos = size < cap ? size : size - 1;  // the last one is dropped when full
                    while (pos > 0 && arr[pos - 1] > v) {
                        arr[pos] = arr[pos - 1];
                        used[pos] = used[pos - 1];
                        --pos;
                    }
                    arr[pos] = v;
                    used[pos] = 0;
                    if (size < cap) ++size;
                    if (pos < curElem) curElem = pos;
                }
                while (curElem < size && used[curElem]) ++curElem;
                s_cnt = size;
                s_go = curElem;
            }
            __syncthreads();
            size = s_cnt;
            curElem = s_go;
        }
        nres = min(k, size);
        res_out = arr;
    } else {
        // candidateQueue (min-heap), closestDistQueue1 (max-heap, at most ef), the k-NN result (max-heap, at most k)
        u64* cand = ws;
        u64* closest = ws + a.n;
        u64* res = closest + ef + 2;
        int nc = 0, ncl = 0;
        if (lane == 0) {
            heap_push<true>(cand, nc, skey(curdist, cur));
            heap_push<false>(closest, ncl, skey(curdist, cur));
            heap_push<false>(res, nres, skey(curdist, cur));
        }
        for (;;) {
            __syncthreads();
            if (lane == 0) {
                s_go = 0;
                if (nc > 0 && cand[0] <= closest[0]) {  // the nearest candidate is not beyond the ef-th closest
                    s_go = 1;
                    s_node = (int)(uint32_t)cand[0];
                    heap_pop<true>(cand, nc);
                }
            }
            __syncthreads();
            if (!s_go) break;
            ++hops;
            const int node = s_node;
            const int32_t* L = a.links0 + (size_t)node * (a.maxM0 + 1);
            const int cnt = L[0];
            for (int c0 = 0; c0 < cnt; c0 += 64) {
                int d = -1;
                if (c0 + lane < cnt) {
                    const int v = L[1 + c0 + lane];
                    const uint32_t bit = 1u << (v & 31);
                    if (!(atomicOr(&vis[v >> 5], bit) & bit)) d = str_dist(a, Q, v, st);
                }
                __syncthreads();
                s_d[lane] = d;
                __syncthreads();
                if (lane == 0) {
                    const int m = min(64, cnt - c0);
                    for (int j = 0; j < m; ++j) {
                        if (s_d[j] < 0) continue;
                        ++ndc;
                        const u64 key = skey(s_d[j], L[1 + c0 + j]);
                        if (key < closest[0] || ncl < ef) {
                            if (nres < k) heap_push<false>(res, nres, key);
                            else if (key < res[0]) {
                                heap_pop<false>(res, nres);
                                heap_push<false>(res, nres, key);
                            }
                            heap_push<true>(cand, nc, key);
                            heap_push<false>(closest, ncl, key);
                            if (ncl > ef) heap_pop<false>(closest, ncl);
                        }
                    }
                }
            }
        }
        if (lane == 0) {  // the result heap, ascending
            int m = nres;
            while (m > 0) {
                const u64 top = res[0];
                heap_pop<false>(res, m);
                res[m] = top;
            }
            s_cnt = nres;  // the heaps live in lane 0: every lane takes the count from it
        }
        __syncthreads();
        nres = s_cnt;
        res_out = res;
    }
    __syncthreads();
    for (int i = lane; i < k; i += 64) {
        const bool ok = i < nres;
        const u64 key = ok ? res_out[i] : 0;
        a.out_ids[(size_t)q * k + i] = ok ? a.ext_ids[(uint32_t)key] : -1;
        a.out_d[(size_t)q * k + i] = ok ? (float)(uint32_t)(key >> 32) : INFINITY;
    }
    if (lane == 0) {
        a.out_cnt[q] = nres;
        a.ndc[q] = ndc;
        a.hops[q] = hops;
        a.hops_up[q] = hops_up;
    }
}

const u64* U(const uint64_t* p) { return reinterpret_cast<const u64*>(p); }
u64* UW(uint64_t* p) { return reinterpret_cast<u64*>(p); }

}  // namespace

size_t leven_mw_ws_words(const ScanPlan& p, int nw) {
    return nw > kStrMwLds ? (size_t)p.nsplit * ((p.nq + p.tq - 1) / p.tq) * 256 * 2 * nw : 0;
}

hipError_t launch_leven_knn(const ScanPlan& p, const int64_t* row_ptr, const uint8_t* data,
                            const int64_t* q_off, const int32_t* q_len, const uint64_t* peq, int nw, uint64_t* mw_ws,
                            float* split_d, int32_t* split_pos, hipStream_t s) {
    const dim3 grid(p.nsplit, (p.nq + p.tq - 1) / p.tq);
    size_t lds = (size_t)p.tq * p.P * 8 + kStrPeqStage + kStrRowStage;
    if (nw == 1 && p.tq == kStrTileQ)
        return launch_with_lds(leven_knn_kernel<kStrTileQ, false>, grid, lds, s, row_ptr, data, p.n, p.rows_per_split,
                               q_off, q_len, U(peq), p.nq, p.k, p.kl, p.P, nw, UW(mw_ws), split_d, split_pos);
    if (nw == 1)
        return launch_with_lds(leven_knn_kernel<1, false>, grid, lds, s, row_ptr, data, p.n, p.rows_per_split, q_off,
                               q_len, U(peq), p.nq, p.k, p.kl, p.P, nw, UW(mw_ws), split_d, split_pos);
    if (p.tq != 1) return hipErrorInvalidValue;
    if (nw <= kStrMwLds) lds += (size_t)256 * 2 * nw * 8;
    return launch_with_lds(leven_knn_kernel<1, true>, grid, lds, s, row_ptr, data, p.n, p.rows_per_split, q_off, q_len,
                           U(peq), p.nq, p.k, p.kl, p.P, nw, UW(mw_ws), split_d, split_pos);
}

hipError_t launch_ham_knn(const ScanPlan& p, const uint32_t* rows, int W, const uint32_t* q, float* split_d,
                          int32_t* split_pos, hipStream_t s) {
    const dim3 grid(p.nsplit, (p.nq + p.tq - 1) / p.tq);
    const size_t lds = (size_t)p.tq * p.P * 8 + kStrHamQStage;
    if (p.tq == kStrTileQ)
        return launch_with_lds(ham_knn_kernel<kStrTileQ>, grid, lds, s, rows, W, p.n, p.rows_per_split, q, p.nq, p.k,
                               p.kl, p.P, split_d, split_pos);
    return launch_with_lds(ham_knn_kernel<1>, grid, lds, s, rows, W, p.n, p.rows_per_split, q, p.nq, p.k, p.kl, p.P,
                           split_d, split_pos);
}

int leven_dist_grid(int n) {
    int grid = (n + 255) / 256;
    return std::max(1, std::min(grid, 4096));
}

hipError_t launch_leven_dist(const int64_t* row_ptr, const uint8_t* data, int n, const uint64_t* peq, int m, int nw,
                             uint64_t* mw_ws, float* d_out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(leven_dist_kernel, dim3(leven_dist_grid(n)), dim3(256), 0, s, row_ptr, data, n, U(peq), m, nw,
                       UW(mw_ws), d_out);
    return hipGetLastError();
}

hipError_t launch_ham_dist(const uint32_t* rows, int W, int n, const uint32_t* q, float* d_out, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    int grid = std::max(1, std::min((n + 255) / 256, 8192));
    hipLaunchKernelGGL(ham_dist_kernel, dim3(grid), dim3(256), 0, s, rows, W, n, q, d_out);
    return hipGetLastError();
}

hipError_t launch_leven_pair(const int64_t* row_ptr, const uint8_t* data, int p2, const uint64_t* peq, int m, int nw,
                             uint64_t* mw_ws, float* out, hipStream_t s) {
    hipLaunchKernelGGL(leven_pair_kernel, dim3(1), dim3(64), 0, s, row_ptr, data, p2, U(peq), m, nw, UW(mw_ws), out);
    return hipGetLastError();
}

size_t string_hnsw_ws_words(const StringHnswArgs& a, bool old) {
    const int cap = std::max(a.ef, a.k);
    const size_t maxl = (size_t)std::max(a.maxM, a.maxM0) + 1;
    return old ? (size_t)a.n + a.ef + 2 + a.k + 1 : (size_t)cap + (cap + 1) / 2 + maxl;
}

hipError_t launch_string_hnsw(const StringHnswArgs& a, bool old, int q0, int nq, hipStream_t s) {
    if (nq <= 0) return hipSuccess;
    if (old) hipLaunchKernelGGL(string_hnsw_kernel<true>, dim3(nq), dim3(64), 0, s, a, q0, nq);
    else hipLaunchKernelGGL(string_hnsw_kernel<false>, dim3(nq), dim3(64), 0, s, a, q0, nq);
    return hipGetLastError();
}

hipError_t launch_ham_pair(const uint32_t* rows, int W, int p1, int p2, float* out, hipStream_t s) {
    hipLaunchKernelGGL(ham_pair_kernel, dim3(1), dim3(64), 0, s, rows, W, p1, p2, out);
    return hipGetLastError();
}

}  // namespace gfxknn
