// l1 fast path of the dense brute force: a filter scan over an 8-bit copy of the rows with v_sad_u8
// (four dimensions per lane-instruction), the exact f32 re-rank of its survivors (launch_bf_rerank: the reference's
// formula on the original rows), a per-query proof that no row outside the lists can belong to the top k, and the adaptive
// VALU selection for the query tiles whose proof fails.  Quantisation and bound: ../l1_quant.hpp.
#include "../l1_quant.hpp"
#include "common_dev.hpp"
#include "split_topk_dev.hpp"

namespace gfxknn {

constexpr int L1_QW = 32;    // queries per wave: one SAD accumulator each per row of the lane
constexpr int L1_RB = 2;     // 64-row blocks per step: a lane owns L1_RB rows
constexpr int L1_P = 128;    // key buffer per query in LDS: up to 64 kept keys + one block's 64 offers
constexpr int L1_STEP = 64 * L1_RB;
typedef __attribute__((address_space(4))) uint32_t ConstU32;
static_assert(L1_STEP == BF_L1_ROW_TILE, "row padding of the copy");
static_assert(4 * L1_QW == BF_TQ, "a workgroup of four waves serves one query tile");

// ---- finalize: column ranges, the byte copy, the residuals -----------------------------------------------------------
// range [0, ld) smallest and [ld, 2 ld) largest element per column as ordered bits (f32_ord; cleared to ~0 / 0 by the
// caller), range[2 ld] != 0: a non-finite element
__global__ __launch_bounds__(256) void l1_col_range_kernel(const float* rows, int n, int ld, int dim, int rows_per_block,
                                                           uint32_t* range) {
    const int c = threadIdx.x % ld, sub = threadIdx.x / ld, nsub = 256 / ld;
    if (sub >= nsub || c >= dim) return;
    const int r0 = blockIdx.x * rows_per_block;
    const int r1 = r0 + rows_per_block < n ? r0 + rows_per_block : n;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u, bad = 0u;
    for (int r = r0 + sub; r < r1; r += nsub) {
        const float x = rows[(size_t)r * ld + c];
        bad |= (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u;
        const uint32_t o = f32_ord(x);
        lo = o < lo ? o : lo;
        hi = o > hi ? o : hi;
    }
    if (lo <= hi) {
        atomicMin(&range[c], lo);
        atomicMax(&range[ld + c], hi);
    }
    if (bad) atomicOr(&range[2 * ld], 1u);
}

// One thread per (64-row block, dword j, row of the block): four columns of a row become one dword of the copy,
// [n_pad / 64][d4][64]; columns past dim and rows past n are zero bytes.  rmax_bits [dim]: the largest residual per
// column, rounded up to f32 (non-negative floats order as their bits).
__global__ __launch_bounds__(256) void l1_quantise_rows_kernel(const float* rows, int n, int n_pad, int ld, int dim, int d4,
                                                               const float* lo, double s, uint32_t* out, uint32_t* rmax_bits) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t total = (size_t)n_pad * d4;
    if (idx >= total) return;   // (n_pad * d4 is a multiple of 64: whole waves leave together)
    const int lane = (int)(idx & 63);
    const size_t bj = idx >> 6;
    const int j = (int)(bj % d4);
    const int row = (int)(bj / d4) * 64 + lane;
    uint32_t word = 0;
    float res[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < n) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * j + e;
            if (c < dim) {
                const float x = rows[(size_t)row * ld + c];
                const uint8_t b = l1q::quantise(x, lo[c], s);
                word |= (uint32_t)b << (8 * e);
                res[e] = l1q::round_up_f32(l1q::residual(x, lo[c], s, b));
            }
        }
    }
    out[idx] = word;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float m = wave_max(res[e]);
        if (lane == 0 && 4 * j + e < dim) atomicMax(&rmax_bits[4 * j + e], __float_as_uint(m));
    }
}

// ---- per batch: the queries' bytes, excess and bound -------------------------------------------------------------------
// One thread per padded query: qt [d4][qpad] dwords (the wave of a scan reads the 32 dwords of its queries in column j
// as uniform values), xe [qpad][2] = X_q, E_q.  Padding queries are zero bytes.
__global__ __launch_bounds__(64) void l1_prep_queries_kernel(const float* raw, int nq, int qpad, int dim, int d4, const float* lo,
                                                             const float* hi, const float* rmax, double s, uint32_t* qt,
                                                             double* xe) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= qpad) return;
    double x = 0, e = 0;
    for (int j = 0; j < d4; ++j) {
        uint32_t word = 0;
        if (q < nq) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = 4 * j + i;
                if (c < dim) {
                    uint8_t b;
                    double xc, ec;
                    l1q::query(raw + (size_t)q * dim + c, lo + c, hi + c, rmax + c, 1, s, &b, &xc, &ec);
                    x += xc;
                    e += ec;
                    word |= (uint32_t)b << (8 * i);
                }
            }
        }
        qt[(size_t)j * qpad + q] = word;
    }
    xe[2 * (size_t)q] = x;
    xe[2 * (size_t)q + 1] = e * (1.0 + 2.2737367544323206e-13);   // (this sum's own rounding, as l1q::query covers its)
}

// ---- the scan ----------------------------------------------------------------------------------------------------------
struct BfL1ScanArgs {
    const uint32_t* rows;   // [n_pad / 64][d4][64]
    const uint32_t* qt;     // [d4][qpad]
    u64* cand;              // [qpad][nsplit][kprime]: (SAD << 32) | ~position, ascending (SAD, position)
    int* cand_cnt;          // [qpad][nsplit]
    int n, n_pad, d4, qpad, nsplit, rows_per_split, kprime;
};

// ascending bitonic sort of L1_P 32-bit keys in LDS by one wave (one pair per lane and stage)
__device__ __forceinline__ void wave_bitonic128_u32(uint32_t* s, int lane) {
    for (int k2 = 2; k2 <= L1_P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const int i = 2 * lane - (lane & (j - 1)), l = i + j;
            const uint32_t a = s[i], b = s[l];
            const bool up = (i & k2) == 0;
            if (up ? (a > b) : (a < b)) {
                s[i] = b;
                s[l] = a;
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

// keeps the kprime smallest of the cnt buffered keys of one query (sorted); the kprime-th becomes the threshold
__device__ __forceinline__ void l1_compact(uint32_t* keys, int* cnt, uint32_t* thr, int kprime, int lane) {
    const int c = *cnt;
    if (lane >= c) keys[lane] = 0xFFFFFFFFu;
    if (lane + 64 >= c) keys[lane + 64] = 0xFFFFFFFFu;
    __builtin_amdgcn_wave_barrier();
    wave_bitonic128_u32(keys, lane);
    if (c >= kprime) {
        const uint32_t t = keys[kprime - 1];
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            *thr = t;
            *cnt = kprime;
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// Grid: (row split, query tile of 128).  The four waves of a workgroup take 32 queries each and walk the same rows (the
// row dwords of the later waves come from cache).  A lane owns L1_RB rows per step and keeps one SAD per (row, query) in
// registers; per column dword j it loads its rows' dword and adds 32 SADs against the uniform query dwords.  Keys are
// (SAD << 16) | row within the split: a split has at most 65536 rows and a SAD is at most 255 * 256.  Per query the
// wave keeps the kprime smallest keys of the split in LDS under a running threshold; only the wave that owns a query
// touches its buffer, so the kernel has no barrier.
__global__ __launch_bounds__(256, 2) void bf_l1_scan_kernel(BfL1ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    uint32_t* keys = reinterpret_cast<uint32_t*>(smem) + (size_t)wave * L1_QW * L1_P;          // [L1_QW][L1_P]
    int* cnt = reinterpret_cast<int*>(smem + (size_t)4 * L1_QW * L1_P * 4) + wave * L1_QW;       // [L1_QW]
    uint32_t* thr = reinterpret_cast<uint32_t*>(smem + (size_t)4 * L1_QW * (L1_P + 1) * 4) + wave * L1_QW;
    const int split = blockIdx.x % a.nsplit, tile = blockIdx.x / a.nsplit;
    const int q0 = tile * BF_TQ + wave * L1_QW;
    // (the query dwords are uniform and never written here: read through the constant address space they come in by
    //  scalar loads and feed v_sad_u8 as its scalar operand)
    const ConstU32* qt = (const ConstU32*)(uintptr_t)(a.qt + q0);
    if (lane < L1_QW) {
        cnt[lane] = 0;
        thr[lane] = 0xFFFFFFFFu;
    }
    __builtin_amdgcn_wave_barrier();
    uint32_t thr_hi[L1_QW];   // SAD part of the thresholds (uniform): the check in the loop is one compare per query
#pragma unroll
    for (int t = 0; t < L1_QW; ++t) thr_hi[t] = 0xFFFFu;

    const int row0 = split * a.rows_per_split;
    const int row_end = row0 + a.rows_per_split < a.n_pad ? row0 + a.rows_per_split : a.n_pad;
    for (int r = row0; r < row_end; r += L1_STEP) {
        const uint32_t* __restrict__ rp = a.rows + (size_t)(r >> 6) * a.d4 * 64 + lane;
        uint32_t acc[L1_RB][L1_QW];
#pragma unroll
        for (int b = 0; b < L1_RB; ++b)
#pragma unroll
            for (int t = 0; t < L1_QW; ++t) acc[b][t] = 0;
        uint32_t next[L1_RB];   // the row dwords of column j + 1 are requested before column j is used
#pragma unroll
        for (int b = 0; b < L1_RB; ++b) next[b] = rp[(size_t)b * a.d4 * 64];
#pragma unroll 2
        for (int j = 0; j < a.d4; ++j) {
            uint32_t rowd[L1_RB];
            const int jn = j + 1 < a.d4 ? j + 1 : j;
#pragma unroll
            for (int b = 0; b < L1_RB; ++b) {
                rowd[b] = next[b];
                next[b] = rp[((size_t)b * a.d4 + jn) * 64];
            }
            const ConstU32* qj = qt + (size_t)j * a.qpad;
#pragma unroll
            for (int t = 0; t < L1_QW; ++t) {
                const uint32_t qv = qj[t];
#pragma unroll
                for (int b = 0; b < L1_RB; ++b) acc[b][t] = __builtin_amdgcn_sad_u8(rowd[b], qv, acc[b][t]);
            }
        }
        // offers, one row block at a time: a buffer holds at most 64 keys before a block and takes at most 64 from it
#pragma unroll
        for (int b = 0; b < L1_RB; ++b) {
            const int lrow = r - row0 + 64 * b + lane;
            const bool valid = row0 + lrow < a.n;   // (rows of the padding are never listed)
            uint32_t big = 0;
#pragma unroll
            for (int t = 0; t < L1_QW; ++t) {
                if (__builtin_amdgcn_ballot_w64(acc[b][t] <= thr_hi[t]) != 0) {
                    const uint32_t key = valid ? (acc[b][t] << 16) | (uint32_t)lrow : 0xFFFFFFFFu;
                    const bool in = key < thr[t];
                    const u64 m = __builtin_amdgcn_ballot_w64(in);
                    if (m != 0) {
                        const int c = cnt[t];
                        const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                        if (in) keys[t * L1_P + c + rank] = key;
                        const int cn = c + (int)__popcll(m);
                        __builtin_amdgcn_wave_barrier();
                        if (lane == 0) cnt[t] = cn;
                        if (cn > L1_P - 64) big |= 1u << t;
                    }
                }
            }
            big = __builtin_amdgcn_readfirstlane(big);
            if (big != 0) {
                __builtin_amdgcn_wave_barrier();
                for (uint32_t rest = big; rest != 0; rest &= rest - 1) {
                    const int t = __builtin_ctz(rest);
                    l1_compact(keys + t * L1_P, cnt + t, thr + t, a.kprime, lane);
                }
#pragma unroll
                for (int t = 0; t < L1_QW; ++t)
                    if ((big >> t) & 1u) thr_hi[t] = thr[t] >> 16;
            }
        }
    }
    // the lists: sorted, then out as the survivor keys the re-rank reads
    for (int t = 0; t < L1_QW; ++t) {
        __builtin_amdgcn_wave_barrier();
        const int c = cnt[t];
        __builtin_amdgcn_wave_barrier();
        l1_compact(keys + t * L1_P, cnt + t, thr + t, a.kprime, lane);
        const int kept = c < a.kprime ? c : a.kprime;
        const size_t o = (size_t)(q0 + t) * a.nsplit + split;
        for (int i = lane; i < kept; i += 64) {
            const uint32_t key = keys[t * L1_P + i];
            const uint32_t pos = (uint32_t)row0 + (key & 0xFFFFu);
            a.cand[o * a.kprime + i] = ((u64)(key >> 16) << 32) | (u64)(0xFFFFFFFFu - pos);
        }
        if (lane == 0) a.cand_cnt[o] = kept;
    }
}

// ---- the proof -----------------------------------------------------------------------------------------------------------
// One thread per query, after the exact re-rank.  d_k: the k-th exact distance.  A split whose list is full left rows out;
// each of them has a SAD of at least the list's largest, m, so its exact f32 distance is at least
// l1q::filter_floor(X_q, E_q, s, m).  The answer is proven when that is strictly above d_k for every full split (a split
// that is not full left nothing out).  Anything else -- fewer than k survivors, a NaN in the bound -- flags the query's
// tile for the adaptive selection.
__global__ __launch_bounds__(64) void bf_l1_verify_kernel(const u64* cand, const int* cand_cnt, const double* xe, double s,
                                                          const float* out_dists, int nq, int k, int nsplit, int kprime,
                                                          int* flags) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nq) return;
    const float dk = out_dists[(size_t)q * k + k - 1];
    const double X = xe[2 * (size_t)q], E = xe[2 * (size_t)q + 1];
    bool ok = dk < INFINITY;   // (k results were found)
    for (int sp = 0; sp < nsplit && ok; ++sp) {
        const size_t o = (size_t)q * nsplit + sp;
        if (cand_cnt[o] < kprime) continue;
        const uint32_t m = (uint32_t)(cand[o * kprime + kprime - 1] >> 32);
        ok = l1q::filter_floor(X, E, s, m) > (double)dk;
    }
    if (!ok) atomicOr(&flags[q / BF_TQ], 1);
}

// ---- host side -------------------------------------------------------------------------------------------------------------
BfL1Fast bf_l1_fast_plan(int n, int dim, int nq, int k) {
    BfL1Fast f{};
    f.use = false;
    if (n < 65536 || nq < 256 || dim < 1 || dim > BF_L1_MAX_DIM || k < 1 || k > 128) return f;
    // lists: 32 keys per (query, split), 64 for k above 24 -- room for the rows inside the error band of the k-th
    // distance, a few dozen per query over ALL splits on ordinary data, several times over
    f.kprime = k <= 24 ? 32 : 64;
    // 64 splits fill the chip at 1024 queries (8 query tiles); a split holds at most 65536 rows (16-bit row field)
    f.nsplit = 64;
    if ((long long)f.nsplit * 65536 < n) f.nsplit = (int)(((long long)n + 65535) / 65536);
    if (f.nsplit * f.kprime > 8192) return f;   // (the re-rank sorts a query's survivors in LDS)
    const int rps = (n + f.nsplit - 1) / f.nsplit;
    f.rows_per_split = (rps + BF_L1_ROW_TILE - 1) / BF_L1_ROW_TILE * BF_L1_ROW_TILE;
    f.d4 = (dim + 3) / 4;
    f.qpad = (nq + BF_TQ - 1) / BF_TQ * BF_TQ;
    f.nqt = f.qpad / BF_TQ;
    f.fallback = bf_make_plan(n, dim, nq, k, false);
    // the lists in the shape launch_bf_rerank reads
    f.list = f.fallback;
    f.list.nsplit = f.nsplit;
    f.list.rows_per_split = f.rows_per_split;
    f.list.kprime = f.kprime;
    f.list.cap = f.kprime;
    int p2 = 1;
    while (p2 < f.nsplit * f.kprime) p2 <<= 1;
    f.list.p2max = p2;
    f.list.lds_rerank = (size_t)p2 * 8 + (f.nsplit + 1) * 4 + 16;
    f.lds_scan = (size_t)4 * L1_QW * (L1_P + 2) * 4;
    f.use = true;
    return f;
}

hipError_t launch_l1_col_range(const float* rows, int n, int ld, int dim, uint32_t* range, hipStream_t s) {
    if (ld > 256) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(range, 0xFF, (size_t)ld * 4, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(range + ld, 0, ((size_t)ld + 1) * 4, s);
    if (e != hipSuccess) return e;
    const int rows_per_block = 2048;
    hipLaunchKernelGGL(l1_col_range_kernel, dim3((n + rows_per_block - 1) / rows_per_block), dim3(256), 0, s, rows, n, ld, dim,
                       rows_per_block, range);
    return hipGetLastError();
}

hipError_t launch_l1_quantise_rows(const float* rows, int n, int ld, int dim, const float* lo, double step, uint32_t* out,
                                   uint32_t* rmax_bits, hipStream_t s) {
    const int d4 = (dim + 3) / 4, n_pad = bf_l1_rows_padded(n);
    hipError_t e = hipMemsetAsync(rmax_bits, 0, (size_t)dim * 4, s);
    if (e != hipSuccess) return e;
    const size_t total = (size_t)n_pad * d4;
    hipLaunchKernelGGL(l1_quantise_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, rows, n, n_pad, ld, dim, d4,
                       lo, step, out, rmax_bits);
    return hipGetLastError();
}

hipError_t launch_bf_l1_fast(const BfL1Fast& f, int nq, int k, const BfF32Rows& rows, const BfL1Rows& copy, const float* queries_raw,
                             float* queries_padded, const BfL1Ws& ws, const BfOut& out, const BfScanEvents& ev, hipStream_t s) {
    hipError_t e = hipMemsetAsync(ws.flags, 0, (size_t)f.nqt * 4, s);
    if (e != hipSuccess) return e;
    e = launch_pad_rows(queries_raw, nq, rows.dim, queries_padded, f.qpad, rows.ldb, 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(l1_prep_queries_kernel, dim3(f.qpad / 64), dim3(64), 0, s, queries_raw, nq, f.qpad, rows.dim, f.d4, copy.lo,
                       copy.hi, copy.rmax, copy.step, ws.qt, ws.xe);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    BfL1ScanArgs a{};
    a.rows = copy.u8;
    a.qt = ws.qt;
    a.cand = ws.cand.cand;
    a.cand_cnt = ws.cand.cnt;
    a.n = rows.n;
    a.n_pad = bf_l1_rows_padded(rows.n);
    a.d4 = f.d4;
    a.qpad = f.qpad;
    a.nsplit = f.nsplit;
    a.rows_per_split = f.rows_per_split;
    a.kprime = f.kprime;
    if (ev.first) (void)hipEventRecord(ev.first, s);
    e = launch_with_lds(bf_l1_scan_kernel, dim3(f.nsplit * f.nqt), f.lds_scan, s, a);
    if (ev.second) (void)hipEventRecord(ev.second, s);
    if (e != hipSuccess) return e;
    e = launch_bf_rerank(f.list, SP_L1, rows.dim, k, rows.orig, queries_padded, ws.cand, BfGate{}, BfVerify{}, out, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(bf_l1_verify_kernel, dim3((nq + 63) / 64), dim3(64), 0, s, ws.cand.cand, ws.cand.cnt, ws.xe, copy.step,
                       out.dists, nq, k, f.nsplit, f.kprime, ws.flags);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    // tiles without a proof: the adaptive VALU selection and its re-rank, as without the fast path
    const BfGate failed{ws.flags, 1};
    e = launch_bf_select_direct_f32(f.fallback, SP_L1, rows.orig, queries_padded, ws.fb, failed, s);
    if (e != hipSuccess) return e;
    return launch_bf_rerank(f.fallback, SP_L1, rows.dim, k, rows.orig, queries_padded, ws.fb, failed, BfVerify{}, out, s);
}

}  // namespace gfxknn
