// Fast path of the exact scan over kldivfast, kldivfastrq, kldivgenfast, kldivgenfastrq and itakurasaitofast (DESIGN.md
// 4.11a): these divergences are sign * (a . b) + R_row + C_query, so a filter scan takes the inner product on the bf16
// matrix cores (operands split hi + lo, three v_mfma_f32_32x32x16_bf16 per 16 columns), the exact scan's own formula
// (diverg_dev.hpp) re-ranks the rows it lists, and a per-query proof shows that no unlisted row can belong to the top k.
// Queries without a proof flag their 16-query group; the host runs those through the exact scan.  Operands, constants
// and the bound: ../diverg_filter.hpp.
// This file is compiled with diverg_kernels.hip's flags (-ffp-contract=off: the re-rank's bits are the exact scan's).
#include "kernels.hpp"
#include "diverg_dev.hpp"
#include "split_topk_dev.hpp"   // launch_with_lds

namespace gfxknn {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
using dvf::kBuf;
using dvf::kKeep;

// ---- per batch: the queries' operand, split, with C_q and E_q ----------------------------------------------------------
// One thread per padded query; padding queries are zeros without a proof.
__global__ __launch_bounds__(64) void diverg_fast_prep_kernel(int form, const float* qv, const float* ql, const float* qi,
                                                              int qstride, int nq, int qpad, int dim, int dpad, dvf::RowMax m,
                                                              uint16_t* qsplit, double* ce) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= qpad) return;
    uint16_t* hi = qsplit + (size_t)q * 2 * dpad;
    uint16_t* lo = hi + dpad;
    double C = 0, E = INFINITY;
    if (q < nq) {
        dvf::query(form, qv + (size_t)q * 4, ql + (size_t)q * 4, qi ? qi + (size_t)q * 4 : nullptr, (size_t)qstride * 4,
                   (size_t)dim, (size_t)dpad, m, hi, lo, &C, &E);
    } else {
        for (int j = 0; j < dpad; ++j) hi[j] = lo[j] = 0;
    }
    ce[2 * (size_t)q] = C;
    ce[2 * (size_t)q + 1] = E;
}

// ---- the scan ----------------------------------------------------------------------------------------------------------
struct DivergScanArgs {
    const bf16x8* frags;    // [nblocks][ksteps][2][64]
    const float* rrow;      // [nblocks * 32]
    const uint16_t* qsplit; // [qpad][2][dpad]
    u64* cand;              // [qpad][nsplit][kKeep]
    int* cand_cnt;          // [qpad][nsplit]
    int n, nblocks, ksteps, dpad, nsplit, blocks_per_split;
    float sign;
};

// keeps the kKeep smallest of the cnt buffered keys of one query (sorted); the kKeep-th becomes the threshold
__device__ __forceinline__ void diverg_compact(u64* keys, int* cnt, u64* thr, int lane) {
    const int c = *cnt;
    for (int i = lane; i < kBuf; i += 64)
        if (i >= c) keys[i] = ~0ull;
    __builtin_amdgcn_wave_barrier();
    wave_bitonic_u64(keys, kBuf, lane, false);
    if (c >= kKeep) {
        const u64 t = keys[kKeep - 1];
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
            *thr = t;
            *cnt = kKeep;
        }
    }
    __builtin_amdgcn_wave_barrier();
}

// one 32-row block as a wave holds it: hi | lo A-fragments of every K-step and the R_row of the lane's 16 accumulator rows
template <int MAXKS>
struct DivergBlock {
    bf16x8 f[2 * MAXKS];
    f32x4 r[4];
};

// Grid: (row split, tile of 128 queries).  The four waves of a workgroup take 32 queries each and walk the same 32-row
// blocks (the later waves' fragments come from cache).  A wave keeps the hi and lo B-fragments of its queries for the whole K
// range in registers (2 * ksteps * 4 registers; MAXKS = 4, 8 or 16 K-steps per instantiation), loads a block's A-fragments
// as pre-tiled 16-byte-per-lane requests one block ahead, and issues three MFMAs per K-step into one 32x32 accumulator:
// lane (j = lane % 32, h = lane / 32) then holds rows 8 g + 4 h + i (register 4 g + i) of query j.  key = sign * acc +
// R_row; one compare against the query's threshold; the rare hit goes out of line.  Keys ((ordered key << 32) | row in the
// split) are appended to a kBuf-key LDS buffer owned by the query's wave; a buffer that the next block could overflow is
// sorted by that wave and cut to the kKeep smallest, the largest of which becomes the threshold.  Only the wave that owns
// a query touches its buffer: the kernel has no barrier.  No load sits under a divergent branch (a block index past the
// split is clamped, not skipped).
template <int MAXKS>
__global__ __launch_bounds__(256) void diverg_mfma_scan_kernel(DivergScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int h = lane >> 5, l31 = lane & 31;
    u64* keys = reinterpret_cast<u64*>(smem) + (size_t)wave * 32 * kBuf;                              // [32][kBuf]
    u64* thr = reinterpret_cast<u64*>(smem + (size_t)4 * 32 * kBuf * 8) + wave * 32;                   // [32]
    int* cnt = reinterpret_cast<int*>(smem + (size_t)4 * 32 * (kBuf + 1) * 8) + wave * 32;             // [32]
    const int split = blockIdx.x % a.nsplit, tile = blockIdx.x / a.nsplit;
    const int q0 = (tile * 4 + wave) * 32;
    const int ks = a.ksteps;

    bf16x8 bh[MAXKS], bl[MAXKS];
    {
        const uint16_t* qp = a.qsplit + (size_t)(q0 + l31) * 2 * a.dpad + 8 * h;
#pragma unroll
        for (int kc = 0; kc < MAXKS; ++kc) {
            const int kk = kc < ks ? kc : 0;   // (a K-step past the range is never multiplied)
            bh[kc] = *reinterpret_cast<const bf16x8*>(qp + 16 * kk);
            bl[kc] = *reinterpret_cast<const bf16x8*>(qp + a.dpad + 16 * kk);
        }
    }
    if (lane < 32) {
        cnt[lane] = 0;
        thr[lane] = ~0ull;
    }
    __builtin_amdgcn_wave_barrier();
    u64 thr64 = ~0ull;          // the threshold of query l31
    float thr_f = INFINITY;     // its key part: the check in the loop is one compare per accumulator

    const int blk0 = split * a.blocks_per_split;
    const int blk1 = blk0 + a.blocks_per_split < a.nblocks ? blk0 + a.blocks_per_split : a.nblocks;

    auto load = [&](int blk, DivergBlock<MAXKS>& d) __attribute__((always_inline)) {
        const int b = blk < a.nblocks ? blk : a.nblocks - 1;
        const bf16x8* fp = a.frags + (size_t)b * ks * 2 * 64 + lane;
#pragma unroll
        for (int kc = 0; kc < MAXKS; ++kc) {
            const int kk = kc < ks ? kc : 0;
            d.f[2 * kc] = fp[(size_t)(2 * kk) * 64];
            d.f[2 * kc + 1] = fp[(size_t)(2 * kk + 1) * 64];
        }
        const f32x4* rp = reinterpret_cast<const f32x4*>(a.rrow + (size_t)b * 32 + 4 * h);
#pragma unroll
        for (int g = 0; g < 4; ++g) d.r[g] = rp[2 * g];
    };
    auto process = [&](int blk, const DivergBlock<MAXKS>& d) __attribute__((always_inline)) {
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.f;
#pragma unroll
        for (int kc = 0; kc < MAXKS; ++kc) {
            if (kc < ks) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d.f[2 * kc], bh[kc], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d.f[2 * kc], bl[kc], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(d.f[2 * kc + 1], bh[kc], acc, 0, 0, 0);
            }
        }
        float key[16];
        bool any = false;
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            key[v] = fmaf(a.sign, acc[v], d.r[v >> 2][v & 3]);
            any = any || key[v] <= thr_f;
        }
        if (__builtin_amdgcn_ballot_w64(any) != 0) {
            const int lrow0 = (blk - blk0) * 32 + 4 * h, grow0 = blk * 32 + 4 * h;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int o = 8 * (v >> 2) + (v & 3);
                const u64 k64 = ((u64)f32_ord(key[v]) << 32) | (uint32_t)(lrow0 + o);
                // (rows of the padding are never listed; the two lanes of a query take their places by an LDS atomic)
                if (grow0 + o < a.n && k64 < thr64) keys[l31 * kBuf + atomicAdd(&cnt[l31], 1)] = k64;
            }
            __builtin_amdgcn_wave_barrier();
            // a buffer holds at most kBuf - 32 keys before a block and takes at most 32 from it
            uint32_t big = (uint32_t)__builtin_amdgcn_ballot_w64(cnt[l31] > kBuf - 32);
            if (big != 0) {
                for (uint32_t rest = big; rest != 0; rest &= rest - 1) {
                    const int t = __builtin_ctz(rest);
                    diverg_compact(keys + t * kBuf, cnt + t, thr + t, lane);
                }
                thr64 = thr[l31];
                thr_f = thr64 == ~0ull ? INFINITY : ord_f32((uint32_t)(thr64 >> 32));
            }
        }
    };

    DivergBlock<MAXKS> d0, d1;
    load(blk0, d0);
    for (int blk = blk0; blk < blk1; blk += 2) {
        load(blk + 1, d1);
        process(blk, d0);
        load(blk + 2, d0);
        if (blk + 1 < blk1) process(blk + 1, d1);
    }

    // the lists: sorted, then out with the rows' positions
    for (int t = 0; t < 32; ++t) {
        __builtin_amdgcn_wave_barrier();
        const int c = cnt[t];
        __builtin_amdgcn_wave_barrier();
        diverg_compact(keys + t * kBuf, cnt + t, thr + t, lane);
        const int kept = c < kKeep ? c : kKeep;
        const size_t o = (size_t)(q0 + t) * a.nsplit + split;
        if (lane < kept) a.cand[o * kKeep + lane] = keys[t * kBuf + lane] + (u64)((uint32_t)blk0 * 32u);
        if (lane == 0) a.cand_cnt[o] = kept;
    }
}

// ---- the re-rank -------------------------------------------------------------------------------------------------------
// One workgroup per query: the exact distance of every listed row with the exact scan's device function, ordered by
// (distance, position) in LDS, the first k out as the exact scan's merge writes them.
template <int F, bool REV>
__global__ __launch_bounds__(256) void diverg_fast_rerank_kernel(const f32x4* rv, const f32x4* rl, int D, int G, const f32x4* qv,
                                                                 const f32x4* ql, int qstride, const u64* cand,
                                                                 const int* cand_cnt, int nsplit, int k, int metr,
                                                                 const int32_t* ext_ids, float* out_d, int32_t* out_ids,
                                                                 int32_t* out_cnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    u64* keys = reinterpret_cast<u64*>(smem);
    __shared__ int s_total;
    const int q = blockIdx.x, tid = threadIdx.x;
    const int slots = nsplit * kKeep, P = next_pow2(slots);
    if (tid == 0) s_total = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < P; i += 256) {
        u64 key = ~0ull;
        const int sp = i / kKeep, j = i - sp * kKeep;
        if (i < slots && j < cand_cnt[(size_t)q * nsplit + sp]) {
            const uint32_t pos = (uint32_t)cand[((size_t)q * nsplit + sp) * kKeep + j];
            const size_t ro = (size_t)(pos >> 6) * G * 64 + (pos & 63);
            const float d = REV ? diverg_eval<F>(D, qv + q, ql + q, (size_t)qstride, rv + ro, rl + ro, 64, metr)
                                : diverg_eval<F>(D, rv + ro, rl + ro, 64, qv + q, ql + q, (size_t)qstride, metr);
            // -0 and +0 are one distance, as in the exact scan
            key = ((u64)f32_ord(d == 0.0f ? 0.0f : d) << 32) | pos;
            ++mine;
        }
        keys[i] = key;
    }
    if (mine) atomicAdd(&s_total, mine);
    __syncthreads();
    block_bitonic_u64_asc(keys, P, tid, 256);
    const int total = s_total, found = total < k ? total : k;
    for (int i = tid; i < k; i += 256) {
        int32_t id = -1;
        float d = INFINITY;
        if (i < found) {
            const u64 key = keys[i];
            id = ext_ids[(uint32_t)key];
            d = ord_f32((uint32_t)(key >> 32));
        }
        out_ids[(size_t)q * k + i] = id;
        out_d[(size_t)q * k + i] = d;
    }
    if (tid == 0) out_cnt[q] = found;
}

// ---- the proof -----------------------------------------------------------------------------------------------------------
// One thread per query, after the re-rank.  d_k: the k-th exact distance.  A split whose list is full left rows out, each with
// a filter key of at least the list's largest, key_m, so its exact f32 distance is at least dvf::filter_floor(key_m, C_q,
// E_q).  The answer is proven when that is strictly above d_k for every full split (a split that is not full left
// nothing out).  Anything else -- fewer than k results, a bound that is not finite -- flags the query's group.
// metr (jsmetr*): the floor goes through the distance's clamp and square root first (djs::proof_floor).
__global__ __launch_bounds__(64) void diverg_fast_verify_kernel(const u64* cand, const int* cand_cnt, const double* ce,
                                                                const float* out_d, int nq, int k, int nsplit, int metr,
                                                                int* flags) {
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nq) return;
    const float dk = out_d[(size_t)q * k + k - 1];
    const double C = ce[2 * (size_t)q], E = ce[2 * (size_t)q + 1];
    bool ok = dk < INFINITY && E < INFINITY;   // (k results were found; false for a NaN on either side)
    for (int sp = 0; sp < nsplit && ok; ++sp) {
        const size_t o = (size_t)q * nsplit + sp;
        if (cand_cnt[o] < kKeep) continue;
        const float key_m = ord_f32((uint32_t)(cand[o * kKeep + kKeep - 1] >> 32));
        ok = djs::proof_floor(key_m, C, E, metr) > (double)dk;
    }
    if (!ok) atomicOr(&flags[q / dvf::kGroup], 1);
}

__global__ void diverg_fast_clear_kernel(int* flags, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n) flags[i] = 0;
}

inline const f32x4* v4(const float* p) { return reinterpret_cast<const f32x4*>(p); }

template <int F, bool REV>
hipError_t launch_rerank(const dvf::Plan& p, int nq, int k, int metr, const DivergRows& rows, const DivergQueries& q,
                         const DivergFastWs& ws, const int32_t* ext_ids, float* out_d, int32_t* out_ids, int32_t* out_cnt,
                         hipStream_t s) {
    int P = 1;
    while (P < p.nsplit * kKeep) P <<= 1;
    hipLaunchKernelGGL((diverg_fast_rerank_kernel<F, REV>), dim3(nq), dim3(256), (size_t)P * 8, s, v4(rows.vals), v4(rows.logs),
                       rows.D, rows.G, v4(q.vals), v4(q.logs), q.stride, ws.cand, ws.cand_cnt, p.nsplit, k, metr, ext_ids, out_d,
                       out_ids, out_cnt);
    return hipGetLastError();
}

}  // namespace

int diverg_fast_form(int space) {
    switch (space) {
        case SP_KLDIV: return dvf::KL;
        case SP_KLDIV_RQ: return dvf::KL_RQ;
        case SP_KLDIVGEN: return dvf::KLGEN;
        case SP_KLDIVGEN_RQ: return dvf::KLGEN_RQ;
        case SP_ITAKURASAITO: return dvf::IS;
        default: return -1;
    }
}

hipError_t launch_diverg_fast(int space, const dvf::Plan& p, int nq, int k, const DivergRows& rows,
                              const DivergFastRows& copy, const DivergQueries& q, const DivergFastWs& ws,
                              const int32_t* ext_ids, float* out_d, int32_t* out_ids, int32_t* out_cnt, hipStream_t s) {
    const int form = diverg_fast_form(space);
    if (form < 0 || !p.use || nq <= 0) return hipErrorInvalidValue;
    const int dpad = 16 * p.ksteps;
    hipLaunchKernelGGL(diverg_fast_clear_kernel, dim3((p.ngroups + 63) / 64), dim3(64), 0, s, ws.flags, p.ngroups);
    hipLaunchKernelGGL(diverg_fast_prep_kernel, dim3(p.qpad / 64), dim3(64), 0, s, form, q.vals, q.logs, q.inv, q.stride, nq,
                       p.qpad, rows.D, dpad, copy.max, ws.qsplit, ws.ce);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    DivergScanArgs a{};
    a.frags = reinterpret_cast<const bf16x8*>(copy.frags);
    a.rrow = copy.rrow;
    a.qsplit = ws.qsplit;
    a.cand = ws.cand;
    a.cand_cnt = ws.cand_cnt;
    a.n = rows.n;
    a.nblocks = p.nblocks;
    a.ksteps = p.ksteps;
    a.dpad = dpad;
    a.nsplit = p.nsplit;
    a.blocks_per_split = p.rows_per_split / dvf::kRowBlock;
    a.sign = (float)dvf::sign_of(form);
    const dim3 grid((unsigned)(p.nsplit * p.nqt));
    const size_t lds = diverg_fast_scan_lds();
    if (p.ksteps_max == 4) e = launch_with_lds(diverg_mfma_scan_kernel<4>, grid, lds, s, a);
    else if (p.ksteps_max == 8) e = launch_with_lds(diverg_mfma_scan_kernel<8>, grid, lds, s, a);
    else e = launch_with_lds(diverg_mfma_scan_kernel<16>, grid, lds, s, a);
    if (e != hipSuccess) return e;
    return launch_diverg_fast_rerank_verify(space, p, nq, k, rows, q, ws, ext_ids, out_d, out_ids, out_cnt, s);
}

hipError_t launch_diverg_fast_rerank_verify(int space, const dvf::Plan& p, int nq, int k, const DivergRows& rows,
                                            const DivergQueries& q, const DivergFastWs& ws, const int32_t* ext_ids,
                                            float* out_d, int32_t* out_ids, int32_t* out_cnt, hipStream_t s) {
    const int metr = space == SP_JSMETR || space == SP_JSMETR_SLOW;
    hipError_t e;
    switch (diverg_fast_form(space)) {
        case dvf::KL: e = launch_rerank<DV_KL, false>(p, nq, k, 0, rows, q, ws, ext_ids, out_d, out_ids, out_cnt, s); break;
        case dvf::KL_RQ: e = launch_rerank<DV_KL, true>(p, nq, k, 0, rows, q, ws, ext_ids, out_d, out_ids, out_cnt, s); break;
        case dvf::KLGEN: e = launch_rerank<DV_KLGEN, false>(p, nq, k, 0, rows, q, ws, ext_ids, out_d, out_ids, out_cnt, s); break;
        case dvf::KLGEN_RQ: e = launch_rerank<DV_KLGEN, true>(p, nq, k, 0, rows, q, ws, ext_ids, out_d, out_ids, out_cnt, s); break;
        case dvf::IS: e = launch_rerank<DV_IS, false>(p, nq, k, 0, rows, q, ws, ext_ids, out_d, out_ids, out_cnt, s); break;
        default:
            if (!diverg_js_space(space)) return hipErrorInvalidValue;
            e = launch_rerank<DV_JS, false>(p, nq, k, metr, rows, q, ws, ext_ids, out_d, out_ids, out_cnt, s);
            break;
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(diverg_fast_verify_kernel, dim3((nq + 63) / 64), dim3(64), 0, s, ws.cand, ws.cand_cnt, ws.ce, out_d, nq,
                       k, p.nsplit, metr, ws.flags);
    return hipGetLastError();
}

}  // namespace gfxknn
