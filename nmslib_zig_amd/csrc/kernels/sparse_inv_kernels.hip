// Inverted-file filter for k-NN over the sparse inner-product spaces (negdotprod_sparse, querynorm_negdotprod_sparse,
// cosinesimil_sparse, angulardist_sparse), with an exact re-rank and a per-query proof (DESIGN.md 4.9a,
// ../sparse_filter.hpp).  The answers are the exact scan's (sparse_kernels.hip), byte for byte: the filter only decides
// which rows the scan's own formula (sparse_pair, sparse_dev.hpp) is evaluated on, and a query whose proof fails is
// flagged and redone by the scan.
//
//   sparse_inv_accum_kernel  : grid = (row block, query), block-major, so the workgroups in flight share one block's
//       postings in L2.  The workgroup owns one f32 accumulator per row of the block in LDS (64 KiB; with the 12 KiB of
//       term staging two workgroups fit a CU).  Per round of kTermChunk query terms: one lane per term bisects the block's
//       term list and stages (segment start, length, query value); then the segments are streamed one at a time by all
//       four waves -- two coalesced streams, row-in-block u16 and value f32 -- as  acc[row] = fma(q_t, b', acc[row]).
//       Rows inside a segment are distinct, so this is a plain LDS read-modify-write, no atomics; consecutive segments can
//       hold the same row, so a barrier separates them (absent terms cost a broadcast read and no barrier).  A row's
//       chain therefore runs in the query's term order: the score is deterministic.
//       Then one pass over the accumulators keeps the K' = k + 8 largest by (score descending, row ascending) with
//       SplitTopK on the order-preserving key of -score (one key for -0 and +0); untouched rows take part with their 0.
//       The block's K'-th score is its threshold T_block (-inf when the block listed all of its rows).
//   sparse_inv_rerank_kernel : one workgroup per query.  sparse_pair<SP>(row, query) for every kept row, the argument
//       order and the zero rule of the scan; the k best by (distance, position) through SplitTopK; positions to external
//       ids; then the proof: with T = max over blocks of T_block, the query is proved when its k-th distance is strictly
//       below spf::floor_dist(T).  Otherwise its flag is set.
// Compiled like sparse_kernels.hip (-ffp-contract=off); the filter's FMAs are explicit.
#include "kernels.hpp"
#include "sparse_dev.hpp"
#include "split_topk_dev.hpp"

namespace gfxknn {

namespace {

constexpr int kB = spf::kBlockRows, kChunk = spf::kTermChunk;
constexpr int kSelP = 512;   // SplitTopK's buffer: a power of two >= K' + 256 (K' <= 136) and >= k + 256
static_assert(kSelP >= spf::kMaxK + spf::kKeepExtra + 256, "the key buffer holds a chunk's offers above the kept keys");
static_assert(kSelP * 8 <= kChunk * 12, "the key buffer reuses the term staging");
static_assert(kB <= 65536, "a posting's row is 16 bits");

__global__ __launch_bounds__(256) void sparse_inv_accum_kernel(SparseInvFile f, const int64_t* __restrict__ q_ptr,
                                                               const uint32_t* __restrict__ q_ids,
                                                               const float* __restrict__ q_vals, int nq, int keep,
                                                               int32_t* __restrict__ cand, float* __restrict__ tblock) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_cnt[1];
    float* acc = reinterpret_cast<float*>(smem);               // [kB]
    float* sval = acc + kB;                                    // [kChunk] the round's query values
    uint32_t* sstart = reinterpret_cast<uint32_t*>(sval + kChunk);
    uint32_t* slen = sstart + kChunk;
    const int tid = threadIdx.x;
    const int b = blockIdx.x / nq, q = blockIdx.x - b * nq;
    const int rows = min(kB, f.n - b * kB);
    f32x4* a4 = reinterpret_cast<f32x4*>(acc);
    for (int i = tid; i < kB / 4; i += 256) a4[i] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int64_t t0 = f.blk_term[b];
    const int nt = (int)(f.blk_term[b + 1] - t0);
    const uint32_t* __restrict__ terms = f.terms + t0;
    const uint32_t* __restrict__ seg = f.seg + t0 + b;
    const int64_t p0 = f.blk_post[b];
    const uint16_t* __restrict__ prow = f.post_row + p0;
    const float* __restrict__ pval = f.post_val + p0;
    const int64_t qb = q_ptr[q];
    const int m = (int)(q_ptr[q + 1] - qb);
    for (int c0 = 0; c0 < m; c0 += kChunk) {
        const int cn = min(kChunk, m - c0);
        __syncthreads();   // (the zeroing; the round before has read its staging)
        for (int i = tid; i < cn; i += 256) {
            const uint32_t id = q_ids[qb + c0 + i];
            int lo = 0, hi = nt;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (terms[mid] < id) lo = mid + 1; else hi = mid;
            }
            const bool hit = lo < nt && terms[lo] == id;
            const uint32_t s = hit ? seg[lo] : 0u;
            sstart[i] = s;
            slen[i] = hit ? seg[lo + 1] - s : 0u;
            sval[i] = q_vals[qb + c0 + i];
        }
        __syncthreads();
        for (int t = 0; t < cn; ++t) {
            const uint32_t len = slen[t];
            if (len == 0) continue;   // (the same for every thread)
            const uint32_t s = sstart[t];
            const float qv = sval[t];
            uint32_t i = tid;
            for (; i + 768 < len; i += 1024) {   // a long segment: four postings per thread in flight
                const int r0 = prow[s + i], r1 = prow[s + i + 256], r2 = prow[s + i + 512], r3 = prow[s + i + 768];
                const float v0 = pval[s + i], v1 = pval[s + i + 256], v2 = pval[s + i + 512], v3 = pval[s + i + 768];
                acc[r0] = fmaf(qv, v0, acc[r0]);
                acc[r1] = fmaf(qv, v1, acc[r1]);
                acc[r2] = fmaf(qv, v2, acc[r2]);
                acc[r3] = fmaf(qv, v3, acc[r3]);
            }
            for (; i < len; i += 256) {
                const int r = prow[s + i];
                acc[r] = fmaf(qv, pval[s + i], acc[r]);
            }
            __syncthreads();   // the next segment can hold the same rows
        }
    }
    __syncthreads();

    SplitTopK<1> sel{reinterpret_cast<u64*>(sval), s_cnt, kSelP, keep, 1};
    sel.init(tid);
    __syncthreads();
    for (int base = 0; base < rows; base += 256) {
        const int r = base + tid;
        if (r < rows) {
            const float s = -acc[r];
            sel.offer(0, f32_ord(s == 0.0f ? 0.0f : s), r);
        }
        sel.chunk_done(tid, base + 256 >= rows);
    }
    int32_t* co = cand + ((size_t)q * f.nblocks + b) * (size_t)keep;
    for (int i = tid; i < keep; i += 256) {
        const u64 key = sel.keys[i];
        co[i] = key != ~0ull ? b * kB + (int)(uint32_t)key : -1;
    }
    if (tid == 0)
        tblock[(size_t)q * f.nblocks + b] = rows >= keep ? -ord_f32((uint32_t)(sel.keys[keep - 1] >> 32)) : -INFINITY;
}

template <int SP>
__global__ __launch_bounds__(256) void sparse_inv_rerank_kernel(
    const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ ids, const float* __restrict__ vals,
    const int64_t* __restrict__ q_ptr, const uint32_t* __restrict__ q_ids, const float* __restrict__ q_vals,
    const double* __restrict__ qnorm, int kind, int nblocks, float beta, int longest, int keep, int k,
    const int32_t* __restrict__ cand, const float* __restrict__ tblock, const int32_t* __restrict__ ext_ids,
    float* __restrict__ out_d, int32_t* __restrict__ out_ids, int32_t* __restrict__ out_cnt, int* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ int s_cnt[1];
    __shared__ uint32_t s_tmax;
    const int tid = threadIdx.x, q = blockIdx.x;
    SplitTopK<1> sel{reinterpret_cast<u64*>(smem), s_cnt, kSelP, k, 1};
    uint32_t* sq_ids = reinterpret_cast<uint32_t*>(sel.keys + kSelP);   // [kSparseQCap]
    float* sq_vals = reinterpret_cast<float*>(sq_ids + kSparseQCap);
    const int64_t qb = q_ptr[q];
    const int m = (int)(q_ptr[q + 1] - qb);   // <= kSparseQCap: the plan's gate
    for (int i = tid; i < m; i += 256) {
        sq_ids[i] = q_ids[qb + i];
        sq_vals[i] = q_vals[qb + i];
    }
    if (tid == 0) s_tmax = 0u;
    sel.init(tid);
    __syncthreads();
    const int ncand = nblocks * keep;
    const int32_t* cq = cand + (size_t)q * ncand;
    for (int base = 0; base < ncand; base += 256) {
        const int c = base + tid;
        const int pos = c < ncand ? cq[c] : -1;
        if (pos >= 0) {
            const int64_t p0 = row_ptr[pos];
            float d, unused;
            sparse_pair<SP>(ids + p0, vals + p0, (int)(row_ptr[pos + 1] - p0), sq_ids, sq_vals, m, d, unused);
            sel.offer(0, f32_ord(d == 0.0f ? 0.0f : d), pos);
        }
        sel.chunk_done(tid, base + 256 >= ncand);
    }
    uint32_t tm = 0u;
    for (int i = tid; i < nblocks; i += 256) tm = max(tm, f32_ord(tblock[(size_t)q * nblocks + i]));
    atomicMax(&s_tmax, tm);
    __syncthreads();
    const int kept = s_cnt[0];
    for (int i = tid; i < k; i += 256) {
        const u64 key = i < kept ? sel.keys[i] : ~0ull;
        const bool ok = key != ~0ull;
        out_ids[(size_t)q * k + i] = ok ? ext_ids[(uint32_t)key] : -1;
        out_d[(size_t)q * k + i] = ok ? ord_f32((uint32_t)(key >> 32)) : INFINITY;
    }
    if (tid == 0) {
        out_cnt[q] = kept;
        bool proved = false;
        if (kept >= k) {
            const double dk = (double)ord_f32((uint32_t)(sel.keys[k - 1] >> 32));
            const double fl = spf::floor_dist(kind, (double)ord_f32(s_tmax), m, m + longest, qnorm[q], (double)beta);
            proved = dk < fl;   // (false for a NaN floor)
        }
        flags[q] = proved ? 0 : 1;
    }
}

template <int SP>
hipError_t launch_rerank(int kind, const spf::Plan& p, const SparseInvFile& f, int m, int k, const int64_t* row_ptr,
                         const uint32_t* ids, const float* vals, const int64_t* q_ptr, const uint32_t* q_ids,
                         const float* q_vals, const double* qnorm, const SparseInvWs& ws, const int32_t* ext_ids,
                         float* out_d, int32_t* out_ids, int32_t* out_cnt, int* flags, hipStream_t s) {
    return launch_with_lds(sparse_inv_rerank_kernel<SP>, dim3(m), (size_t)kSelP * 8 + (size_t)kSparseQCap * 8, s, row_ptr,
                           ids, vals, q_ptr, q_ids, q_vals, qnorm, kind, p.nblocks, f.beta, f.longest, p.keep, k, ws.cand,
                           ws.tblock, ext_ids, out_d, out_ids, out_cnt, flags);
}

}  // namespace

int sparse_fast_kind(int space) {
    switch (space) {
        case SP_NEGDOT: return spf::DOT;
        case SP_QNORM_NEGDOT: return spf::QNORM;
        case SP_COSINE: return spf::COS;
        case SP_ANGULAR: return spf::ANG;
        default: return -1;
    }
}

hipError_t launch_sparse_inv(int space, const spf::Plan& p, const SparseInvFile& f, int q0, int m, int k,
                             const int64_t* row_ptr, const uint32_t* ids, const float* vals, const int64_t* q_ptr,
                             const uint32_t* q_ids, const float* q_vals, const double* qnorm, const SparseInvWs& ws,
                             const int32_t* ext_ids, float* out_d, int32_t* out_ids, int32_t* out_cnt, hipStream_t s) {
    const int kind = sparse_fast_kind(space);
    if (kind < 0 || m < 1 || (long long)m * p.nblocks > 2147483647LL) return hipErrorInvalidValue;
    const size_t lds = (size_t)kB * 4 + (size_t)kChunk * 12;
    hipError_t e = launch_with_lds(sparse_inv_accum_kernel, dim3((unsigned)(m * p.nblocks)), lds, s, f, q_ptr + q0, q_ids,
                                   q_vals, m, p.keep, ws.cand, ws.tblock);
    if (e != hipSuccess) return e;
    float* od = out_d + (size_t)q0 * k;
    int32_t* oi = out_ids + (size_t)q0 * k;
    switch (space) {
        case SP_NEGDOT:
            return launch_rerank<SP_NEGDOT>(kind, p, f, m, k, row_ptr, ids, vals, q_ptr + q0, q_ids, q_vals, qnorm + q0, ws,
                                            ext_ids, od, oi, out_cnt + q0, ws.flags + q0, s);
        case SP_QNORM_NEGDOT:
            return launch_rerank<SP_QNORM_NEGDOT>(kind, p, f, m, k, row_ptr, ids, vals, q_ptr + q0, q_ids, q_vals,
                                                  qnorm + q0, ws, ext_ids, od, oi, out_cnt + q0, ws.flags + q0, s);
        case SP_COSINE:
            return launch_rerank<SP_COSINE>(kind, p, f, m, k, row_ptr, ids, vals, q_ptr + q0, q_ids, q_vals, qnorm + q0, ws,
                                            ext_ids, od, oi, out_cnt + q0, ws.flags + q0, s);
        default:
            return launch_rerank<SP_ANGULAR>(kind, p, f, m, k, row_ptr, ids, vals, q_ptr + q0, q_ids, q_vals, qnorm + q0, ws,
                                             ext_ids, od, oi, out_cnt + q0, ws.flags + q0, s);
    }
}

}  // namespace gfxknn
