// Batched range search on the exact scan: many queries in one pass over the rows.
//   1. range_batch_mask : a wave owns 64 consecutive rows and keeps them in registers, lane l holding each row's elements
//                         l, l + 64, ...  A tile of queries sits in LDS.  For one query every lane runs its chain for all 64
//                         rows; the 64 x 64 partials are reduced in the order of wave_sum / wave_max as a reduce-scatter
//                         (half the values go to the partner at xor 32, a quarter at xor 16, ...), after which lane i holds
//                         row i's distance: 63 adds per lane for 64 pairs (the exchanges at xor 32 and 16 are lane-swap
//                         instructions, the rest shuffles).  One ballot of d <= r is the 64 match bits of
//                         (query, these rows), written as one word.
//   2. range_batch_count: matches per (query, 1024-row block) = popcounts of 16 words;
//   3. range_batch_scan : per query the exclusive scan of its block counts, the total behind them;
//   4. range_batch_pad  : -1 / +inf behind the entries a query gets;
//   5. range_batch_scatter: the first `capacity` matches in position order, each with its external id and the distance
//                         wave_exact_distance_* returns -- the function the single-query path calls.
// The rule (range_batch_plan.hpp's callers rely on it): a distance in pass 1 is, bit for bit, what wave_exact_distance_f32 /
// _u8 returns for that pair -- the same 64 chains with the same operation per step, the same butterfly, the same finish -- so
// a batch answers exactly as nmslib_range_query_fill does per query.  This file is built with the flags of range_kernels.hip.
#include "../range_batch_plan.hpp"
#include "common_dev.hpp"
#include "kernels.hpp"

namespace gfxknn {

namespace {

enum { RB_L2, RB_L1, RB_LINF, RB_DOT, RB_COS };
constexpr int kTile = (int)kRangeBatchQueryTile;
static_assert(kRangeBatchRowsPerWg == 256 && kRangeBatchSelectRows == 1024, "the kernels' shapes");

// one step of a lane's chain, as wave_exact_distance_f32 writes it
template <int KIND>
__device__ __forceinline__ float rb_step(float s, float a, float q) {
    if (KIND == RB_L2) {
        const float t = a - q;
        return fmaf(t, t, s);
    }
    if (KIND == RB_L1) return s + fabsf(a - q);
    if (KIND == RB_LINF) return fmaxf(s, fabsf(a - q));
    return fmaf(a, q, s);
}

// v[r] = this lane's partial of row r -> the value wave_sum / wave_max returns for row `lane`.  At offset o a lane keeps the
// o rows whose bit o equals its own and adds the partner's partials of them: the operands of every addition are those of
// the butterfly's, so are the bits.  Every index is a compile-time constant.  Offsets 32 and 16 are one half-exchange each
// (v_permlane32_swap: lanes 32..63 of the first operand change places with lanes 0..31 of the second; v_permlane16_swap:
// the odd 16-lane rows of the first with the even rows of the second): afterwards one operand holds what the lane keeps
// and the other what its partner sent, in every lane.  The smaller offsets select and shuffle.
template <bool MAX, typename T>
__device__ __forceinline__ T rb_combine(T a, T b) {
    if constexpr (MAX) return fmaxf(a, b);
    else return a + b;
}
template <bool MAX, typename T>
__device__ __forceinline__ T rb_reduce_scatter(T (&v)[64], int lane) {
    static_assert(sizeof(T) == 4, "one register per value");
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, v[i]), __builtin_bit_cast(unsigned, v[i + 32]),
                                                        false, false);
        v[i] = rb_combine<MAX>(__builtin_bit_cast(T, (unsigned)r[0]), __builtin_bit_cast(T, (unsigned)r[1]));
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, v[i]), __builtin_bit_cast(unsigned, v[i + 16]),
                                                        false, false);
        v[i] = rb_combine<MAX>(__builtin_bit_cast(T, (unsigned)r[0]), __builtin_bit_cast(T, (unsigned)r[1]));
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) {
        const bool up = (lane & o) != 0;
#pragma unroll
        for (int i = 0; i < o; ++i) {
            const T lo = v[i], hi = v[i + o];
            const T keep = up ? hi : lo, send = up ? lo : hi;
            v[i] = rb_combine<MAX>(keep, (T)__shfl_xor(send, o, 64));
        }
    }
    return v[0];
}

// C = ceil(dim / 64) elements of a row per lane; TAIL: dim is no multiple of 64, the last element's step is skipped by the
// lanes past the row's end as the loop of wave_exact_distance_f32 skips it.
// grid (row blocks of 256, query splits): a workgroup takes the query tiles blockIdx.y, blockIdx.y + gridDim.y, ...
template <int KIND, int C, bool TAIL>
__global__ __launch_bounds__(256) void range_batch_mask_kernel(int space, const float* __restrict__ rows, int ld, int n,
                                                               const float* __restrict__ queries, int dim, int nq,
                                                               const float* __restrict__ radii, u64* __restrict__ masks,
                                                               size_t mask_words) {
    __shared__ float qs[kTile * C * 64];
    __shared__ float qnorm[kTile];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t word = (size_t)blockIdx.x * 4 + wave;   // the mask word of this wave's rows
    const bool active = word * 64 < (size_t)n;           // (a wave past the rows only keeps the barriers)
    const bool last_ok = lane + 64 * (C - 1) < dim;

    float rv[64][C];
    float rnorm = 0.f;
    if (active) {
#pragma unroll
        for (int r = 0; r < 64; ++r) {
            const size_t row = word * 64 + r < (size_t)n ? word * 64 + r : (size_t)n - 1;
            const float* a = rows + row * (size_t)ld;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int d = lane + 64 * c;
                const bool ok = d < dim;
                const float x = a[ok ? d : 0];
                rv[r][c] = ok ? x : 0.f;
            }
        }
        if (KIND == RB_COS) {   // the rows' squared norms: lane i keeps row i's
            float v[64];
#pragma unroll
            for (int r = 0; r < 64; ++r) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float t = fmaf(rv[r][c], rv[r][c], s);
                    s = (TAIL && c == C - 1 && !last_ok) ? s : t;
                }
                v[r] = s;
            }
            rnorm = rb_reduce_scatter<false>(v, lane);
        }
    }

    const int ntiles = (nq + kTile - 1) / kTile;
    for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
        const int q0 = t * kTile;
        const int tq = nq - q0 < kTile ? nq - q0 : kTile;
        __syncthreads();   // the last tile has been read
        for (int i = threadIdx.x; i < kTile * C * 64; i += 256) {
            const int qi = i / (C * 64), d = i % (C * 64);
            const bool ok = qi < tq && d < dim;
            const float x = queries[ok ? (size_t)(q0 + qi) * dim + d : 0];
            qs[i] = ok ? x : 0.f;
        }
        __syncthreads();
        if (KIND == RB_COS) {   // the queries' squared norms, one wave per query
            for (int qi = wave; qi < tq; qi += 4) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float y = qs[qi * C * 64 + c * 64 + lane];
                    const float t2 = fmaf(y, y, s);
                    s = (TAIL && c == C - 1 && !last_ok) ? s : t2;
                }
                s = wave_sum(s);
                if (lane == 0) qnorm[qi] = s;
            }
            __syncthreads();
        }
        if (!active) continue;
        for (int qi = 0; qi < tq; ++qi) {
            float qv[C];
#pragma unroll
            for (int c = 0; c < C; ++c) qv[c] = qs[qi * C * 64 + c * 64 + lane];
            float v[64];
#pragma unroll
            for (int r = 0; r < 64; ++r) {
                float s = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float t2 = rb_step<KIND>(s, rv[r][c], qv[c]);
                    s = (TAIL && c == C - 1 && !last_ok) ? s : t2;
                }
                v[r] = s;
            }
            float d = rb_reduce_scatter<KIND == RB_LINF>(v, lane);
            if (KIND == RB_L2) {
                if (space == SP_L2) d = sqrtf(d);
            } else if (KIND == RB_DOT) {
                if (space == SP_NEGDOT) {
                    d = -d;
                } else {
                    const float c = fmaxf(-1.0f, fminf(1.0f, d));
                    d = fmaxf(0.0f, 1.0f - c);
                }
            } else if (KIND == RB_COS) {
                const float sim = normdot_finish(d, rnorm, qnorm[qi]);
                d = space == SP_ANGULAR ? acosf(sim) : fmaxf(0.0f, 1.0f - sim);
            }
            const bool hit = word * 64 + lane < (size_t)n && d <= radii[q0 + qi];
            const u64 b = __ballot(hit);
            if (lane == 0) masks[(size_t)(q0 + qi) * mask_words + word] = b;
        }
    }
}

// l2sqr_sift: 128 bytes per row, two per lane (one 16-bit load), kept as two 16-bit integers in a register; a pair is one
// packed subtraction and one v_dot2_i32_i16.  Integer arithmetic, exact in any order.
typedef short rb_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ rb_short2 rb_two_bytes(unsigned short x) {
    rb_short2 r;
    r.x = (short)(x & 255);
    r.y = (short)(x >> 8);
    return r;
}
__global__ __launch_bounds__(256) void range_batch_mask_u8_kernel(const uint8_t* __restrict__ rows, int n,
                                                                  const uint8_t* __restrict__ queries, int nq,
                                                                  const float* __restrict__ radii, u64* __restrict__ masks,
                                                                  size_t mask_words) {
    __shared__ uint8_t qs[kTile * 128];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t word = (size_t)blockIdx.x * 4 + wave;
    const bool active = word * 64 < (size_t)n;
    rb_short2 rv[64];
    if (active) {
#pragma unroll
        for (int r = 0; r < 64; ++r) {
            const size_t row = word * 64 + r < (size_t)n ? word * 64 + r : (size_t)n - 1;
            rv[r] = rb_two_bytes(reinterpret_cast<const unsigned short*>(rows + row * 128)[lane]);   // (rows are 128-byte aligned)
        }
    }
    const int ntiles = (nq + kTile - 1) / kTile;
    for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
        const int q0 = t * kTile;
        const int tq = nq - q0 < kTile ? nq - q0 : kTile;
        __syncthreads();
        for (int i = threadIdx.x; i < kTile * 128; i += 256) {   // (the caller's queries have no alignment: byte loads)
            const bool ok = i / 128 < tq;
            const uint8_t x = queries[ok ? (size_t)q0 * 128 + i : 0];
            qs[i] = ok ? x : (uint8_t)0;
        }
        __syncthreads();
        if (!active) continue;
        for (int qi = 0; qi < tq; ++qi) {
            const rb_short2 y = rb_two_bytes(reinterpret_cast<const unsigned short*>(qs + qi * 128)[lane]);
            int v[64];
#pragma unroll
            for (int r = 0; r < 64; ++r) {
                const rb_short2 d = rv[r] - y;
                v[r] = __builtin_amdgcn_sdot2(d, d, 0, false);
            }
            const float d = (float)rb_reduce_scatter<false>(v, lane);
            const bool hit = word * 64 + lane < (size_t)n && d <= radii[q0 + qi];
            const u64 b = __ballot(hit);
            if (lane == 0) masks[(size_t)(q0 + qi) * mask_words + word] = b;
        }
    }
}

// counts[q][b] = matches of query q in rows [1024 b, 1024 b + 1024); grid (ceil(nb / 256), queries)
__global__ __launch_bounds__(256) void range_batch_count_kernel(const u64* __restrict__ masks, size_t mask_words, int nb,
                                                                int* __restrict__ counts) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const u64* m = masks + (size_t)blockIdx.y * mask_words;
    int c = 0;
    for (size_t w = (size_t)b * 16; w < (size_t)b * 16 + 16 && w < mask_words; ++w) c += __popcll(m[w]);
    counts[(size_t)blockIdx.y * (nb + 1) + b] = c;
}

__device__ __forceinline__ int rb_block_exclusive_scan(int v, int* total) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; ++w) base += wsum[w];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return base + incl - v;
}

// one workgroup per query: exclusive scan of its nb block counts in place (256 per pass, a running carry), the total behind
// them and into the caller's arrays
__global__ __launch_bounds__(256) void range_batch_scan_kernel(int* __restrict__ counts, int nb, size_t capacity,
                                                               int32_t* __restrict__ out_counts,
                                                               int32_t* __restrict__ out_totals) {
    int* c = counts + (size_t)blockIdx.x * (nb + 1);
    int carry = 0;
    for (int base = 0; base < nb; base += 256) {
        const int i = base + threadIdx.x;
        const int v = i < nb ? c[i] : 0;
        int total;
        const int ex = rb_block_exclusive_scan(v, &total);
        if (i < nb) c[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) {
        c[nb] = carry;
        if (out_totals) out_totals[blockIdx.x] = carry;
        if (out_counts) out_counts[blockIdx.x] = (size_t)carry < capacity ? carry : (int32_t)capacity;
    }
}

// entries [min(total, capacity), capacity) of every query: -1 / +inf; grid (ceil(capacity / 256), queries).  total[q *
// total_stride] is query q's number of matches.
__global__ __launch_bounds__(256) void range_batch_pad_kernel(const int* __restrict__ total, size_t total_stride,
                                                              size_t capacity, int32_t* __restrict__ out_ids,
                                                              float* __restrict__ out_dists) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= capacity || i < (size_t)total[(size_t)blockIdx.y * total_stride]) return;
    out_ids[(size_t)blockIdx.y * capacity + i] = -1;
    out_dists[(size_t)blockIdx.y * capacity + i] = INFINITY;
}

// grid (nb, queries): a wave takes 4 of the block's 16 words and emits their matches one by one, in position order
__global__ __launch_bounds__(256) void range_batch_scatter_kernel(int space, const void* __restrict__ rows, int ld, int dim,
                                                                  const void* __restrict__ queries,
                                                                  const u64* __restrict__ masks, size_t mask_words, int nb,
                                                                  const int* __restrict__ counts,
                                                                  const int32_t* __restrict__ ext_ids, size_t capacity,
                                                                  int32_t* __restrict__ out_ids, float* __restrict__ out_dists) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t q = blockIdx.y;
    const int* c = counts + q * (nb + 1);
    const int off = c[blockIdx.x];
    if (c[blockIdx.x + 1] == off || (size_t)off >= capacity) return;
    const u64* m = masks + q * mask_words;
    const size_t w0 = (size_t)blockIdx.x * 16;
    size_t at = (size_t)off;
    for (int i = 0; i < wave * 4; ++i)
        if (w0 + i < mask_words) at += __popcll(m[w0 + i]);
    for (int j = 0; j < 4; ++j) {
        const size_t w = w0 + wave * 4 + j;
        if (w >= mask_words) return;
        u64 left = m[w];
        while (left) {
            if (at >= capacity) return;
            const size_t row = w * 64 + __builtin_ctzll(left);
            left &= left - 1;
            float d;
            if (space == SP_L2SQR_SIFT)
                d = (float)wave_exact_distance_u8(static_cast<const uint8_t*>(rows) + row * 128,
                                                  static_cast<const uint8_t*>(queries) + q * 128, lane);
            else
                d = wave_exact_distance_f32(space, static_cast<const float*>(rows) + row * (size_t)ld,
                                            static_cast<const float*>(queries) + q * (size_t)dim, dim, lane);
            if (lane == 0) {
                out_ids[q * capacity + at] = ext_ids[row];
                out_dists[q * capacity + at] = d;
            }
            ++at;
        }
    }
}

template <int KIND, int C>
void rb_launch_mask(bool tail, dim3 grid, hipStream_t s, const RangeBatchArgs& a) {
    const float* rows = static_cast<const float*>(a.rows);
    const float* q = static_cast<const float*>(a.queries);
    if (tail)
        hipLaunchKernelGGL((range_batch_mask_kernel<KIND, C, true>), grid, dim3(256), 0, s, a.space, rows, a.ld, a.n, q, a.dim,
                           a.nq, a.radii, a.masks, a.mask_words);
    else
        hipLaunchKernelGGL((range_batch_mask_kernel<KIND, C, false>), grid, dim3(256), 0, s, a.space, rows, a.ld, a.n, q,
                           a.dim, a.nq, a.radii, a.masks, a.mask_words);
}

template <int KIND>
void rb_launch_mask_c(int chunks, bool tail, dim3 grid, hipStream_t s, const RangeBatchArgs& a) {
    if (chunks == 1) rb_launch_mask<KIND, 1>(tail, grid, s, a);
    else if (chunks == 2) rb_launch_mask<KIND, 2>(tail, grid, s, a);
    else if (chunks == 3) rb_launch_mask<KIND, 3>(tail, grid, s, a);
    else rb_launch_mask<KIND, 4>(tail, grid, s, a);
}

}  // namespace

hipError_t launch_range_batch(const RangeBatchArgs& a, hipStream_t s) {
    if (a.nq <= 0) return hipSuccess;
    const bool u8 = a.space == SP_L2SQR_SIFT;
    if (a.n < 0 || a.grid_y < 1 || (!u8 && (a.dim < 1 || a.dim > (int)kRangeBatchMaxDim)) || (u8 && a.dim != 128))
        return hipErrorInvalidValue;
    const int nb = (int)(((size_t)a.n + kRangeBatchSelectRows - 1) / kRangeBatchSelectRows);
    if (a.n > 0) {
        if ((size_t)a.grid_x * kRangeBatchRowsPerWg < (size_t)a.n || a.mask_words * 64 < (size_t)a.n) return hipErrorInvalidValue;
        const dim3 grid(a.grid_x, a.grid_y);
        if (u8) {
            hipLaunchKernelGGL(range_batch_mask_u8_kernel, grid, dim3(256), 0, s, static_cast<const uint8_t*>(a.rows), a.n,
                               static_cast<const uint8_t*>(a.queries), a.nq, a.radii, a.masks, a.mask_words);
        } else {
            const int chunks = (a.dim + 63) / 64;
            const bool tail = a.dim % 64 != 0;
            switch (a.space) {
                case SP_L2:
                case SP_L2SQR: rb_launch_mask_c<RB_L2>(chunks, tail, grid, s, a); break;
                case SP_L1: rb_launch_mask_c<RB_L1>(chunks, tail, grid, s, a); break;
                case SP_LINF: rb_launch_mask_c<RB_LINF>(chunks, tail, grid, s, a); break;
                case SP_NEGDOT:
                case SP_NORMCOS: rb_launch_mask_c<RB_DOT>(chunks, tail, grid, s, a); break;
                case SP_COSINE:
                case SP_ANGULAR: rb_launch_mask_c<RB_COS>(chunks, tail, grid, s, a); break;
                default: return hipErrorInvalidValue;
            }
        }
        hipLaunchKernelGGL(range_batch_count_kernel, dim3((nb + 255) / 256, a.nq), dim3(256), 0, s, a.masks, a.mask_words, nb,
                           a.counts);
    }
    hipLaunchKernelGGL(range_batch_scan_kernel, dim3(a.nq), dim3(256), 0, s, a.counts, nb, a.capacity, a.out_counts,
                       a.out_totals);
    if (a.capacity > 0) {
        if (a.pad)
            hipLaunchKernelGGL(range_batch_pad_kernel, dim3((unsigned)((a.capacity + 255) / 256), a.nq), dim3(256), 0, s,
                           a.counts + nb, (size_t)nb + 1, a.capacity, a.out_ids, a.out_dists);
        if (a.n > 0)
            hipLaunchKernelGGL(range_batch_scatter_kernel, dim3(nb, a.nq), dim3(256), 0, s, a.space, a.rows, a.ld, a.dim,
                               a.queries, a.masks, a.mask_words, nb, a.counts, a.ext_ids, a.capacity, a.out_ids, a.out_dists);
    }
    return hipGetLastError();
}

__global__ void range_batch_one_kernel(const int* __restrict__ total, size_t capacity, int32_t* __restrict__ out_count,
                                       int32_t* __restrict__ out_total) {
    if (out_total) *out_total = *total;
    if (out_count) *out_count = (size_t)*total < capacity ? *total : (int32_t)capacity;
}

hipError_t launch_range_batch_finish(const int* total, size_t capacity, int32_t* out_ids, float* out_dists,
                                     int32_t* out_count, int32_t* out_total, bool pad, hipStream_t s) {
    if (out_count || out_total) hipLaunchKernelGGL(range_batch_one_kernel, dim3(1), dim3(1), 0, s, total, capacity, out_count, out_total);
    if (capacity > 0 && pad)
        hipLaunchKernelGGL(range_batch_pad_kernel, dim3((unsigned)((capacity + 255) / 256), 1), dim3(256), 0, s, total,
                           (size_t)0, capacity, out_ids, out_dists);
    return hipGetLastError();
}

}  // namespace gfxknn
