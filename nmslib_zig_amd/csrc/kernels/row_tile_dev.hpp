// The distance arrangement of the batched exact scans (range_batch_kernels.hip, bigk_batch_kernels.hip): a wave owns 64
// consecutive rows and keeps them in registers, lane l holding each row's elements l, l + 64, ...  For one query every lane
// runs its chain for all 64 rows; the 64 x 64 partials are reduced in the order of wave_sum / wave_max as a reduce-scatter
// (half the values go to the partner at xor 32, a quarter at xor 16, ...), after which lane i holds row i's distance: 63
// adds per lane for 64 pairs.
// The rule both files rely on: such a distance is, bit for bit, what wave_exact_distance_f32 / _u8 returns for that pair --
// the same 64 chains with the same operation per step, the same butterfly, the same finish.
#pragma once
#include "common_dev.hpp"

namespace gfxknn {

enum { RB_L2, RB_L1, RB_LINF, RB_DOT, RB_COS };

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

// ---- float rows.  C = ceil(dim / 64) elements of a row per lane; TAIL: dim is no multiple of 64, the last element's step
// is skipped by the lanes past the row's end as the loop of wave_exact_distance_f32 skips it (last_ok: this lane's last
// element lies inside the row).

// rv = rows [first, first + 64) (a row past n - 1 repeats the last one), zeros past dim; RB_COS: -> this lane's row's
// squared norm (row `lane` of the 64), else 0
template <int KIND, int C, bool TAIL>
__device__ __forceinline__ float rb_load_rows(const float* __restrict__ rows, int ld, int n, size_t first, int dim, int lane,
                                              bool last_ok, float (&rv)[64][C]) {
#pragma unroll
    for (int r = 0; r < 64; ++r) {
        const size_t row = first + r < (size_t)n ? first + r : (size_t)n - 1;
        const float* a = rows + row * (size_t)ld;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int d = lane + 64 * c;
            const bool ok = d < dim;
            const float x = a[ok ? d : 0];
            rv[r][c] = ok ? x : 0.f;
        }
    }
    if (KIND != RB_COS) return 0.f;
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
    return rb_reduce_scatter<false>(v, lane);
}

// A tile of tq <= TILE queries, the first one q0, into qs [TILE][C * 64] (zeros past dim and past tq) by a workgroup of 256
// threads; RB_COS: their squared norms into qnorm.  Ends behind a barrier; the caller keeps one before the call.
template <int KIND, int C, bool TAIL, int TILE>
__device__ __forceinline__ void rb_stage_queries(const float* __restrict__ queries, int dim, int q0, int tq, bool last_ok,
                                                 float* qs, float* qnorm) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < TILE * C * 64; i += 256) {
        const int qi = i / (C * 64), d = i % (C * 64);
        const bool ok = qi < tq && d < dim;
        const float x = queries[ok ? (size_t)(q0 + qi) * dim + d : 0];
        qs[i] = ok ? x : 0.f;
    }
    __syncthreads();
    if (KIND == RB_COS) {   // one wave per query
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
}

// lane i: the distance of row i of rv to the query at q (C * 64 staged floats); rnorm, qnorm: RB_COS only
template <int KIND, int C, bool TAIL>
__device__ __forceinline__ float rb_tile_distance(int space, const float (&rv)[64][C], const float* q, int lane, bool last_ok,
                                                  float rnorm, float qnorm) {
    float qv[C];
#pragma unroll
    for (int c = 0; c < C; ++c) qv[c] = q[c * 64 + lane];
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
        const float sim = normdot_finish(d, rnorm, qnorm);
        d = space == SP_ANGULAR ? acosf(sim) : fmaxf(0.0f, 1.0f - sim);
    }
    return d;
}

// ---- l2sqr_sift: 128 bytes per row, two per lane (one 16-bit load), kept as two 16-bit integers in a register; a pair is
// one packed subtraction and one v_dot2_i32_i16.  Integer arithmetic, exact in any order.
typedef short rb_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ rb_short2 rb_two_bytes(unsigned short x) {
    rb_short2 r;
    r.x = (short)(x & 255);
    r.y = (short)(x >> 8);
    return r;
}
// rv = rows [first, first + 64) (rows are 128-byte aligned)
__device__ __forceinline__ void rb_load_rows_u8(const uint8_t* __restrict__ rows, int n, size_t first, int lane,
                                                rb_short2 (&rv)[64]) {
#pragma unroll
    for (int r = 0; r < 64; ++r) {
        const size_t row = first + r < (size_t)n ? first + r : (size_t)n - 1;
        rv[r] = rb_two_bytes(reinterpret_cast<const unsigned short*>(rows + row * 128)[lane]);
    }
}
// a tile of tq <= TILE queries into qs [TILE][128] (the caller's queries have no alignment: byte loads); 256 threads
template <int TILE>
__device__ __forceinline__ void rb_stage_queries_u8(const uint8_t* __restrict__ queries, int q0, int tq, uint8_t* qs) {
    for (int i = threadIdx.x; i < TILE * 128; i += 256) {
        const bool ok = i / 128 < tq;
        const uint8_t x = queries[ok ? (size_t)q0 * 128 + i : 0];
        qs[i] = ok ? x : (uint8_t)0;
    }
    __syncthreads();
}
// lane i: the distance of row i to the staged query q (128 bytes, 2-byte aligned)
__device__ __forceinline__ float rb_tile_distance_u8(const rb_short2 (&rv)[64], const uint8_t* q, int lane) {
    const rb_short2 y = rb_two_bytes(reinterpret_cast<const unsigned short*>(q)[lane]);
    int v[64];
#pragma unroll
    for (int r = 0; r < 64; ++r) {
        const rb_short2 d = rv[r] - y;
        v[r] = __builtin_amdgcn_sdot2(d, d, 0, false);
    }
    return (float)rb_reduce_scatter<false>(v, lane);
}

}  // namespace gfxknn
