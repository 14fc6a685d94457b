// Inner-product form of the Bregman "fast" divergences for the bf16 MFMA filter scan, with the bound
// that ties the filter's key back to the f32 distance the exact scan (DivAcc, kernels/diverg_dev.hpp) returns.
// Header-only and free of HIP, so that a plain host program can include it; under hipcc the functions are also callable
// on the device.  All arithmetic is f64 on the f32 inputs.
//
// With x the row, q the query, lx / lq their stored logarithms and iq = fl(1 / q) as the scan rounds it, in real numbers
//     d(row, query) = sign * (a . b) + R_row + C_q
//   form       a    b    sign  R_row               C_q
//   KL         x    lq   -1    sum x lx            0
//   KL_RQ      lx   q    -1    0                   sum q lq
//   KLGEN      x    lq   -1    sum x lx - sum x    sum q
//   KLGEN_RQ   lx   q    -1    sum x               sum q lq - sum q
//   IS         x    iq   +1    -sum lx             sum lq - D
// Every operand value v is split into two bf16 numbers, v = hi + lo + r, and the filter takes
//     key = fl32(sign * acc + R32),   acc = MFMA chain of a_hi.b_hi + a_hi.b_lo + a_lo.b_hi,   R32 = fl32(R_row).
// query() gives E_q with | key + C_q - d^ | <= E_q for every stored row, d^ the f32 distance of the exact scan.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define DVF_HD __host__ __device__
#else
#define DVF_HD
#endif

namespace gfxknn {
namespace dvf {

enum Form : int { KL = 0, KL_RQ = 1, KLGEN = 2, KLGEN_RQ = 3, IS = 4 };
constexpr int kMaxDim = 256;        // 16 K-steps of query fragments: 128 registers
constexpr int kMinRows = 65536, kMinQueries = 256, kMaxK = 128;

DVF_HD inline bool row_is_log(int form) { return form == KL_RQ || form == KLGEN_RQ; }
DVF_HD inline double sign_of(int form) { return form == IS ? 1.0 : -1.0; }

// ---- the bf16 split ------------------------------------------------------------------------------------------------
DVF_HD inline uint32_t f32_bits(float f) {
    union { float f; uint32_t u; } c;
    c.f = f;
    return c.u;
}
DVF_HD inline float bits_f32(uint32_t u) {
    union { float f; uint32_t u; } c;
    c.u = u;
    return c.f;
}
// round to nearest even to 8 significant bits; subnormal results become zero (the matrix cores may flush them: what is
// dropped here is measured as residual instead); NaN and infinity keep their class
DVF_HD inline uint16_t bf16_rn(float f) {
    const uint32_t u = f32_bits(f);
    if ((u & 0x7F800000u) == 0x7F800000u) return (uint16_t)((u >> 16) | ((u & 0xFFFFu) ? 0x40u : 0u));
    const uint32_t r = u + 0x7FFFu + ((u >> 16) & 1u);
    if ((r & 0x7F800000u) == 0u) return (uint16_t)((u >> 16) & 0x8000u);
    return (uint16_t)(r >> 16);
}
DVF_HD inline float bf16_f32(uint16_t h) { return bits_f32((uint32_t)h << 16); }
DVF_HD inline void split(float v, uint16_t* hi, uint16_t* lo) {
    *hi = bf16_rn(v);
    *lo = bf16_rn(v - bf16_f32(*hi));   // (the difference of a float and its 8-bit rounding is a float: exact)
}

// the smallest float that is not below r (r >= 0)
DVF_HD inline float round_up_f32(double r) {
    float f = (float)r;
    if ((double)f < r) f = std::nextafterf(f, INFINITY);
    return f;
}

// ---- rows ------------------------------------------------------------------------------------------------------------
DVF_HD inline float row_operand(int form, float x, float lx) { return row_is_log(form) ? lx : x; }

// Largest values over the stored rows, each rounded up to f32: norms of the operand, of its hi and lo parts and of its
// split residual; sum of the absolute terms of R_row.  (Norms: sqrt of an f64 sum of squares, widened by 2^-40.)
struct RowMax {
    float a, a_hi, a_lo, a_res, r_abs;
};

// one row: hi / lo [dpad] bf16 bits (zero past dim), R_row, and the row's own five figures into m (largest so far)
DVF_HD inline double row(int form, const float* x, const float* lx, size_t dim, size_t dpad, uint16_t* hi, uint16_t* lo,
                         RowMax* m) {
    double R = 0, Rabs = 0, na = 0, nh = 0, nl = 0, nr = 0;
    for (size_t j = dim; j < dpad; ++j) hi[j] = lo[j] = 0;
    for (size_t j = 0; j < dim; ++j) {
        const double xv = x[j], lv = lx[j];
        double t;   // this element's part of R_row; its absolute terms
        double ta;
        switch (form) {
            case KL: t = xv * lv, ta = std::fabs(t); break;
            case KL_RQ: t = 0, ta = 0; break;
            case KLGEN: t = xv * lv - xv, ta = std::fabs(xv * lv) + std::fabs(xv); break;
            case KLGEN_RQ: t = xv, ta = std::fabs(xv); break;
            default: t = -lv, ta = std::fabs(lv); break;
        }
        R += t;
        Rabs += ta;
        const float a = row_operand(form, x[j], lx[j]);
        split(a, &hi[j], &lo[j]);
        const double h = bf16_f32(hi[j]), l = bf16_f32(lo[j]), r = (double)a - h - l;   // (exact in f64)
        na += (double)a * a, nh += h * h, nl += l * l, nr += r * r;
    }
    const double w = 1.0 + 9.094947017729282e-13;   // 2^-40: the f64 sums and roots above
    const float v[5] = {round_up_f32(std::sqrt(na) * w), round_up_f32(std::sqrt(nh) * w), round_up_f32(std::sqrt(nl) * w),
                        round_up_f32(std::sqrt(nr) * w), round_up_f32(Rabs * w)};
    // (a NaN compares false and would be lost: it is carried over instead)
    m->a = !(v[0] <= m->a) ? v[0] : m->a;
    m->a_hi = !(v[1] <= m->a_hi) ? v[1] : m->a_hi;
    m->a_lo = !(v[2] <= m->a_lo) ? v[2] : m->a_lo;
    m->a_res = !(v[3] <= m->a_res) ? v[3] : m->a_res;
    m->r_abs = !(v[4] <= m->r_abs) ? v[4] : m->r_abs;
    return R;
}

// ---- queries ---------------------------------------------------------------------------------------------------------
DVF_HD inline float query_operand(int form, float q, float lq, float iq) {
    return form == IS ? iq : (row_is_log(form) ? q : lq);
}

constexpr double kU32 = 5.9604644775390625e-08;      // 2^-24: unit roundoff of f32, round to nearest
constexpr double kUAcc = 1.1920928955078125e-07;     // 2^-23: one f32 addition of the matrix cores, rounded or truncated
constexpr double kTiny = 1e-30;   // what underflow can lose in any of the (at most a few thousand) f32 operations

// One query: hi / lo [dim] bf16 bits of b, C_q and E_q (an upper bound of its real value).  iq: the reciprocals, read for
// IS only.  dpad: the scan's K range (dim padded to 16; the padding multiplies zeros).  Not finite -- no proof -- for a
// NaN or an infinity anywhere, and for a zero element (its stored logarithm is the -1e5 sentinel, its reciprocal inf).
//
// With T >= sum |products of the chain|, S >= sum |terms of the exact formula| (both by Cauchy-Schwarz on the rows'
// largest norms):
//   dropped lo.lo and split residuals   |a_lo||b_lo| + |a_res||b| + (|a| + |a_res|)|b_res|
//   MFMA chain, 3 dpad additions        1.001 * 3 dpad * 2^-23 * T
//   key = fl32(sign acc + R32)          2^-24 (1.001 T + 1.001 r_abs)
//   R32 = fl32(R_row), R_row in f64     (2^-24 + 2^-40) r_abs;   C_q in f64: 2^-40 c_abs
//   exact scan (DivAcc)                 1.001 (dim / 2 + 12) 2^-24 S:  a term passes at most 2 roundings before it enters
//                                       a lane's sum, 2 per element step there (dim / 4 steps), 3 in the combination, 6 in
//                                       the tail, 1 in finish
// Element j of q / lq / iq is at p[(j / 4) * gs + j % 4]: gs = 4 for plain arrays, the group stride of a query pack.
DVF_HD inline void query(int form, const float* q, const float* lq, const float* iq, size_t gs, size_t dim, size_t dpad,
                         const RowMax& m, uint16_t* hi, uint16_t* lo, double* C, double* E) {
    double c = 0, cabs = 0, nb = 0, nh = 0, nl = 0, nr = 0;
    bool proof = true;
    for (size_t j = dim; j < dpad; ++j) hi[j] = lo[j] = 0;
    for (size_t j = 0; j < dim; ++j) {
        const size_t at = (j >> 2) * gs + (j & 3);
        const float qf = q[at], lf = lq[at];
        const double qv = qf, lv = lf;
        proof = proof && qf > 0.0f && std::isfinite(qf) && std::isfinite(lf);
        switch (form) {
            case KL: break;
            case KL_RQ: c += qv * lv, cabs += std::fabs(qv * lv); break;
            case KLGEN: c += qv, cabs += std::fabs(qv); break;
            case KLGEN_RQ: c += qv * lv - qv, cabs += std::fabs(qv * lv) + std::fabs(qv); break;
            default: c += lv, cabs += std::fabs(lv) + 1.0; break;
        }
        const float b = query_operand(form, qf, lf, form == IS ? iq[at] : 0.f);
        proof = proof && std::isfinite(b);
        split(b, &hi[j], &lo[j]);
        const double h = bf16_f32(hi[j]), l = bf16_f32(lo[j]), r = (double)b - h - l;
        nb += (double)b * b, nh += h * h, nl += l * l, nr += r * r;
    }
    if (form == IS) c -= (double)dim;
    const double w = 1.0 + 9.094947017729282e-13;
    const double B = std::sqrt(nb) * w, Bh = std::sqrt(nh) * w, Bl = std::sqrt(nl) * w, Br = std::sqrt(nr) * w;
    const double T = (double)m.a_hi * Bh + (double)m.a_hi * Bl + (double)m.a_lo * Bh;
    const double S = (double)m.r_abs + cabs + (double)m.a * B;
    double e = (double)m.a_lo * Bl + (double)m.a_res * B + ((double)m.a + (double)m.a_res) * Br;
    e += 1.001 * 3.0 * (double)dpad * kUAcc * T;
    e += kU32 * 1.001 * (T + (double)m.r_abs);
    e += (kU32 + 9.094947017729282e-13) * (double)m.r_abs + 9.094947017729282e-13 * cabs;
    e += 1.001 * ((double)dim / 2 + 12.0) * kU32 * S;
    e = e * w + kTiny;
    // a chain whose partial sums could leave f32's range can give an infinite or NaN key, which no list holds: no proof
    proof = proof && T + (double)m.r_abs < 1e37;
    *C = c;
    *E = proof ? e : INFINITY;
}

// Lower bound of the f32 distance the exact scan returns for a row whose filter key is at least key_m, less the rounding
// of this expression itself.  A row can be left out of the re-rank when this is STRICTLY above the k-th exact distance
// (ties are ordered by position, so equality proves nothing).  NaN when there is no proof.
DVF_HD inline double filter_floor(float key_m, double C, double E) {
    const double k = (double)key_m;
    return (k + C - E) - (std::fabs(k) + std::fabs(C) + E) * 9.094947017729282e-13;   // 2^-40
}

// ---- plan ------------------------------------------------------------------------------------------------------------
constexpr int kRowBlock = 32;     // rows of one MFMA block
constexpr int kQueryTile = 128;   // queries of a workgroup: four waves of 32
constexpr int kKeep = 32;         // k': keys kept per (query, split)
// key buffer per query in LDS.  A buffer is sorted and cut to kKeep when the next block's 32 offers could overflow it, so
// kBuf - 32 - kKeep = 64 offers pass between two sorts.  (With kBuf = 64 every offer after the first cut cost a sort: at
// 1M x 128 about 250 sorts per list, 14 ms of scan)
constexpr int kBuf = 128;
constexpr int kSplits = 64;
constexpr int kGroup = 16;        // queries per fallback flag: the exact scan's tile

struct Plan {
    bool use;
    int ksteps, ksteps_max;   // K-steps of 16 columns; the kernel instantiation that holds them (4, 8 or 16)
    int nsplit, rows_per_split, nblocks;
    int qpad, nqt, ngroups;
};

inline Plan plan(int form, int n, int dim, int nq, int k, bool have_copy) {
    Plan p{};
    p.use = form >= KL && form <= IS && have_copy && n >= kMinRows && nq >= kMinQueries && dim >= 1 && dim <= kMaxDim &&
            k >= 1 && k <= kMaxK;
    p.ksteps = (dim + 15) / 16;
    p.ksteps_max = p.ksteps <= 4 ? 4 : (p.ksteps <= 8 ? 8 : 16);
    p.nblocks = (n + kRowBlock - 1) / kRowBlock;
    p.nsplit = kSplits;
    const int bps = (p.nblocks + p.nsplit - 1) / p.nsplit;
    p.rows_per_split = bps * kRowBlock;
    p.qpad = (nq + kQueryTile - 1) / kQueryTile * kQueryTile;
    p.nqt = p.qpad / kQueryTile;
    p.ngroups = (nq + kGroup - 1) / kGroup;
    return p;
}

}  // namespace dvf
}  // namespace gfxknn
