// 8-bit quantisation of f32 rows and queries for the l1 filter scan, with the bound that ties the
// scan's sum of absolute byte differences (SAD) back to the l1 distance.  Header-only and free of HIP, so that a plain host
// program can include it; under hipcc the per-element functions are also callable on the device, where the copy is made
// from the rows already in HBM.
//
// One step s serves the whole index (SAD weighs all bytes alike), one offset lo_c per column (SAD does not see offsets):
//     byte(x, c) = rint((x - lo_c) / s),   s = max_c (hi_c - lo_c) / 255,   lo_c / hi_c = column minimum / maximum.
// All arithmetic is f64 on f32 inputs; s is the f64 value, exactly.  In real numbers, with residuals
// x = lo_c + s * byte + rho:
//     | L1(q, b) - X_q - s * SAD(q^, b^) |  <=  E_q          for every stored row b,
//     X_q = sum_c |q_c - clamp(q_c, lo_c, hi_c)|,   E_q = sum_c (|rho(clamp q_c)| + rmax_c),   rmax_c >= |rho(b_c)|.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define L1Q_HD __host__ __device__
#else
#define L1Q_HD
#endif

namespace gfxknn {
namespace l1q {

// The common step of columns spanning at most `max_range` (= max_c hi_c - lo_c, taken in f64).  ok = false: the path is
// declined (constant data, a range whose step is no normal float, or no finite range at all).
inline double step_of(double max_range, bool* ok) {
    const double s = max_range / 255.0;
    const float sf = (float)s;
    *ok = std::isfinite(sf) && sf >= 1.17549435e-38f;
    return s;
}
// max_c (hi_c - lo_c); NaN or inf when a column holds a non-finite value
inline double max_range(const float* lo, const float* hi, size_t dim) {
    double r = 0;
    for (size_t c = 0; c < dim; ++c) {
        const double d = (double)hi[c] - (double)lo[c];
        if (!(d <= r)) r = d;   // (a NaN range sticks)
    }
    return r;
}

// byte of x in a column starting at lo; x inside [lo, hi] lands in 0..255 by construction, anything else (a query that was
// not clamped, NaN) is forced there
L1Q_HD inline uint8_t quantise(float x, float lo, double s) {
    const double v = std::rint(((double)x - (double)lo) / s);
    if (!(v >= 0.0)) return 0;
    return v > 255.0 ? (uint8_t)255 : (uint8_t)v;
}
// |x - (lo + s * byte)| in f64, plus what the f64 evaluation itself may have lost: an upper bound of the real residual
L1Q_HD inline double residual(float x, float lo, double s, uint8_t byte) {
    const double back = (double)lo + s * (double)byte;
    const double mag = std::fabs((double)lo) + std::fabs(back) + std::fabs((double)x);
    return std::fabs((double)x - back) + mag * 8.8817841970012523e-16;   // 2^-50
}
// the smallest float that is not below r (r >= 0)
L1Q_HD inline float round_up_f32(double r) {
    float f = (float)r;
    if ((double)f < r) f = std::nextafterf(f, INFINITY);
    return f;
}
L1Q_HD inline float clampf(float q, float lo, float hi) { return q < lo ? lo : (q > hi ? hi : q); }

// One query: bytes [dim], the excess X_q and the bound E_q.  E is an upper bound of its real value; X is a plain f64 sum,
// whose rounding (relative 2^-50 at most) lies inside the slack of the proof's comparison, see filter_floor.
// A NaN element makes X and E NaN: the proof's comparison then fails and the query is served by the fallback.
L1Q_HD inline void query(const float* q, const float* lo, const float* hi, const float* rmax, size_t dim, double s,
                         uint8_t* bytes, double* X, double* E) {
    double x = 0, e = 0;
    for (size_t c = 0; c < dim; ++c) {
        const float qc = clampf(q[c], lo[c], hi[c]);
        x += std::fabs((double)q[c] - (double)qc);
        bytes[c] = quantise(qc, lo[c], s);
        e += residual(qc, lo[c], s, bytes[c]) + (double)rmax[c];
    }
    *X = x;
    *E = e * (1.0 + 2.2737367544323206e-13);   // (the sum's own rounding: dim * 2^-53 << 2^-42)
}

// Relative error of the exact f32 l1 distance (wave_exact_distance_f32, SP_L1, up to 256 dimensions: at most four
// terms per lane and six levels of the wave sum, each rounding 2^-24) -- 2^-20 with room to spare.
constexpr double kF32SumSlack = 9.5367431640625e-07;

// Lower bound of the f32 distance the exact re-rank returns for a row whose SAD is at least `sad`:
// (X + s * sad - E) (1 - 2^-20), less the rounding of this expression itself.  A row can be left out of the re-rank
// when this is STRICTLY above the k-th exact distance (ties are ordered by position, so equality proves nothing).
L1Q_HD inline double filter_floor(double X, double E, double s, uint32_t sad) {
    const double t = s * (double)sad;
    return (X + t - E) * (1.0 - kF32SumSlack) - (X + t + E) * 9.094947017729282e-13;   // 2^-40
}

// Host reference of finalize: column ranges, bytes [n][dim] and rmax [dim] of rows [n][ld].  false: declined.
inline bool quantise_rows(const float* rows, size_t n, size_t dim, size_t ld, float* lo, float* hi, double* s, uint8_t* bytes,
                          float* rmax) {
    if (n == 0 || dim == 0) return false;
    for (size_t c = 0; c < dim; ++c) lo[c] = INFINITY, hi[c] = -INFINITY;
    for (size_t i = 0; i < n; ++i)
        for (size_t c = 0; c < dim; ++c) {
            const float x = rows[i * ld + c];
            if (!std::isfinite(x)) return false;
            lo[c] = x < lo[c] ? x : lo[c];
            hi[c] = x > hi[c] ? x : hi[c];
        }
    bool ok = false;
    *s = step_of(max_range(lo, hi, dim), &ok);
    if (!ok) return false;
    for (size_t c = 0; c < dim; ++c) rmax[c] = 0.f;
    for (size_t i = 0; i < n; ++i)
        for (size_t c = 0; c < dim; ++c) {
            const float x = rows[i * ld + c];
            const uint8_t b = quantise(x, lo[c], *s);
            bytes[i * dim + c] = b;
            const float r = round_up_f32(residual(x, lo[c], *s, b));
            rmax[c] = r > rmax[c] ? r : rmax[c];
        }
    return true;
}

}  // namespace l1q
}  // namespace gfxknn
