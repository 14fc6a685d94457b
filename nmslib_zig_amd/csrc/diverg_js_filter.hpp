// One-logarithm form of Jensen-Shannon for the hardware-log2 filter scan, with the bound that ties the
// filter's key back to the f32 value the exact scan (DivAcc<DV_JS>, kernels/diverg_dev.hpp) holds before finish()'s clamp and
// square root.  Header-only and free of HIP like diverg_filter.hpp, whose plan type, gates and filter_floor it reuses.
// All arithmetic is f64 on the f32 inputs.
//
// With x the row, y the query, s_i = x_i + y_i and 0 ln 0 = 0, in real numbers
//     JS(x, y) = R_row + C_q - (ln2 / 2) T(x, y),   T = sum s_i log2 s_i
//     R_row = 1/2 sum x ln x + (ln2 / 2) sum x,     C_q = 1/2 sum y ln y + (ln2 / 2) sum y
// (m ln m with m = s / 2 is (s / 2) ln s - (ln2 / 2) s).  The filter takes, over the G = ceil(D / 4) groups of the value plane,
//     s = fl(x + y'),  y' = max(y, 2^-100);  lane sum a_(i mod 4) = fma(s, hwlog2(s), a_(i mod 4));  T^ = ((a0 + a1) + a2) + a3
//     key = fl32(R32 - fl32(ln2 / 2) T^),  R32 = fl32(R_row)
// query() gives C_q and E_q with | key + C_q - v^ | <= E_q for every stored row.
#pragma once
#include "diverg_filter.hpp"

namespace gfxknn {
namespace djs {

// The raw logarithm instruction (v_log_f32) is taken to be within this many ulp of log2, in ulp of its result: what
// tools/probe/hwlog_probe.hip measures over every f32 in [2^-100, 2^128), rounded up to a whole ulp, and not below the 1 ulp
// the ISA manual states.
constexpr double kHwLog2Ulps = 1.0;
constexpr float kClamp = 7.888609052210118e-31f;   // 2^-100: the least query element the filter reads
constexpr double kHalfLn2 = 0.34657359027997264;
constexpr double kLog2E = 1.4426950408889634;
constexpr int kTileQ = 16;      // queries of a workgroup: the exact scan's tile and the group of a fallback flag
constexpr int kRowBlock = 64;   // rows of one step: one per lane

// Largest values over the stored rows, each rounded up to f32: |log2| of a positive element, sum x, sum |x ln x|
struct RowMax {
    float lam, sum, xlnx;
};

// one row: R_row, and its own three figures into m.  *ok goes false at a negative or non-finite element (the index then
// keeps the exact scan).
DVF_HD inline double row(const float* x, size_t dim, RowMax* m, bool* ok) {
    double sx = 0, sl = 0, sa = 0, lam = 0;
    for (size_t j = 0; j < dim; ++j) {
        const double v = x[j];
        if (!(v >= 0) || !std::isfinite(v)) *ok = false;
        if (!(v > 0) || !std::isfinite(v)) continue;
        const double l = std::log(v);
        sx += v, sl += v * l, sa += std::fabs(v * l);
        lam = std::fabs(l) > lam ? std::fabs(l) : lam;
    }
    const double w = 1.0 + 9.094947017729282e-13;   // 2^-40: the f64 logarithms and sums above
    const float v[3] = {dvf::round_up_f32(lam * kLog2E * w), dvf::round_up_f32(sx * w), dvf::round_up_f32(sa * w)};
    m->lam = v[0] > m->lam ? v[0] : m->lam;
    m->sum = v[1] > m->sum ? v[1] : m->sum;
    m->xlnx = v[2] > m->xlnx ? v[2] : m->xlnx;
    return 0.5 * sl + kHalfLn2 * sx;
}

// One query: C_q and E_q (an upper bound of its real value).  Element j of the query is at q[(j / 4) * gs + j % 4].  Zeros are
// legal; E_q is infinite -- no proof -- for a NaN, an infinity or a negative element.
//
// W >= sum |s log2 s| over the 4 G elements the loop reads: |log2(a + b)| <= max(|log2 a|, |log2 b|) + 1, so with lam the
// larger of the rows' and the query's largest |log2| of a positive element, W = (max sum x + sum y')(lam + 1) + 4 G 101 2^-100
// (an element whose query side is the clamp has s in [x, 2 x] or s <= 2^-99).  u = 2^-24.
//   hardware logarithm             (2 kHwLog2Ulps + 1) u W (ln2 / 2): K ulp of a result are at most K 2^-23 of it; one u more,
//                                  so that K ulp may be counted from the correctly rounded logarithm
//   the loop                       s = fl(x + y'): u (W + sum s / ln2);  G fmas into a lane sum and 3 additions: (G + 3) u W
//   key, R32, C_q                  the constant fl32(ln2 / 2) and the key's rounding: 2 u (ln2 / 2) W + u R_abs;
//                                  R32 = fl32(R_row): u R_abs;  R_row and C_q in f64: (2^-40 + D 2^-50)(R_abs + C_abs)
//   exact scan (DivAcc<DV_JS>)     u [(D + 7)(A / 2 + B) + sum m]: a stored or device logf within 2 ulp of the f64 logarithm (4 u),
//                                  2 roundings of a product and a pair sum, D sequential additions, 1 in v^ = 0.5 r - r2;
//                                  m = fl(x + y) / 2 moves m ln m by u m (|ln m| + 1);  A = sum |x ln x| + sum |y ln y|,
//                                  B = (ln2 / 2)(W + sum s) >= sum |m ln m|
//   clamp                          an element moves s log2 s by at most 300 2^-100
//   underflow and the FLT_MIN guards of the exact scan: 1e-30 (1 + D / 1024)
DVF_HD inline void query(const float* q, size_t gs, size_t dim, const RowMax& m, double* C, double* E) {
    double sy = 0, sl = 0, sa = 0, lam = 0;
    bool proof = true;
    for (size_t j = 0; j < dim; ++j) {
        const double v = q[(j >> 2) * gs + (j & 3)];
        proof = proof && v >= 0 && std::isfinite(v);
        if (!(v > 0) || !std::isfinite(v)) continue;
        const double l = std::log(v);
        sy += v, sl += v * l, sa += std::fabs(v * l);
        lam = std::fabs(l) > lam ? std::fabs(l) : lam;
    }
    const double w = 1.0 + 9.094947017729282e-13, u = dvf::kU32;
    const double G = (double)((dim + 3) / 4), c = (double)kClamp;
    lam = lam * kLog2E * w;
    const double ssum = ((double)m.sum + sy) * w + 4.0 * G * c;
    const double W = ssum * ((lam > (double)m.lam ? lam : (double)m.lam) + 1.0) * w + 4.0 * G * 101.0 * c;
    const double Rabs = 0.5 * (double)m.xlnx + kHalfLn2 * (double)m.sum, Cabs = 0.5 * sa + kHalfLn2 * sy;
    double e = kHalfLn2 * 1.001 * u * ((2.0 * kHwLog2Ulps + 1.0) * W + (W + kLog2E * ssum) + (G + 3.0) * W);
    e += 1.001 * u * (2.0 * kHalfLn2 * W + 2.0 * Rabs);
    e += (9.094947017729282e-13 + (double)dim * 8.881784197001252e-16) * (Rabs + Cabs);
    e += 1.001 * u * (((double)dim + 7.0) * (0.5 * ((double)m.xlnx + sa) + kHalfLn2 * (W + ssum)) + 0.5 * ssum);
    e += kHalfLn2 * 4.0 * G * 300.0 * c;
    e = e * w + dvf::kTiny * (1.0 + (double)dim / 1024.0);
    // a sum that could leave f32's range can give an infinite or NaN key, which no list holds: no proof
    proof = proof && W + Rabs < 1e37;
    *C = 0.5 * sl + kHalfLn2 * sy;
    *E = proof ? e : INFINITY;
}

// What the proof compares with the k-th distance, strictly above: a lower bound of the distance finish() returns for a row whose
// filter key is at least key_m.  jsdiv*: dvf::filter_floor (the distance is max(v^, 0) >= v^).  jsmetr*: two JS values can share
// a square root and ties order by position, so the floor goes through the exact scan's own steps: rounded down to f32 (v^ is an
// f32 at or above it), max(., 0), the correctly rounded sqrtf (monotone).  No proof (NaN floor): 0, which is above no distance.
DVF_HD inline double proof_floor(float key_m, double C, double E, int metr) {
    const double fl = dvf::filter_floor(key_m, C, E);
    if (!metr) return fl;
    float f = (float)fl;
    if ((double)f > fl) f = std::nextafterf(f, -INFINITY);
    return (double)sqrtf(f > 0.0f ? f : 0.0f);
}

// The Bregman filter's gates and list shape (kMinRows, kMinQueries, kMaxK, kSplits lists of kKeep keys per query) over rows in
// blocks of 64, one contiguous 1/64 of the blocks per wave, any D.  have: the index holds R32 and the row maxima.
inline dvf::Plan plan(int n, int dim, int nq, int k, bool have) {
    dvf::Plan p{};
    p.use = have && n >= dvf::kMinRows && nq >= dvf::kMinQueries && dim >= 1 && k >= 1 && k <= dvf::kMaxK;
    p.nblocks = (n + kRowBlock - 1) / kRowBlock;
    p.nsplit = dvf::kSplits;
    p.rows_per_split = (p.nblocks + p.nsplit - 1) / p.nsplit * kRowBlock;
    p.qpad = (nq + kTileQ - 1) / kTileQ * kTileQ;
    p.nqt = p.qpad / kTileQ;
    p.ngroups = (nq + dvf::kGroup - 1) / dvf::kGroup;
    return p;
}

}  // namespace djs
}  // namespace gfxknn
