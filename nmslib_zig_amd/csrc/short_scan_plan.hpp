// The short scan of the exact f32 path (DESIGN 4.1b "short scan"): a filter on the first 64 columns of the rows and queries
// rotated by the eigenvectors of the rows' second-moment matrix.  What finalize decides on the host is here, without HIP:
// the rotation (a cyclic Jacobi sweep), the constants of the error bound E_s, the index gate.  The kernels restate
// short_error() term for term (bf_kernels.hip, bf_f32_prep_short_kernel).
//
// The bound.  Vh = the first 64 columns of V as stored (f32, orthogonal only up to rounding), bh = the row's computed head
// (any 64 numbers), tb = b - Vh bh its exact reconstruction residual; qh, tq likewise for a query.  Then, exactly,
//     q.b - qh.bh = (Vh^T q - qh).bh + qh.(Vh^T tb) + tq.tb
// The last term is at most |tq||tb| (Cauchy-Schwarz): the tier's price.  The first two are rounding terms:
//   - a head is 64 f32 dot products of `dim` terms: |computed - exact| <= g |x| |v_j| per column, g = gamma(dim) -- in
//     norm  g |x| |Vh|_F;
//   - Vh^T tb = (I - Vh^T Vh) Vh^T b - Vh^T Vh eb  with eb the row head's rounding error: at most
//     delta nu |b| + (1 + delta) g |b| |Vh|_F, delta = |Vh^T Vh - I|_F, nu = sqrt(1 + delta) >= |Vh|_2.
// With |bh|, |qh| <= nu (1 + g |Vh|_F) |x| the two sum to at most  coeff |q||b|,
//     coeff = nu (1 + g F) (g F + delta nu + (1 + delta) g F),   F = |Vh|_F,
// which Rotation::coeff holds with a margin of 1 %, from delta and F MEASURED on the stored f32 matrix in f64.
// The tails are measured in f32 from the reconstruction, whose own rounding (64 fma per element on |x_i| + sum |h_j||V_ij|)
// is at most  gamma(65) (1 + nu F (1 + g F)) |x|  in norm: tail_allowance() adds it, and 2^-20 relative for the norm's sum.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SHORT_SCAN_HD __host__ __device__
#else
#define SHORT_SCAN_HD
#endif

namespace gfxknn {
namespace shortscan {

constexpr int kHead = 64;           // columns of the rotated rows the filter keeps (P)
constexpr int kMaxDim = 128;        // one chunk of the one-product scan
constexpr int kMaxSample = 1 << 16; // rows of the second-moment sample
constexpr float kGate = 1.0f / 16;  // index gate: largest tail <= kGate * largest row norm

// Eigenvectors of the symmetric n x n matrix a (row-major, destroyed) by cyclic Jacobi sweeps in f64.  v (row-major,
// n x n): column j is the eigenvector of eig[j]; columns sorted by falling eigenvalue.  Returns the sweeps taken.
inline int jacobi_eigen(std::vector<double>& a, int n, std::vector<double>& v, std::vector<double>& eig) {
    v.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
    auto A = [&](int i, int j) -> double& { return a[(size_t)i * n + j]; };
    int sweep = 0;
    for (; sweep < 64; ++sweep) {
        double off = 0, diag = 0;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) (i == j ? diag : off) += A(i, j) * A(i, j);
        if (off <= 1e-30 * diag || off == 0) break;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                const double apq = A(p, q);
                if (apq == 0) continue;
                const double theta = (A(q, q) - A(p, p)) / (2 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
                const double c = 1 / std::sqrt(t * t + 1), s = t * c;
                for (int k = 0; k < n; ++k) {   // columns p, q of A
                    const double akp = A(k, p), akq = A(k, q);
                    A(k, p) = c * akp - s * akq;
                    A(k, q) = s * akp + c * akq;
                }
                for (int k = 0; k < n; ++k) {   // rows p, q of A
                    const double apk = A(p, k), aqk = A(q, k);
                    A(p, k) = c * apk - s * aqk;
                    A(q, k) = s * apk + c * aqk;
                }
                for (int k = 0; k < n; ++k) {
                    const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
                    v[(size_t)k * n + p] = c * vkp - s * vkq;
                    v[(size_t)k * n + q] = s * vkp + c * vkq;
                }
            }
    }
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return A(x, x) > A(y, y); });
    std::vector<double> vs((size_t)n * n);
    eig.resize(n);
    for (int j = 0; j < n; ++j) {
        eig[j] = A(order[j], order[j]);
        for (int i = 0; i < n; ++i) vs[(size_t)i * n + j] = v[(size_t)i * n + order[j]];
    }
    v.swap(vs);
    return sweep;
}

// What the kernels need of the rotation: Vh as f32 [kMaxDim][kHead] (rows >= dim are zero) and the constants of the bound
struct Rotation {
    std::vector<float> vh;
    double delta = 0, frob = 0;   // |Vh^T Vh - I|_F and |Vh|_F of the stored matrix
    float coeff = 0;              // rounding terms of the bound: coeff |q||b|
    float tail_abs = 0;           // the tails' own f32 allowance: tail_abs |x|
};

inline double gamma_of(int terms) {
    const double u = std::ldexp(1.0, -24);
    return terms * u / (1 - terms * u);
}

// second moment m (dim x dim, row-major, f64; destroyed) -> the rotation
inline Rotation make_rotation(std::vector<double>& m, int dim) {
    Rotation r;
    std::vector<double> v, eig;
    jacobi_eigen(m, dim, v, eig);
    r.vh.assign((size_t)kMaxDim * kHead, 0.f);
    for (int i = 0; i < dim; ++i)
        for (int j = 0; j < kHead && j < dim; ++j) r.vh[(size_t)i * kHead + j] = (float)v[(size_t)i * dim + j];
    double d2 = 0, f2 = 0;
    for (int a = 0; a < kHead; ++a)
        for (int b = 0; b < kHead; ++b) {
            double s = 0;
            for (int i = 0; i < dim; ++i) s += (double)r.vh[(size_t)i * kHead + a] * (double)r.vh[(size_t)i * kHead + b];
            const double e = s - (a == b ? 1.0 : 0.0);
            d2 += e * e;
            if (a == b) f2 += s;
        }
    r.delta = std::sqrt(d2);
    r.frob = std::sqrt(f2);
    const double g = gamma_of(dim), F = r.frob, nu = std::sqrt(1 + r.delta);
    r.coeff = (float)(1.01 * nu * (1 + g * F) * (g * F + r.delta * nu + (1 + r.delta) * g * F));
    r.tail_abs = (float)(1.01 * gamma_of(kHead + 1) * (1 + nu * F * (1 + g * F)));
    return r;
}

// The narrow tier: a head of the first kHeadNarrow columns.  The columns are sorted by falling eigenvalue, so the narrow Vh is
// the PREFIX of the stored one (row stride kHead) and no second matrix exists.  The derivation above holds with 32 in place
// of 64 throughout: delta and F measured on the stored prefix, 32 fma per element of the reconstruction (gamma(33)).
constexpr int kHeadNarrow = 32;
struct HeadConstants {
    double delta = 0, frob = 0;
    float coeff = 0, tail_abs = 0;
};
// the constants of the bound for a head of the first `width` columns of r.vh (width = kHead: Rotation's own, bit for bit)
inline HeadConstants head_constants(const Rotation& r, int dim, int width) {
    HeadConstants c;
    double d2 = 0, f2 = 0;
    for (int a = 0; a < width; ++a)
        for (int b = 0; b < width; ++b) {
            double s = 0;
            for (int i = 0; i < dim; ++i) s += (double)r.vh[(size_t)i * kHead + a] * (double)r.vh[(size_t)i * kHead + b];
            const double e = s - (a == b ? 1.0 : 0.0);
            d2 += e * e;
            if (a == b) f2 += s;
        }
    c.delta = std::sqrt(d2);
    c.frob = std::sqrt(f2);
    const double g = gamma_of(dim), F = c.frob, nu = std::sqrt(1 + c.delta);
    c.coeff = (float)(1.01 * nu * (1 + g * F) * (g * F + c.delta * nu + (1 + c.delta) * g * F));
    c.tail_abs = (float)(1.01 * gamma_of(width + 1) * (1 + nu * F * (1 + g * F)));
    return c;
}

// a measured tail and the norm of its vector -> an upper bound of the true tail
SHORT_SCAN_HD inline float tail_allowance(float tail, float norm, float tail_abs) {
    return tail * (1.0f + 9.6e-7f) + tail_abs * norm;
}

inline bool index_gate(float b_tailmax, float bmax) { return bmax > 0.f && b_tailmax <= kGate * bmax; }

// E_s of one query in the scan's units.  e_head: one_product_error over the head parts (already in those units);
// unit = scale_rows * scale_queries; q_tail, b_tailmax: with their allowances; qn, bmax: the norms of the query and of the
// longest row.  (The products are rounded up by 2^-20: three f32 operations.)
SHORT_SCAN_HD inline float short_error(float e_head, float unit, float q_tail, float b_tailmax, float qn, float bmax, float coeff) {
    return e_head + 1.000001f * unit * (q_tail * b_tailmax + coeff * qn * bmax);
}

}  // namespace shortscan
}  // namespace gfxknn
