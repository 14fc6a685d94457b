// The inverted-file filter of the sparse inner-product spaces: its plan, the bound that ties the
// filter's score back to the f32 distance the exact scan (UnionAcc, kernels/sparse_dev.hpp) returns, and the floor under
// the distance of every row the filter did not list.  Header-only and free of HIP, so that a plain host program can
// include it; under hipcc the functions are also callable on the device.  All arithmetic is f64.
//
// With q the query (m elements), b a stored row and b' the value the inverted file holds for it
//     kind    space                          b'                   distance of (row, query)
//     DOT     negdotprod_sparse              b                    -(q . b)
//     QNORM   querynorm_negdotprod_sparse    b                    -(q . b) / |q|
//     COS     cosinesimil_sparse             fl32(b / |b|)        max(0, 1 - clamp(q . b / (|q| |b|)))
//     ANG     angulardist_sparse             fl32(b / |b|)        acos(clamp(q . b / (|q| |b|)))
// the filter's score of a row is A = the f32 chain  acc = fma(q_t, b'_t, acc)  over the shared terms t in the query's
// order.  Every one of these distances falls as the inner product rises, so a row whose score is at most T has a
// distance of at least  dist(T + errors): floor_dist().
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define SPF_HD __host__ __device__
#else
#define SPF_HD
#endif

namespace gfxknn {
namespace spf {

enum Kind : int { DOT = 0, QNORM = 1, COS = 2, ANG = 3 };

constexpr int kBlockRows = 16384;   // rows of one block of the inverted file: one f32 accumulator each is 64 KiB of LDS
constexpr int kKeepExtra = 8;       // K' = k + 8 rows are kept per (query, block)
constexpr int kMaxK = 128;
constexpr int kMinRows = 65536;
constexpr int kMaxQueryLen = 4096;  // elements of a query (what the scan stages in LDS, kSparseQCap)
constexpr int kMinQueries = 1;      // measured: the path wins from a batch of one
constexpr int kTermChunk = 1024;    // query terms located and streamed per round of the accumulate kernel

constexpr double kU = 5.9604644775390625e-08;   // 2^-24: unit roundoff of f32
constexpr double kTiny = 1e-30;                 // what underflow can lose in the (at most a few thousand) f32 operations
constexpr double kZeroNorm2 = 2.350988701644575e-38;   // 2 * FLT_MIN: the reference's zero-norm test is n < this
// Squared norms the proof works with.  Below kSafeLo a sum of squares is too close to the zero-norm test and to the
// subnormals for a relative bound; above kSafeHi the f32 sums can overflow.
constexpr double kSafeLo = 1e-30, kSafeHi = 1e30;

SPF_HD inline bool cosine_kind(int kind) { return kind == COS || kind == ANG; }

// ---- rows (finalize) -------------------------------------------------------------------------------------------------
enum RowClass : int { ROW_POSTED = 0, ROW_EMPTY = 1, ROW_DECLINE = 2 };
// norm2: the row's sum of squares in f64.  Cosine family: a row under half the zero-norm threshold gets no postings (the
// reference's test fires for it whatever the rounding of its f32 sum, and its similarity is the 0 the filter then holds);
// a row between that and kSafeLo, or above kSafeHi, makes the index decline the copy.
SPF_HD inline int row_class(int kind, double norm2) {
    if (!cosine_kind(kind)) return ROW_POSTED;
    if (norm2 < 0.5 * kZeroNorm2) return ROW_EMPTY;
    return (norm2 >= kSafeLo && norm2 <= kSafeHi) ? ROW_POSTED : ROW_DECLINE;
}
// the posting's value: the quotient is rounded once
SPF_HD inline float stored_value(int kind, float b, double norm) { return cosine_kind(kind) ? (float)((double)b / norm) : b; }

// the smallest float that is not below r (r >= 0)
SPF_HD inline float round_up_f32(double r) {
    float f = (float)r;
    if ((double)f < r) f = std::nextafterf(f, INFINITY);
    return f;
}

// ---- the bounds ------------------------------------------------------------------------------------------------------
// qnorm = |q|_2, beta >= |b'|_2 of every stored row (both from f64 sums).
//
// E_q: | A - sum q_t b'_t | for any row.  The chain has at most m fused steps, one rounding each, so the error is at most
// gamma_m * sum |q_t b'_t| <= 1.001 m u |q| beta (Cauchy-Schwarz over the shared terms; m u < 1e-3).
SPF_HD inline double filter_err(int m, double qnorm, double beta) { return 1.001 * (double)m * kU * qnorm * beta + kTiny; }

// E_ref: | the scan's f32 inner product of the pair - sum q_t b_t |, relative to |q| |b|.  The union of the two id lists
// has at most L = m + (longest row) positions; a product is rounded once and passes at most L / 4 additions in its lane,
// 3 in the lanes' combination and 3 in the tail (positions with a zero on one side add exact zeros): gamma_(L + 8) covers
// every order.  The same count holds for the two sums of squares of the cosine family.
SPF_HD inline double ref_err_rel(int L) { return 1.001 * ((double)L + 8.0) * kU; }

// Lower bound of the f32 distance the exact scan returns for a row whose filter score is at most T, in a batch query of m
// elements and norm qnorm, less the rounding of this expression itself.  A row can be left out of the re-rank when this
// is STRICTLY above the k-th exact distance (equal distances are ordered by position, so equality proves nothing).  NaN
// when there is no proof: a norm outside [kSafeLo, kSafeHi] (zero-norm and non-finite queries among them), products that
// could leave f32's range.  T = -infinity (every block listed all of its rows): +infinity.
//
//   the row's real sum over the stored values         S' <= T + E_q
//   DOT    d^ >= -S' - E_ref |q| beta
//   QNORM  d^ = -fl(qs / sqrtf(c0)), qs <= S' + E_ref |q| beta; c0 is the query's own f32 sum of squares, within gamma_m of
//          |q|^2, then a root and a quotient: the quotient is within 1.001 (m + 8) u of (that bound) / |q|, relatively
//   COS    b' = b / |b| (1 + d), |d| <= u, so the real cosine c <= S' / |q| + 1.001 u.  The scan's value
//          fl(fl(s / sqrtf(n1)) / sqrtf(n2)) is within E_cos = 1.001 (2 (L + 8) + 8) u + L 1e-15 of c: s within
//          gamma_(L+8) |b||q|, n1 and n2 within gamma_(L+8) relatively (halved by the roots), four more roundings, and what
//          gradual underflow can lose against norms of at least 1e-15.  d^ = max(0, fl(1 - v)) >= 1 - v - 2 u.
//   ANG    the same v; the device's acosf is within 4 ulp of acos (the bound its math library is built to), that is
//          8 u relatively: the floor gives 16 u.
SPF_HD inline double floor_dist(int kind, double T, int m, int L, double qnorm, double beta) {
    const double q2 = qnorm * qnorm;
    if (!(q2 >= kSafeLo && q2 <= kSafeHi) || !(beta >= 0.0 && beta < 1e30) || !(qnorm * beta < 1e37) || T != T || m < 1)
        return NAN;
    if (T == -INFINITY) return INFINITY;
    if (!(T < INFINITY)) return NAN;
    const double hi = T + filter_err(m, qnorm, beta);
    double f;
    if (kind == DOT) {
        f = -hi - ref_err_rel(L) * qnorm * beta;
    } else if (kind == QNORM) {
        const double v = (hi + ref_err_rel(L) * qnorm * beta) / qnorm;
        f = -v - std::fabs(v) * 1.001 * ((double)m + 8.0) * kU - kTiny;
    } else {
        const double e_cos = 1.001 * (2.0 * ((double)L + 8.0) + 8.0) * kU + (double)L * 1e-15;
        const double c = hi / qnorm + 1.001 * kU + e_cos;
        if (kind == COS) {
            f = 1.0 - c - 4.0 * kU;
        } else {
            const double cc = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
            f = std::acos(cc) * (1.0 - 16.0 * kU) - kTiny;
        }
    }
    return f - (std::fabs(f) + 1.0) * 9.094947017729282e-13;   // 2^-40
}

// ---- plan ------------------------------------------------------------------------------------------------------------
struct Plan {
    bool use;
    int nblocks, keep;   // blocks of kBlockRows rows; K' rows kept per (query, block)
};

// kind: of the index's space (-1: not served); max_query_len: the batch's longest query; ascending: every query's ids are
// strictly ascending (a repeated id would be summed twice by the filter and once by the scan's merge)
SPF_HD inline Plan plan(int kind, long long n, long long nq, long long k, long long max_query_len, bool ascending,
                        bool have_copy) {
    Plan p{};
    p.use = kind >= DOT && kind <= ANG && have_copy && n >= kMinRows && n <= 2147483647LL && nq >= kMinQueries &&
            k >= 1 && k <= kMaxK && max_query_len <= kMaxQueryLen && ascending;
    p.nblocks = (int)((n + kBlockRows - 1) / kBlockRows);
    p.keep = (int)(k <= kMaxK ? k : kMaxK) + kKeepExtra;
    return p;
}

}  // namespace spf
}  // namespace gfxknn
