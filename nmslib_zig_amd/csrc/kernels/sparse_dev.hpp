// The sparse distance of one pair, shared by the exact scan (sparse_kernels.hip) and the inverted-file path's re-rank
// (sparse_inv_kernels.hip): one copy of the formula, hence one set of bits.
//
// The reference's sparse distance (ComputeDistanceHelper, include/space/space_sparse_vector.h:137-215) merges the two
// sorted id lists into union order, writes 0 for an id missing on one side, and calls the DENSE function on the two
// union arrays; sparse_kernels.hip describes how UnionAcc restates that.  Translation units that include this header
// are compiled with -ffp-contract=off; the tails' FMAs are explicit.
#pragma once
#include "common_dev.hpp"

namespace gfxknn {

constexpr float kEps = 1.17549435e-38f * 2.0f;  // numeric_limits<float>::min() * 2

// Accumulators of one pair in union order.  x = value of obj1, y = value of obj2 (0 where the id is missing).
template <int SP>
struct UnionAcc {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;  // L2: (x-y)^2, L1: |x-y|, dot: x*y, cosine: x*y
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;  // cosine: x*x  (query-norm: sequential x*x)
    float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f;  // cosine: y*y  (query-norm: sequential y*y)
    float px0 = 0.f, px1 = 0.f, px2 = 0.f, py0 = 0.f, py1 = 0.f, py2 = 0.f;  // held-back group
    float m = 0.f;   // Linf: running max (order-independent)
    float qs = 0.f;  // query-norm: sequential sum of x*y
    int c = 0;       // positions in the held-back group

    __device__ __forceinline__ static void lane(float x, float y, float& a, float& b, float& cc) {
        if constexpr (SP == SP_L2) {
            const float d = x - y;
            a = a + d * d;
        } else if constexpr (SP == SP_L1) {
            a = a + fabsf(x - y);
        } else if constexpr (SP == SP_NEGDOT) {
            a = a + x * y;
        } else {  // cosine / angular
            a = a + x * y;
            b = b + x * x;
            cc = cc + y * y;
        }
    }

    __device__ __forceinline__ void push(float x, float y) {
        if constexpr (SP == SP_LINF) {
            const float d = fabsf(x - y);
            m = m > d ? m : d;
        } else if constexpr (SP == SP_QNORM_NEGDOT) {
            // QueryNormScalarProduct (src/distcomp_scalar.cc:64-79): one sequential loop, contracted
            b0 = fmaf(x, x, b0);
            c0 = fmaf(y, y, c0);
            qs = fmaf(x, y, qs);
        } else {
            if (c == 3) {
                lane(px0, py0, a0, b0, c0);
                lane(px1, py1, a1, b1, c1);
                lane(px2, py2, a2, b2, c2);
                lane(x, y, a3, b3, c3);
            } else {
                px0 = c == 0 ? x : px0;
                py0 = c == 0 ? y : py0;
                px1 = c == 1 ? x : px1;
                py1 = c == 1 ? y : py1;
                px2 = c == 2 ? x : px2;
                py2 = c == 2 ? y : py2;
            }
            c = (c + 1) & 3;
        }
    }

    // fwd = distance(obj1, obj2), rev = distance(obj2, obj1)
    __device__ __forceinline__ void finish(float& fwd, float& rev) const {
        if constexpr (SP == SP_LINF) {
            fwd = rev = m;
        } else if constexpr (SP == SP_QNORM_NEGDOT) {
            // -QueryNormScalarProduct(p1, p2): normalised by the norm of the SECOND argument
            fwd = -(qs / sqrtf(fmaxf(c0, kEps)));
            rev = -(qs / sqrtf(fmaxf(b0, kEps)));
        } else if constexpr (SP == SP_L1) {
            double r = (double)(((a0 + a1) + a2) + a3);  // distcomp_lp.cc:190-251: float lanes, double tail
            if (c > 0) r += (double)fabsf(px0 - py0);
            if (c > 1) r += (double)fabsf(px1 - py1);
            if (c > 2) r += (double)fabsf(px2 - py2);
            fwd = rev = (float)r;
        } else if constexpr (SP == SP_L2) {
            float r = ((a0 + a1) + a2) + a3;  // distcomp_lp.cc:304-371
            float d;
            if (c > 0) { d = px0 - py0; r = fmaf(d, d, r); }
            if (c > 1) { d = px1 - py1; r = fmaf(d, d, r); }
            if (c > 2) { d = px2 - py2; r = fmaf(d, d, r); }
            fwd = rev = sqrtf(r);
        } else if constexpr (SP == SP_NEGDOT) {
            float r = ((a0 + a1) + a2) + a3;  // distcomp_scalar.cc:193-245
            if (c > 0) r = fmaf(px0, py0, r);
            if (c > 1) r = fmaf(px1, py1, r);
            if (c > 2) r = fmaf(px2, py2, r);
            fwd = rev = -r;
        } else {  // NormScalarProductSIMD, distcomp_scalar.cc:83-168
            float s = ((a0 + a1) + a2) + a3;
            float n1 = ((b0 + b1) + b2) + b3;
            float n2 = ((c0 + c1) + c2) + c3;
            if (c > 0) { s = fmaf(px0, py0, s); n1 = fmaf(px0, px0, n1); n2 = fmaf(py0, py0, n2); }
            if (c > 1) { s = fmaf(px1, py1, s); n1 = fmaf(px1, px1, n1); n2 = fmaf(py1, py1, n2); }
            if (c > 2) { s = fmaf(px2, py2, s); n1 = fmaf(px2, px2, n1); n2 = fmaf(py2, py2, n2); }
            float vf = 0.f, vr = 0.f;
            if (!(n1 < kEps || n2 < kEps)) {
                vf = s / sqrtf(n1) / sqrtf(n2);
                vr = s / sqrtf(n2) / sqrtf(n1);
                vf = fmaxf(-1.0f, fminf(1.0f, vf));
                vr = fmaxf(-1.0f, fminf(1.0f, vr));
            }
            if constexpr (SP == SP_ANGULAR) {  // AngularDistance, distcomp_scalar.cc:254-258
                fwd = acosf(vf);
                rev = acosf(vr);
            } else {  // CosineSimilarity, distcomp_scalar.cc:267-271
                fwd = fmaxf(0.0f, 1.0f - vf);
                rev = fmaxf(0.0f, 1.0f - vr);
            }
        }
    }
};

// One pair, obj1 = (ia, va, na), obj2 = (ib, vb, nb), merged in union order (space_sparse_vector.h:170-200).
template <int SP>
__device__ __forceinline__ void sparse_pair(const uint32_t* ia, const float* va, int na, const uint32_t* ib,
                                            const float* vb, int nb, float& fwd, float& rev) {
    UnionAcc<SP> acc;
    int i = 0, j = 0;
    while (i < na && j < nb) {
        const uint32_t a = ia[i], b = ib[j];
        const float xa = va[i], yb = vb[j];
        const bool ta = a <= b, tb = b <= a;
        acc.push(ta ? xa : 0.f, tb ? yb : 0.f);
        i += ta;
        j += tb;
    }
    for (; i < na; ++i) acc.push(va[i], 0.f);
    for (; j < nb; ++j) acc.push(0.f, vb[j]);
    acc.finish(fwd, rev);
}

}  // namespace gfxknn
