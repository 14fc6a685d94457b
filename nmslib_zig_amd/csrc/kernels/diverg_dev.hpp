// The divergence formulas of one (obj1, obj2) pair on the device, shared by the exact scan (diverg_kernels.hip) and the
// re-rank of the MFMA filter scan (diverg_mfma_kernels.hip): one summation order, hence one set of bits.
//
// Summation order of one pair (DivAcc), the same in every kernel, tile, split and batch:
//   KL / generalized KL / Itakura-Saito "fast": the reference's SSE order -- four running sums over i mod 4 for
//     i < 4*floor(D/4) with product and sum rounded separately, combined ((s0 + s1) + s2) + s3, then the last D mod 4
//     elements one by one as the reference's build evaluates them (clang contracts a*b + c of one expression: FMA).
//     Itakura-Saito multiplies by the rounded reciprocal of obj2 instead of dividing (at most 1.5 ulp per quotient).
//   kldivgenslow, Jensen-Shannon: one running sum (JS: two) over i = 0 .. D-1, the reference's loops.
// Files that include this are compiled with -ffp-contract=off; the FMAs are explicit.
#pragma once
#include "common_dev.hpp"

namespace gfxknn {

typedef float f32x2 __attribute__((ext_vector_type(2)));

enum DivergFormula : int { DV_KL, DV_KLGEN, DV_KLGEN_SLOW, DV_IS, DV_JS };

constexpr float kFltMin = 1.17549435e-38f;  // numeric_limits<float>::min()

// Accumulators of one pair: obj1 = (x, lx), obj2 = (y, ly, iy = 1 / y)
template <int F>
struct DivAcc {
    f32x2 s01 = {0.f, 0.f}, s23 = {0.f, 0.f};  // running sums of elements i mod 4 = 0, 1 and 2, 3 (packed f32 math)
    float r = 0.f, r2 = 0.f;                   // the sequential sums; after combine() the pair's sum

    __device__ __forceinline__ void seq(float x, float lx, float y, float ly) {
        if constexpr (F == DV_KLGEN_SLOW) {  // KLGeneralStandard, distcomp_bregman.cc:277-286
            r = r + (fmaf(x, logf(x / y), y) - x);
        } else {  // JSStandard / JSPrecomp, distcomp_js.cc:47-87
            r = r + (x * lx + y * ly);
            const float m = 0.5f * (x + y);
            if (m >= kFltMin) r2 = r2 + m * logf(m);
        }
    }

    // elements 4g .. 4g+3 of a complete group
    __device__ __forceinline__ void group(f32x4 x, f32x4 lx, f32x4 y, f32x4 ly, f32x4 iy) {
        if constexpr (F == DV_KL) {  // KLPrecompSIMD, distcomp_bregman.cc:213-273
            s01 = s01 + x.xy * (lx.xy - ly.xy);
            s23 = s23 + x.zw * (lx.zw - ly.zw);
        } else if constexpr (F == DV_KLGEN) {  // KLGeneralPrecompSIMD, :325-393
            s01 = (s01 + x.xy * (lx.xy - ly.xy)) + (y.xy - x.xy);
            s23 = (s23 + x.zw * (lx.zw - ly.zw)) + (y.zw - x.zw);
        } else if constexpr (F == DV_IS) {  // ItakuraSaitoPrecompSIMD, :80-146
            s01 = s01 + (x.xy * iy.xy - (lx.xy - ly.xy));
            s23 = s23 + (x.zw * iy.zw - (lx.zw - ly.zw));
        } else {
            seq(x.x, lx.x, y.x, ly.x);
            seq(x.y, lx.y, y.y, ly.y);
            seq(x.z, lx.z, y.z, ly.z);
            seq(x.w, lx.w, y.w, ly.w);
        }
    }

    // after the last complete group
    __device__ __forceinline__ void combine() {
        if constexpr (F == DV_KL || F == DV_KLGEN || F == DV_IS) r = ((s01.x + s01.y) + s23.x) + s23.y;
    }

    // one of the last D mod 4 elements
    __device__ __forceinline__ void tail(float x, float lx, float y, float ly, float iy) {
        if constexpr (F == DV_KL) r = fmaf(x, lx - ly, r);
        else if constexpr (F == DV_KLGEN) r = r + (fmaf(x, lx - ly, y) - x);
        else if constexpr (F == DV_IS) r = r + (x * iy - (lx - ly));
        else seq(x, lx, y, ly);
    }

    __device__ __forceinline__ float finish(int D, int metr) const {
        if constexpr (F == DV_IS) return r - (float)D;
        if constexpr (F == DV_JS) {
            const float v = 0.5f * r - r2;
            const float c = v < 0.0f ? 0.0f : v;  // std::max(v, 0)
            return metr ? sqrtf(c) : c;           // space_js.h:99-101
        }
        return r;
    }
};

// the last D mod 4 elements, held in one (partial) group
template <int F>
__device__ __forceinline__ void tail_group(DivAcc<F>& a, int rem, f32x4 x, f32x4 lx, f32x4 y, f32x4 ly, f32x4 iy) {
    if (rem > 0) a.tail(x.x, lx.x, y.x, ly.x, iy.x);
    if (rem > 1) a.tail(x.y, lx.y, y.y, ly.y, iy.y);
    if (rem > 2) a.tail(x.z, lx.z, y.z, ly.z, iy.z);
}

// formula(obj1 = a, obj2 = b): group g of an object at p[g * stride]; the reciprocals of obj2 are taken here
template <int F>
__device__ __forceinline__ float diverg_eval(int D, const f32x4* av, const f32x4* al, size_t sa, const f32x4* bv,
                                             const f32x4* bl, size_t sb, int metr) {
    DivAcc<F> acc;
    const int G4 = D >> 2, rem = D & 3;
    for (int g = 0; g < G4; ++g) {
        const f32x4 y = bv[g * sb];
        acc.group(av[g * sa], al[g * sa], y, bl[g * sb], 1.0f / y);
    }
    acc.combine();
    if (rem) {
        const f32x4 y = bv[G4 * sb];
        f32x4 iy = {1.0f / y.x, rem > 1 ? 1.0f / y.y : 0.f, rem > 2 ? 1.0f / y.z : 0.f, 0.f};
        tail_group<F>(acc, rem, av[G4 * sa], al[G4 * sa], y, bl[G4 * sb], iy);
    }
    return acc.finish(D, metr);
}

}  // namespace gfxknn
