// The bit_jaccard distance from its two exact counts, shared by every kernel that reports one (the scan, the range and
// pair kernels of jaccard_kernels.hip and the matrix-core scan's out-of-line path), so that all of them give the same bits.
#pragma once
#include "common_dev.hpp"

namespace gfxknn {

// num = |a & b|, den = |a | b|, both below 2^24 and so exact in f32.  SpaceBitJaccard (include/distcomp.h:227-237) in
// dist_t = float arithmetic: one correctly rounded division, one subtraction.  (__fdiv_rn is a plain division to this
// toolchain: the Makefile pins -fhip-fp32-correctly-rounded-divide-sqrt for the objects that include this.)  Two empty
// codes (den = 0; the reference divides 0 by 0) are identical sets: distance 0.
__device__ __forceinline__ float jac_distance(int num, int den) {
    return den == 0 ? 0.0f : 1.0f - __fdiv_rn((float)num, (float)den);
}

// A distance in [0, 1] orders as its bit pattern does (1 - x with x <= 1 never gives -0 under round-to-nearest)
struct JacKeyToDist {
    __device__ float operator()(uint32_t hi) const { return __uint_as_float(hi); }
};

}  // namespace gfxknn
