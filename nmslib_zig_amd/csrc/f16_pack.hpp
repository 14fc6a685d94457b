// Packing of f32 rows into the fp16 traversal copy of the HNSW search: one power-of-two scale per index and
// round-to-nearest-even conversion.  Header-only and free of HIP, so that a plain host program can include it; under hipcc
// the conversion is also callable on the device, where the copy is made from the rows already in HBM.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define F16PACK_HD __host__ __device__
#else
#define F16PACK_HD
#endif

namespace gfxknn {
namespace f16pack {

// Exponent e of the scale 2^e that puts the largest |element| into [2^14, 2^15): a factor 2 below fp16's largest finite
// value (65504), and as far above its subnormal range (below 2^-14) as the format allows.  0 for rows that are all zero
// or hold no finite maximum.  (|e| <= 100: the scale and its inverse stay normal floats.)
inline int scale_exp(float max_abs) {
    if (!(max_abs > 0.f) || !std::isfinite(max_abs)) return 0;
    int ex = 0;
    (void)std::frexp(max_abs, &ex);  // max_abs in [2^(ex-1), 2^ex)
    const int e = 15 - ex;
    return e < -100 ? -100 : (e > 100 ? 100 : e);
}
inline float scale_of(int e) { return std::ldexp(1.f, e); }

// f32 -> fp16 bits, round to nearest even (overflow -> inf, NaN stays NaN, fp16 subnormals are produced)
F16PACK_HD inline uint16_t round_f16(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7FFFFFFFu;
    if (u >= 0x7F800000u) return (uint16_t)(sign | (u > 0x7F800000u ? 0x7E00u : 0x7C00u));
    if (u >= 0x47800000u) return (uint16_t)(sign | 0x7C00u);  // >= 2^16
    if (u < 0x38800000u) {                                    // below 2^-14: an fp16 subnormal, h * 2^-24
        if (u < 0x33000000u) return (uint16_t)sign;           // below 2^-25: zero
        const int shift = 126 - (int)(u >> 23);               // 14 .. 24
        const uint32_t m = (u & 0x7FFFFFu) | 0x800000u;
        uint32_t h = m >> shift;
        const uint32_t rem = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
        if (rem > half || (rem == half && (h & 1u))) ++h;
        return (uint16_t)(sign | h);
    }
    uint32_t h = (u - 0x38000000u) >> 13;  // exponent re-biased (127 -> 15), 10 mantissa bits kept
    const uint32_t rem = u & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (h & 1u))) ++h;  // (a carry into the exponent is the right result, up to inf)
    return (uint16_t)(sign | h);
}

// dst[i][d] = fp16(scale * src[i][d]) for d < dim, zero for dim <= d < ld_dst
inline void pack_rows(const float* src, size_t n, size_t dim, size_t ld_src, float scale, uint16_t* dst, size_t ld_dst) {
    for (size_t i = 0; i < n; ++i) {
        for (size_t d = 0; d < dim; ++d) dst[i * ld_dst + d] = round_f16(scale * src[i * ld_src + d]);
        for (size_t d = dim; d < ld_dst; ++d) dst[i * ld_dst + d] = 0;
    }
}

// halves per row of the copy: rows start on 16-byte boundaries
inline size_t row_stride(size_t dim) { return (dim + 7) & ~(size_t)7; }

}  // namespace f16pack
}  // namespace gfxknn
