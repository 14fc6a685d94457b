// Packing of f32 rows into the 8-bit traversal copy of the HNSW search: one power-of-two scale per index,
// round-to-nearest-even codes in [-127, 127] and, behind the codes of a row, the sum of their squares.  Header-only and free
// of HIP, so that a plain host program can include it; under hipcc the conversion is also callable on the device, where the
// copy is made from the rows already in HBM and where the walk kernel codes its query.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define Q8PACK_HD __host__ __device__
#else
#define Q8PACK_HD
#endif

namespace gfxknn {
namespace q8pack {

// Exponent e of the unit 2^e that puts the largest |element| into [64, 128) code units: up to one bit below what max / 127
// would give, and in exchange values on a small integer grid (times any power of two) are their own codes.  0 for rows that
// are all zero or hold no finite maximum.  (|e| <= 100: the unit and its inverse stay normal floats.)
inline int scale_exp(float max_abs) {
    if (!(max_abs > 0.f) || !std::isfinite(max_abs)) return 0;
    int ex = 0;
    (void)std::frexp(max_abs, &ex);  // max_abs in [2^(ex-1), 2^ex)
    const int e = ex - 7;
    return e < -100 ? -100 : (e > 100 ? 100 : e);
}
inline float inv_unit_of(int e) { return std::ldexp(1.f, -e); }

// x already divided by the unit -> its code: round to nearest even, clamped to [-127, 127]; NaN -> 0
Q8PACK_HD inline int code(float x) {
    if (!(x == x)) return 0;
    const float c = x < -127.f ? -127.f : (x > 127.f ? 127.f : x);
    return (int)__builtin_rintf(c);
}

// codes per row, zero padded so that a row is whole 16-byte loads; the row stride adds the 16-byte slot of the sum
inline size_t codes_stride(size_t dim) { return (dim + 15) & ~(size_t)15; }
inline size_t row_stride(size_t dim) { return codes_stride(dim) + 16; }

// dst row i = the codes of src row i / 2^e, zeros up to codes_stride, then the int32 sum of the squared codes and 12 zero bytes
inline void pack_rows(const float* src, size_t n, size_t dim, size_t ld_src, int e, int8_t* dst) {
    const size_t lc = codes_stride(dim), ld = lc + 16;
    const float inv = inv_unit_of(e);
    for (size_t i = 0; i < n; ++i) {
        int32_t ss = 0;
        for (size_t d = 0; d < dim; ++d) {
            const int c = code(src[i * ld_src + d] * inv);
            dst[i * ld + d] = (int8_t)c;
            ss += c * c;
        }
        for (size_t d = dim; d < ld; ++d) dst[i * ld + d] = 0;
        __builtin_memcpy(dst + i * ld + lc, &ss, 4);
    }
}

}  // namespace q8pack
}  // namespace gfxknn
