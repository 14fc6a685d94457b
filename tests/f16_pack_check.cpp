// Stand-alone check of nmslib_zig_amd/csrc/f16_pack.hpp (no HIP, no library): tests/test_hnsw_f16_cpu.py builds it with
// -fsanitize=address,undefined, runs it and compares the values it writes with numpy's float16 rounding.
//   argv[1]: output file = uint32 count, then count floats (what was rounded) and count uint16 (the fp16 bits)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../nmslib_zig_amd/csrc/f16_pack.hpp"

using namespace gfxknn;

static int fail(const char* what) {
    std::printf("FAILED: %s\n", what);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 2) return fail("usage: f16_pack_check <out>");
    // rows whose magnitudes span 2^-30 .. 2^30 (every binade), both signs, odd length (the stride pads it)
    const size_t n = 61, dim = 37, ld_src = 40;
    std::vector<float> rows(n * ld_src, 0.f);
    unsigned long long st = 12345;
    auto rnd = [&]() {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(st >> 11) / 9007199254740992.0;
    };
    float max_abs = 0.f;
    for (size_t i = 0; i < n; ++i)
        for (size_t d = 0; d < dim; ++d) {
            const int e = (int)i - 30;  // row i lives in binade 2^e
            float v = (float)std::ldexp(1.0 + rnd(), e);
            if (v > std::ldexp(1.f, 30)) v = std::ldexp(1.f, 30);
            if (rnd() < 0.5) v = -v;
            rows[i * ld_src + d] = v;
            max_abs = std::fmax(max_abs, std::fabs(v));
        }
    const int e = f16pack::scale_exp(max_abs);
    const float scale = f16pack::scale_of(e);
    int ex = 0;
    if (std::frexp(scale, &ex) != 0.5f) return fail("the scale is not a power of two");
    if (f16pack::scale_of(e) * f16pack::scale_of(-e) != 1.f) return fail("the inverse scale is not exact");
    const size_t ld = f16pack::row_stride(dim);
    if (ld % 8 != 0 || ld < dim || ld >= dim + 8) return fail("row stride");
    std::vector<uint16_t> packed(n * ld, 0xFFFF);
    f16pack::pack_rows(rows.data(), n, dim, ld_src, scale, packed.data(), ld);
    std::vector<float> vals;
    std::vector<uint16_t> bits;
    unsigned largest = 0;
    for (size_t i = 0; i < n; ++i)
        for (size_t d = 0; d < ld; ++d) {
            const uint16_t h = packed[i * ld + d];
            if (d >= dim) {
                if (h != 0) return fail("padding is not zero");
                continue;
            }
            if ((h & 0x7C00u) == 0x7C00u) return fail("a packed value is inf or NaN");
            if ((unsigned)(h & 0x7FFFu) > largest) largest = h & 0x7FFFu;
            vals.push_back(scale * rows[i * ld_src + d]);
            bits.push_back(h);
        }
    // fp16 bits of [2^14, 2^15): exponent field 29
    if (largest < 0x7400u || largest >= 0x7800u) return fail("the largest packed value is outside [2^14, 2^15)");
    // all-zero rows and a non-finite maximum leave the scale at 1
    if (f16pack::scale_exp(0.f) != 0 || f16pack::scale_exp(INFINITY) != 0 || f16pack::scale_exp(NAN) != 0) return fail("degenerate scale");
    // extreme maxima: the largest value still lands in [2^14, 2^15) while the exponent is inside the clamp
    for (float m : {3.0e-20f, 1.0f, 65504.f, 7.0e19f})
        if (const float s = m * f16pack::scale_of(f16pack::scale_exp(m)); s < 16384.f || s >= 32768.f) return fail("scale_exp");
    // the rounding itself at its edges: ties, the subnormal range, overflow
    for (float v : {0.f, -0.f, 1.f, 1.00048828125f, 1.0009765625f, 1.00146484375f, 2047.f, 2049.f, 2051.f, 65504.f, 65519.996f,
                    65520.f, 70000.f, 5.9604645e-8f, 2.9802322e-8f, 2.9802326e-8f, 8.9406967e-8f, 6.1035156e-5f, 6.1005e-5f,
                    6.0975552e-5f, 1.0e-9f, -3.3333333f, 0.33333334f, -12345.678f}) {
        vals.push_back(v);
        bits.push_back(f16pack::round_f16(v));
    }
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return fail("cannot write the output file");
    const unsigned cnt = (unsigned)vals.size();
    std::fwrite(&cnt, 4, 1, f);
    std::fwrite(vals.data(), 4, cnt, f);
    std::fwrite(bits.data(), 2, cnt, f);
    std::fclose(f);
    std::printf("f16 pack ok %u\n", cnt);
    return 0;
}
