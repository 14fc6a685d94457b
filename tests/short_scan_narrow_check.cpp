// Stand-alone check of the narrow tier of nmslib_zig_amd/csrc/short_scan_plan.hpp (no HIP), built and run by
// tests/test_short_scan_narrow_cpu.py.
//   short_scan_narrow_check ROWS QUERIES OUT n nq : rows [n][128], queries [nq][128] (f32 files) -> restates what finalize and
//       the query preparation compute for a head of kHeadNarrow columns (the prefix of the stored rotation; f32 fma chains in
//       the kernels' order, fp16 rounding of the scaled heads) and writes to OUT: gate, b_tail, bmax, scale, then per query
//       E_s / unit, then per pair the head score / unit.  Asserts here: the 64-wide constants of head_constants() are
//       make_rotation()'s own, the narrow ones differ from them as the derivation says.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../nmslib_zig_amd/csrc/short_scan_plan.hpp"

using namespace gfxknn::shortscan;

static int failures = 0;
#define CHECK(c)                                             \
    do {                                                     \
        if (!(c)) {                                          \
            ++failures;                                      \
            std::printf("FAIL line %d: %s\n", __LINE__, #c); \
        }                                                    \
    } while (0)

constexpr int W = kHeadNarrow;

static std::vector<float> read_f32(const char* path, size_t count) {
    std::vector<float> v(count);
    FILE* f = std::fopen(path, "rb");
    if (!f || std::fread(v.data(), 4, count, f) != count) {
        std::printf("cannot read %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

// the kernels' short_head_tail<32> for one vector of 128 values: the head chains run over the rows of Vh in order, the
// reconstruction stops at column W
static void head_tail(const float* x, const std::vector<float>& vh, float* head, float* tail) {
    for (int j = 0; j < W; ++j) {
        float h = 0.f;
        for (int i = 0; i < kMaxDim; ++i) h = std::fmaf(x[i], vh[(size_t)i * kHead + j], h);
        head[j] = h;
    }
    float t2 = 0.f;
    for (int i = 0; i < kMaxDim; ++i) {
        float r = x[i];
        for (int j = 0; j < W; ++j) r = std::fmaf(-head[j], vh[(size_t)i * kHead + j], r);
        t2 += r * r;
    }
    *tail = std::sqrt(t2) * (1.0f + 4e-7f);   // (the kernel sums in another order: within the allowance's 9.6e-7)
}
static float norm_of(const float* x, int n) {
    double s = 0;
    for (int i = 0; i < n; ++i) s += (double)x[i] * x[i];
    return (float)(std::sqrt(s) * (1 + 1e-6));
}
// v rounded to fp16's grid (11 significant bits, ties to even, subnormal spacing 2^-24; |v| stays far below 65504 here)
static float to_f16(float v) {
    if (v == 0.f || !std::isfinite(v)) return v;
    int e;
    std::frexp(v, &e);
    const int q = std::max(e - 11, -24);
    return std::ldexp(std::nearbyint(std::ldexp(v, -q)), q);
}

int main(int argc, char** argv) {
    if (argc != 6) {
        std::printf("usage: short_scan_narrow_check ROWS QUERIES OUT n nq\n");
        return 2;
    }
    const int n = std::atoi(argv[4]), nq = std::atoi(argv[5]);
    const std::vector<float> rows = read_f32(argv[1], (size_t)n * kMaxDim), qs = read_f32(argv[2], (size_t)nq * kMaxDim);
    std::vector<double> m((size_t)kMaxDim * kMaxDim, 0.0);
    for (int r = 0; r < n; ++r)
        for (int i = 0; i < kMaxDim; ++i)
            for (int j = 0; j < kMaxDim; ++j) m[(size_t)i * kMaxDim + j] += (double)rows[(size_t)r * kMaxDim + i] * rows[(size_t)r * kMaxDim + j];
    const Rotation rot = make_rotation(m, kMaxDim);
    // 64 columns: Rotation's own constants, bit for bit
    const HeadConstants wide = head_constants(rot, kMaxDim, kHead);
    CHECK(wide.delta == rot.delta && wide.frob == rot.frob);
    CHECK(std::memcmp(&wide.coeff, &rot.coeff, 4) == 0 && std::memcmp(&wide.tail_abs, &rot.tail_abs, 4) == 0);
    // 32 columns: |Vh|_F = sqrt(32) up to delta, the allowance of 33 fma in place of 65
    const HeadConstants hc = head_constants(rot, kMaxDim, W);
    CHECK(hc.delta <= rot.delta && hc.delta <= 1e-5);
    CHECK(hc.frob > 5.65 && hc.frob < 5.66);
    CHECK(hc.coeff > 0.f && hc.coeff < rot.coeff && hc.tail_abs > 0.f && hc.tail_abs < rot.tail_abs);

    std::vector<float> heads((size_t)n * W);
    float el = 0.f, tailmax = 0.f, headmax = 0.f, bmax = 0.f;
    for (int r = 0; r < n; ++r) {
        float t;
        head_tail(&rows[(size_t)r * kMaxDim], rot.vh, &heads[(size_t)r * W], &t);
        tailmax = std::max(tailmax, t);
        for (int j = 0; j < W; ++j) el = std::max(el, std::fabs(heads[(size_t)r * W + j]));
        headmax = std::max(headmax, norm_of(&heads[(size_t)r * W], W));
        bmax = std::max(bmax, norm_of(&rows[(size_t)r * kMaxDim], kMaxDim));
    }
    const float b_tail = tail_allowance(tailmax, bmax, hc.tail_abs);
    const float scale = std::ldexp(1.f, 13 - (int)std::floor(std::log2(el)));
    float bres = 0.f;
    for (int r = 0; r < n; ++r) {
        double s = 0;
        for (int j = 0; j < W; ++j) {
            float& h = heads[(size_t)r * W + j];
            const float v = scale * h, hh = to_f16(v);
            s += (double)(v - hh) * (v - hh);
            h = hh;
        }
        bres = std::max(bres, (float)(std::sqrt(s) * (1 + 1e-6)));
    }
    FILE* out = std::fopen(argv[3], "wb");
    if (!out) return 2;
    const double unit = (double)scale * scale;
    const double hdr[4] = {index_gate(b_tail, bmax) ? 1.0 : 0.0, b_tail, bmax, scale};
    std::fwrite(hdr, 8, 4, out);
    std::vector<double> es(nq), scores((size_t)nq * n);
    for (int q = 0; q < nq; ++q) {
        float qh[W], t;
        head_tail(&qs[(size_t)q * kMaxDim], rot.vh, qh, &t);
        const float qn = norm_of(&qs[(size_t)q * kMaxDim], kMaxDim);
        double ss = 0, rr = 0;
        for (int j = 0; j < W; ++j) {
            const float v = scale * qh[j], hh = to_f16(v);
            ss += (double)v * v;
            rr += (double)(v - hh) * (v - hh);
            qh[j] = hh;
        }
        const float qnh = (float)std::sqrt(ss), qr = (float)std::sqrt(rr);
        const float e_head = 1.01f * (qr * scale * headmax + 1.004f * qnh * bres) + 2e-5f * qnh * scale * headmax;
        es[q] = short_error(e_head, (float)unit, tail_allowance(t, qn, hc.tail_abs), b_tail, qn, bmax, hc.coeff) / unit;
        for (int r = 0; r < n; ++r) {
            float acc = 0.f;   // (f32 accumulation, like the matrix cores')
            for (int j = 0; j < W; ++j) acc = std::fmaf(qh[j], heads[(size_t)r * W + j], acc);
            scores[(size_t)q * n + r] = (double)acc / unit;
        }
    }
    std::fwrite(es.data(), 8, es.size(), out);
    std::fwrite(scores.data(), 8, scores.size(), out);
    std::fclose(out);
    if (failures) return 1;
    std::printf("narrow bound written: gate %d b_tail %.6g bmax %.6g coeff %.4g (64 columns: %.4g)\n", (int)hdr[0], (double)b_tail,
                (double)bmax, (double)hc.coeff, (double)rot.coeff);
    return 0;
}
