// Stand-alone check of nmslib_zig_amd/csrc/short_scan_plan.hpp (no HIP), built and run by tests/test_short_scan_plan_cpu.py.
//   short_scan_plan_check jacobi                      : a random 128 x 128 second-moment matrix -> V^T V = I to 1e-5,
//                                                        eigenvalues sorted, V^T M V diagonal
//   short_scan_plan_check bound ROWS QUERIES OUT n nq : rows [n][128], queries [nq][128] (f32 files) -> restates what
//       finalize and the query preparation compute (f32 fma chains in the kernels' order, fp16 rounding of the scaled heads)
//       and writes to OUT: gate, b_tail, bmax, scale, then per query E_s / unit, then per pair the head score / unit.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>

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

// the kernels' short_head_tail for one vector of 128 values
static void head_tail(const float* x, const std::vector<float>& vh, float* head, float* tail) {
    for (int j = 0; j < kHead; ++j) {
        float h = 0.f;
        for (int i = 0; i < kMaxDim; ++i) h = std::fmaf(x[i], vh[(size_t)i * kHead + j], h);
        head[j] = h;
    }
    float t2 = 0.f;
    for (int i = 0; i < kMaxDim; ++i) {
        float r = x[i];
        for (int j = 0; j < kHead; ++j) r = std::fmaf(-head[j], vh[(size_t)i * kHead + j], r);
        t2 += r * r;
    }
    *tail = std::sqrt(t2) * (1.0f + 4e-7f);   // (the kernel sums in another order: within the allowance's 9.6e-7)
}
static float norm_of(const float* x, int n) {
    double s = 0;
    for (int i = 0; i < n; ++i) s += (double)x[i] * x[i];
    return (float)(std::sqrt(s) * (1 + 1e-6));
}

static int run_jacobi() {
    const int n = 128;
    std::mt19937_64 rng(7);
    std::normal_distribution<double> nd;
    std::vector<double> x((size_t)400 * n), m((size_t)n * n, 0.0);
    for (double& v : x) v = nd(rng);
    for (int r = 0; r < 400; ++r)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) m[(size_t)i * n + j] += x[(size_t)r * n + i] * (1 + i % 7) * x[(size_t)r * n + j] * (1 + j % 7);
    const std::vector<double> m0 = m;
    std::vector<double> v, eig;
    const int sweeps = jacobi_eigen(m, n, v, eig);
    CHECK(sweeps < 64);
    for (int j = 1; j < n; ++j) CHECK(eig[j - 1] >= eig[j]);
    double worst = 0, worst_d = 0;
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            double s = 0, d = 0;
            for (int i = 0; i < n; ++i) {
                s += v[(size_t)i * n + a] * v[(size_t)i * n + b];
                double mv = 0;
                for (int k = 0; k < n; ++k) mv += m0[(size_t)i * n + k] * v[(size_t)k * n + b];
                d += v[(size_t)i * n + a] * mv;
            }
            worst = std::max(worst, std::fabs(s - (a == b ? 1.0 : 0.0)));
            worst_d = std::max(worst_d, std::fabs(d - (a == b ? eig[a] : 0.0)) / eig[0]);
        }
    std::printf("jacobi: sweeps %d |V^T V - I|max %.3g |V^T M V - diag|max / eig0 %.3g\n", sweeps, worst, worst_d);
    CHECK(worst <= 1e-5);
    CHECK(worst_d <= 1e-9);
    // the stored f32 columns: still orthogonal to 1e-5, and the constants say so
    std::vector<double> m1 = m0;
    const Rotation rot = make_rotation(m1, n);
    CHECK(rot.delta <= 1e-5 && rot.frob > 7.99 && rot.frob < 8.01);
    CHECK(rot.coeff > 0.f && rot.coeff < 5e-4f && rot.tail_abs > 0.f && rot.tail_abs < 1e-4f);
    CHECK(index_gate(1.0f, 45.0f) && !index_gate(8.0f, 11.0f) && !index_gate(0.f, 0.f));
    if (!failures) std::printf("short scan jacobi ok\n");
    return failures != 0;
}

// v rounded to fp16's grid (11 significant bits, ties to even, subnormal spacing 2^-24; |v| stays far below 65504 here)
static float to_f16(float v) {
    if (v == 0.f || !std::isfinite(v)) return v;
    int e;
    std::frexp(v, &e);
    const int q = std::max(e - 11, -24);
    return std::ldexp(std::nearbyint(std::ldexp(v, -q)), q);
}

static int run_bound(const char* rows_path, const char* q_path, const char* out_path, int n, int nq) {
    const std::vector<float> rows = read_f32(rows_path, (size_t)n * kMaxDim), qs = read_f32(q_path, (size_t)nq * kMaxDim);
    std::vector<double> m((size_t)kMaxDim * kMaxDim, 0.0);
    for (int r = 0; r < n; ++r)
        for (int i = 0; i < kMaxDim; ++i)
            for (int j = 0; j < kMaxDim; ++j) m[(size_t)i * kMaxDim + j] += (double)rows[(size_t)r * kMaxDim + i] * rows[(size_t)r * kMaxDim + j];
    const Rotation rot = make_rotation(m, kMaxDim);
    std::vector<float> heads((size_t)n * kHead);
    float el = 0.f, tailmax = 0.f, headmax = 0.f, bmax = 0.f;
    for (int r = 0; r < n; ++r) {
        float t;
        head_tail(&rows[(size_t)r * kMaxDim], rot.vh, &heads[(size_t)r * kHead], &t);
        tailmax = std::max(tailmax, t);
        for (int j = 0; j < kHead; ++j) el = std::max(el, std::fabs(heads[(size_t)r * kHead + j]));
        headmax = std::max(headmax, norm_of(&heads[(size_t)r * kHead], kHead));
        bmax = std::max(bmax, norm_of(&rows[(size_t)r * kMaxDim], kMaxDim));
    }
    const float b_tail = tail_allowance(tailmax, bmax, rot.tail_abs);
    const float scale = std::ldexp(1.f, 13 - (int)std::floor(std::log2(el)));
    float bres = 0.f;
    for (int r = 0; r < n; ++r) {
        double s = 0;
        for (int j = 0; j < kHead; ++j) {
            float& h = heads[(size_t)r * kHead + j];
            const float v = scale * h, hh = to_f16(v);
            s += (double)(v - hh) * (v - hh);
            h = hh;
        }
        bres = std::max(bres, (float)(std::sqrt(s) * (1 + 1e-6)));
    }
    FILE* out = std::fopen(out_path, "wb");
    if (!out) return 2;
    const double unit = (double)scale * scale;
    const double hdr[4] = {index_gate(b_tail, bmax) ? 1.0 : 0.0, b_tail, bmax, scale};
    std::fwrite(hdr, 8, 4, out);
    std::vector<double> es(nq), scores((size_t)nq * n);
    for (int q = 0; q < nq; ++q) {
        float qh[kHead], t;
        head_tail(&qs[(size_t)q * kMaxDim], rot.vh, qh, &t);
        const float qn = norm_of(&qs[(size_t)q * kMaxDim], kMaxDim);
        double ss = 0, rr = 0;
        for (int j = 0; j < kHead; ++j) {
            const float v = scale * qh[j], hh = to_f16(v);
            ss += (double)v * v;
            rr += (double)(v - hh) * (v - hh);
            qh[j] = hh;
        }
        const float qnh = (float)std::sqrt(ss), qr = (float)std::sqrt(rr);
        const float e_head = 1.01f * (qr * scale * headmax + 1.004f * qnh * bres) + 2e-5f * qnh * scale * headmax;
        es[q] = short_error(e_head, (float)unit, tail_allowance(t, qn, rot.tail_abs), b_tail, qn, bmax, rot.coeff) / unit;
        for (int r = 0; r < n; ++r) {
            float acc = 0.f;   // (f32 accumulation, like the matrix cores')
            for (int j = 0; j < kHead; ++j) acc = std::fmaf(qh[j], heads[(size_t)r * kHead + j], acc);
            scores[(size_t)q * n + r] = (double)acc / unit;
        }
    }
    std::fwrite(es.data(), 8, es.size(), out);
    std::fwrite(scores.data(), 8, scores.size(), out);
    std::fclose(out);
    std::printf("short scan bound written: gate %d b_tail %.6g bmax %.6g\n", (int)hdr[0], (double)b_tail, (double)bmax);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 2 && std::string(argv[1]) == "jacobi") return run_jacobi();
    if (argc == 7 && std::string(argv[1]) == "bound") return run_bound(argv[2], argv[3], argv[4], std::atoi(argv[5]), std::atoi(argv[6]));
    std::printf("usage: short_scan_plan_check jacobi | bound ROWS QUERIES OUT n nq\n");
    return 2;
}
