// Stand-alone check of nmslib_zig_amd/csrc/diverg_js_filter.hpp (no HIP), built with the host sanitizers by
// tests/test_js_filter_cpu.py.  For every (row, query) pair of its inputs: the filter's key by a software model of the loop
// (same order, f32 arithmetic, the logarithm an f64 log2 pushed to either end of +-kHwLog2Ulps ulp) lies within E_q of the f32
// value in DivAcc<DV_JS>'s order, and the floor is not above it; queries with a NaN, an infinity or a negative element get no
// proof; the square-root floor of jsmetr* is not above the f32 distance; the plan's gates.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../nmslib_zig_amd/csrc/diverg_js_filter.hpp"

using namespace gfxknn;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); } } while (0)

static const float kFltMin = 1.17549435e-38f;

// DivAcc<DV_JS> before finish(); fast: the logarithm rule of jsdivfast / jsmetrfast, else of the slow spaces
static float divacc_js(const float* x, const float* y, size_t D, bool fast) {
    auto lg = [&](float v) { return fast ? (v > 0 ? logf(v) : -1e5f) : (v < kFltMin ? 0.0f : logf(v)); };
    float r = 0.f, r2 = 0.f;
    for (size_t j = 0; j < D; ++j) {
        r = r + (x[j] * lg(x[j]) + y[j] * lg(y[j]));
        const float m = 0.5f * (x[j] + y[j]);
        if (m >= kFltMin) r2 = r2 + m * logf(m);
    }
    return 0.5f * r - r2;
}

// the filter's key; push: ulps added to every logarithm
static float model_key(const float* x, const float* y, size_t D, float R32, int push) {
    float a[4] = {0, 0, 0, 0};
    for (size_t j = 0; j < (D + 3) / 4 * 4; ++j) {
        const float xv = j < D ? x[j] : 0.f, yv = j < D && y[j] > djs::kClamp ? y[j] : djs::kClamp;
        const float s = xv + yv;
        float l = (float)std::log2((double)s);
        for (int i = 0; i < std::abs(push); ++i) l = std::nextafterf(l, push > 0 ? INFINITY : -INFINITY);
        a[j & 3] = fmaf(s, l, a[j & 3]);
    }
    return fmaf(-(float)djs::kHalfLn2, ((a[0] + a[1]) + a[2]) + a[3], R32);
}

static void run(const std::vector<float>& rows, const std::vector<float>& qs, size_t D) {
    const size_t n = rows.size() / D, nq = qs.size() / D;
    std::vector<float> R32(n);
    djs::RowMax m{0, 0, 0};
    bool ok = true;
    for (size_t r = 0; r < n; ++r) R32[r] = (float)djs::row(&rows[r * D], D, &m, &ok);
    CHECK(ok, "D=%zu: clean rows refused", D);
    const int K = (int)djs::kHwLog2Ulps;
    size_t proven = 0;
    double worst = 0;
    for (size_t iq = 0; iq < nq; ++iq) {
        const float* q = &qs[iq * D];
        std::vector<float> pack((D + 3) / 4 * 8, 0.f);   // a query pack with a group stride of 8 floats
        for (size_t j = 0; j < D; ++j) pack[(j >> 2) * 8 + (j & 3)] = q[j];
        double C, E;
        djs::query(pack.data(), 8, D, m, &C, &E);
        bool clean = true;
        for (size_t j = 0; j < D; ++j) clean = clean && q[j] >= 0 && std::isfinite(q[j]);
        CHECK(clean == std::isfinite(E), "D=%zu: query %zu clean %d but E %g", D, iq, (int)clean, E);
        if (!std::isfinite(E)) {
            CHECK(!(djs::proof_floor(0.f, C, E, 0) > -INFINITY) && !(djs::proof_floor(0.f, C, E, 1) > 0), "a floor without a proof");
            continue;
        }
        ++proven;
        for (size_t r = 0; r < n; ++r)
            for (int push = -K; push <= K; push += 2 * K)
                for (int fast = 0; fast < 2; ++fast) {
                    const float key = model_key(&rows[r * D], q, D, R32[r], push);
                    const float v = divacc_js(&rows[r * D], q, D, fast != 0);
                    const double err = std::fabs((double)key + C - (double)v);
                    worst = err / E > worst ? err / E : worst;
                    CHECK(std::isfinite(key) && err <= E, "D=%zu q %zu row %zu |key + C - v| %g above E %g", D, iq, r, err, E);
                    CHECK(!(dvf::filter_floor(key, C, E) > (double)v), "D=%zu q %zu row %zu floor above the f32 value", D, iq, r);
                    const float d = sqrtf(v < 0.0f ? 0.0f : v);
                    CHECK(!(djs::proof_floor(key, C, E, 1) > (double)d), "D=%zu q %zu row %zu sqrt floor above the distance", D, iq, r);
                }
    }
    std::printf("js D=%zu: %zu rows, %zu of %zu queries with a proof, largest |key + C - v| / E %.3f\n", D, n, proven, nq, worst);
}

int main() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> uni(0.0f, 1.0f);
    const size_t dims[4] = {1, 5, 100, 257};
    for (size_t D : dims) {
        const size_t n = 40, nq = 12;
        std::vector<float> rows(n * D), qs(nq * D);
        // histograms; every third element of the odd rows and of the queries 3 k + 1 is a zero
        for (size_t i = 0; i < rows.size(); ++i) rows[i] = (i / D) % 2 && i % 3 == 0 ? 0.f : uni(rng) / (float)D;
        for (size_t i = 0; i < qs.size(); ++i) qs[i] = (i / D) % 3 == 1 && i % 3 == 1 ? 0.f : uni(rng) / (float)D;
        for (size_t j = 0; j < D; ++j) {
            rows[1 * D + j] = 1e-30f * (1 + j % 3);   // tiny elements, elements above 1, all zeros
            rows[2 * D + j] = 3.0f + (float)(j % 7);
            rows[3 * D + j] = 0.f;
            rows[4 * D + j] = qs[0 * D + j];          // a copy of query 0 and a near-copy
            rows[5 * D + j] = qs[0 * D + j] * (1 + 1e-4f * (j % 5));
            qs[2 * D + j] = 1e-30f;
            qs[3 * D + j] = 2.0f + (float)(j % 3);
            qs[4 * D + j] = 0.f;
            qs[5 * D + j] = j % 2 ? 1e-36f : 0.5f;     // below the clamp
        }
        qs[9 * D + D / 2] = -0.25f;    // no proof: a negative element, a NaN, an infinity
        qs[10 * D] = NAN;
        qs[11 * D + D - 1] = INFINITY;
        run(rows, qs, D);
    }
    djs::RowMax m{0, 0, 0};
    bool ok = true;
    const float neg[3] = {0.5f, -1e-3f, 0.25f}, inf[2] = {INFINITY, 1.f};
    djs::row(neg, 3, &m, &ok);
    CHECK(!ok, "a negative row element was accepted");
    ok = true;
    djs::row(inf, 2, &m, &ok);
    CHECK(!ok, "an infinite row element was accepted");
    // the plan's gates, either side of each edge, and its shape at the GPU test's sizes
    auto use = [](int n, int dim, int nq, int k, bool have) { return djs::plan(n, dim, nq, k, have).use; };
    CHECK(use(65536, 257, 256, 128, true) && use(65536, 1, 256, 1, true), "gates: the base cases");
    CHECK(!use(65535, 128, 256, 10, true) && !use(65536, 128, 255, 10, true), "gates: n, nq");
    CHECK(!use(65536, 128, 256, 129, true) && !use(65536, 128, 256, 0, true) && !use(65536, 128, 256, 10, false), "gates: k, rows");
    const dvf::Plan p = djs::plan(65536 + 37, 100, 300, 10, true);
    CHECK(p.nblocks == 1025 && p.rows_per_split == 1088 && p.nsplit == 64 && p.qpad == 304 && p.nqt == 19 && p.ngroups == 19, "plan");
    if (failures == 0) std::printf("js filter ok\n");
    return failures ? 1 : 0;
}
