// Stand-alone check of nmslib_zig_amd/csrc/sparse_filter.hpp (no HIP), built with the host sanitizers by
// tests/test_sparse_filter_cpu.py.  For each served kind and every (row, query) pair of its inputs: the filter's score A,
// accumulated in the kernel's order (fused steps over the shared terms, in the query's order), is within
// spf::filter_err of the real sum over the stored values, and spf::floor_dist at T = A is not above the f32 distance in
// the exact scan's union order (UnionAcc restated here: four lanes, the contracted tail; the sequential fused loop of the
// query-norm space).  Queries the proof cannot serve get a NaN floor; the plan is on the right side of each gate.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../nmslib_zig_amd/csrc/sparse_filter.hpp"

using namespace gfxknn;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); } } while (0)

struct Vec {
    std::vector<uint32_t> id;
    std::vector<float> v;
};

// the scan's distance(row, query): x = the row's values, y = the query's over the union of the ids
static float union_dist(int kind, const Vec& a, const Vec& b) {
    std::vector<float> x, y;
    size_t i = 0, j = 0;
    while (i < a.id.size() && j < b.id.size()) {
        const bool ta = a.id[i] <= b.id[j], tb = b.id[j] <= a.id[i];
        x.push_back(ta ? a.v[i] : 0.f);
        y.push_back(tb ? b.v[j] : 0.f);
        i += ta, j += tb;
    }
    for (; i < a.id.size(); ++i) x.push_back(a.v[i]), y.push_back(0.f);
    for (; j < b.id.size(); ++j) x.push_back(0.f), y.push_back(b.v[j]);
    const size_t L = x.size(), L4 = L / 4 * 4;
    const float eps = 1.17549435e-38f * 2.0f;
    if (kind == spf::QNORM) {
        float qs = 0.f, c0 = 0.f;
        for (size_t p = 0; p < L; ++p) c0 = fmaf(y[p], y[p], c0), qs = fmaf(x[p], y[p], qs);
        return -(qs / sqrtf(fmaxf(c0, eps)));
    }
    float s[4] = {0, 0, 0, 0}, n1[4] = {0, 0, 0, 0}, n2[4] = {0, 0, 0, 0};
    for (size_t p = 0; p < L4; ++p) {
        s[p & 3] = s[p & 3] + x[p] * y[p];
        n1[p & 3] = n1[p & 3] + x[p] * x[p];
        n2[p & 3] = n2[p & 3] + y[p] * y[p];
    }
    float S = ((s[0] + s[1]) + s[2]) + s[3], N1 = ((n1[0] + n1[1]) + n1[2]) + n1[3], N2 = ((n2[0] + n2[1]) + n2[2]) + n2[3];
    for (size_t p = L4; p < L; ++p) S = fmaf(x[p], y[p], S), N1 = fmaf(x[p], x[p], N1), N2 = fmaf(y[p], y[p], N2);
    if (kind == spf::DOT) return -S;
    float v = 0.f;
    if (!(N1 < eps || N2 < eps)) v = fmaxf(-1.0f, fminf(1.0f, S / sqrtf(N1) / sqrtf(N2)));
    return kind == spf::ANG ? acosf(v) : fmaxf(0.0f, 1.0f - v);
}

static double norm2(const Vec& a) {
    double s = 0;
    for (float v : a.v) s += (double)v * v;
    return s;
}

// every pair of rows x queries; `proved` queries must get a floor, the others must not
static void run(const char* name, int kind, const std::vector<Vec>& rows, const std::vector<Vec>& qs, size_t proved) {
    size_t longest = 0, got = 0;
    double beta2 = 0;
    std::vector<Vec> stored(rows.size());
    for (size_t r = 0; r < rows.size(); ++r) {
        longest = std::max(longest, rows[r].id.size());
        const double s = norm2(rows[r]);
        const int cls = spf::row_class(kind, s);
        CHECK(cls != spf::ROW_DECLINE, "%s: row %zu of norm^2 %g declines the copy", name, r, s);
        if (cls != spf::ROW_POSTED) continue;   // no postings: the score stays 0
        stored[r].id = rows[r].id;
        for (float v : rows[r].v) stored[r].v.push_back(spf::stored_value(kind, v, std::sqrt(s)));
        beta2 = std::max(beta2, norm2(stored[r]));
    }
    const double beta = spf::round_up_f32(std::sqrt(beta2) * (1.0 + 9.094947017729282e-13));
    for (size_t qi = 0; qi < qs.size(); ++qi) {
        const Vec& q = qs[qi];
        const int m = (int)q.id.size(), L = m + (int)longest;
        const double qn = std::sqrt(norm2(q));
        const bool has = std::isfinite(spf::floor_dist(kind, 0.0, m, L, qn, beta));
        got += has;
        for (size_t r = 0; r < rows.size() && has; ++r) {
            float A = 0.f;
            double real = 0;
            for (size_t j = 0; j < q.id.size(); ++j)
                for (size_t i = 0; i < stored[r].id.size(); ++i)
                    if (stored[r].id[i] == q.id[j]) {
                        A = fmaf(q.v[j], stored[r].v[i], A);
                        real += (double)q.v[j] * (double)stored[r].v[i];
                    }
            CHECK(std::fabs((double)A - real) <= spf::filter_err(m, qn, beta), "%s: row %zu query %zu: A %g real %g", name, r, qi,
                  (double)A, real);
            const double fl = spf::floor_dist(kind, (double)A, m, L, qn, beta);
            const float d = union_dist(kind, rows[r], q);
            CHECK(fl <= (double)d, "%s: row %zu query %zu: floor %.9g above the scan's %.9g", name, r, qi, fl, (double)d);
        }
    }
    CHECK(got == proved, "%s: %zu queries with a proof, expected %zu", name, got, proved);
    std::printf("%s: %zu of %zu queries with a proof\n", name, got, qs.size());
}

static Vec random_vec(std::mt19937& g, int len, uint32_t vocab, float lo, float hi, bool sign) {
    std::vector<bool> used(vocab, false);
    std::uniform_real_distribution<float> u(lo, hi);
    Vec v;
    for (int i = 0; i < len; ++i) used[(size_t)(vocab * std::pow(std::uniform_real_distribution<double>(0, 1)(g), 3.0))] = true;
    for (uint32_t t = 0; t < vocab; ++t)
        if (used[t]) v.id.push_back(t), v.v.push_back((sign && (g() & 1)) ? -u(g) : u(g));
    return v;
}

int main() {
    std::mt19937 g(7);
    for (int kind = spf::DOT; kind <= spf::ANG; ++kind) {
        const char* names[] = {"dot", "qnorm", "cos", "ang"};
        std::vector<Vec> rows, qs;
        for (int i = 0; i < 40; ++i) rows.push_back(random_vec(g, 1 + (int)(g() % 60), 300, 0.1f, 1.0f, i & 1));
        rows.push_back(random_vec(g, 4000, 6000, 0.1f, 1.0f, true));          // as long as the recorded maximum
        Vec c;                                                                // cancelling signed values
        for (uint32_t t = 0; t < 64; ++t) c.id.push_back(t), c.v.push_back((t & 1) ? -1000.0f : 1000.0f + 1e-3f * (float)t);
        rows.push_back(c);
        rows.push_back(Vec{{5}, {0.25f}});                                    // one shared term at most
        rows.push_back(Vec{{1, 5}, {1.0e-15f, 1.0e-17f}});                    // norm^2 just above kSafeLo
        rows.push_back(Vec{{2, 5}, {1.0e-20f, 3.0e-21f}});                    // under the zero-norm test: no postings for cosine
        rows.push_back(Vec{{3, 7}, {3e14f, -2e14f}});                         // large: norm^2 just under kSafeHi
        for (int i = 0; i < 12; ++i) qs.push_back(random_vec(g, 1 + (int)(g() % 40), 300, 0.1f, 1.0f, i & 1));
        qs.push_back(random_vec(g, 4096, 6000, 0.5f, 1.0f, true));
        Vec ones;
        for (uint32_t t = 0; t < 64; ++t) ones.id.push_back(t), ones.v.push_back(1.0f);
        qs.push_back(ones);                                                   // against the cancelling row
        qs.push_back(Vec{{5}, {2.0f}});                                       // a single element
        qs.push_back(Vec{{1, 2, 5}, {1.1e-15f, 1e-16f, 1e-16f}});             // norm^2 just above kSafeLo
        const size_t proved = qs.size();
        qs.push_back(Vec{{5}, {1e-16f}});                                     // norm^2 under kSafeLo
        qs.push_back(Vec{{5}, {0.0f}});                                       // zero norm
        qs.push_back(Vec{{5, 9}, {1.0f, NAN}});
        qs.push_back(Vec{{5, 9}, {1.0f, INFINITY}});
        qs.push_back(Vec{{5}, {1e20f}});                                      // products could leave f32's range
        run(names[kind], kind, rows, qs, proved);
    }
    // the cosine family declines rows whose norm the proof cannot work with
    CHECK(spf::row_class(spf::COS, 1e-35) == spf::ROW_DECLINE && spf::row_class(spf::ANG, 1e31) == spf::ROW_DECLINE, "row classes");
    CHECK(spf::row_class(spf::COS, 1e-39) == spf::ROW_EMPTY && spf::row_class(spf::DOT, 1e-39) == spf::ROW_POSTED, "row classes");
    CHECK(spf::floor_dist(spf::COS, -INFINITY, 3, 10, 1.0, 1.0) == INFINITY, "every row listed");
    // the plan: either side of each gate
    const auto use = [](int kind, long long n, long long nq, long long k, long long len, bool asc, bool have) {
        return spf::plan(kind, n, nq, k, len, asc, have).use;
    };
    CHECK(use(spf::DOT, 65536, 1, 128, 4096, true, true), "the plan at its gates");
    CHECK(!use(-1, 65536, 1, 128, 4096, true, true) && !use(4, 65536, 1, 128, 4096, true, true), "space gate");
    CHECK(!use(spf::COS, 65535, 1, 10, 10, true, true) && use(spf::COS, 65536, 1, 10, 10, true, true), "row gate");
    CHECK(!use(spf::COS, 70000, 1, 129, 10, true, true) && !use(spf::COS, 70000, 1, 0, 10, true, true), "k gate");
    CHECK(!use(spf::ANG, 70000, 3, 10, 4097, true, true) && !use(spf::ANG, 70000, 0, 10, 10, true, true), "query gates");
    CHECK(!use(spf::QNORM, 70000, 3, 10, 10, false, true) && !use(spf::QNORM, 70000, 3, 10, 10, true, false), "order / copy gates");
    const spf::Plan p = spf::plan(spf::DOT, 65536 + 37, 300, 10, 100, true, true);
    CHECK(p.nblocks == 5 && p.keep == 18, "plan figures %d %d", p.nblocks, p.keep);
    if (failures == 0) std::printf("sparse filter ok\n");
    return failures != 0;
}
