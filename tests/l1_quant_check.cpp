// Stand-alone check of nmslib_zig_amd/csrc/l1_quant.hpp (no HIP): built by tests/test_l1_quant_cpu.py with the host
// sanitizers.  For every (query, row) pair of every accepted input it checks, in long double,
//     | L1(q, b) - X_q - s * SAD(q^, b^) | <= E_q
// and that l1q::filter_floor(X_q, E_q, s, SAD) is not above the f32 distance in the exact re-rank's summation order
// (64 strided lane sums, then the xor tree of the wave sum).  Declined inputs must be declined.  The bytes of rows and
// queries are dumped for the test to recompute: per accepted case
//     u32 n, dim, nq | f32 lo[dim] | f64 s | f32 rows[n][dim] | u8 bytes[n][dim] | f32 q[nq][dim] | u8 qbytes[nq][dim]
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../nmslib_zig_amd/csrc/l1_quant.hpp"

using namespace gfxknn;

static int failures = 0;
#define CHECK(c, ...)                     \
    do {                                  \
        if (!(c)) {                       \
            ++failures;                   \
            std::printf("FAIL " __VA_ARGS__); \
            std::printf("\n");            \
        }                                 \
    } while (0)

// the f32 l1 distance as wave_exact_distance_f32 sums it
static float wave_l1(const float* a, const float* q, size_t dim) {
    float v[64];
    for (int l = 0; l < 64; ++l) {
        float s = 0.f;
        for (size_t d = (size_t)l; d < dim; d += 64) s += std::fabs(a[d] - q[d]);
        v[l] = s;
    }
    for (int o = 32; o > 0; o >>= 1) {
        float w[64];
        for (int l = 0; l < 64; ++l) w[l] = v[l] + v[l ^ o];
        for (int l = 0; l < 64; ++l) v[l] = w[l];
    }
    return v[0];
}

static void put(FILE* f, const void* p, size_t bytes) {
    if (std::fwrite(p, 1, bytes, f) != bytes) {
        std::printf("FAIL write\n");
        std::exit(2);
    }
}

// returns whether the input was accepted
static bool run_case(const char* name, const std::vector<float>& rows, size_t n, size_t dim, const std::vector<float>& extra_q,
                     FILE* dump) {
    std::vector<float> lo(dim), hi(dim), rmax(dim);
    std::vector<uint8_t> bytes(n * dim);
    double s = 0;
    if (!l1q::quantise_rows(rows.data(), n, dim, dim, lo.data(), hi.data(), &s, bytes.data(), rmax.data())) {
        std::printf("%s: declined\n", name);
        return false;
    }
    // queries: some rows themselves (inside), rows pushed outside, exactly lo and hi, the extras
    std::vector<float> q;
    for (size_t i = 0; i < n && i < 8; ++i) q.insert(q.end(), rows.begin() + i * dim, rows.begin() + (i + 1) * dim);
    for (size_t i = 0; i < n && i < 8; ++i)
        for (size_t c = 0; c < dim; ++c) {
            const float x = rows[i * dim + c];
            q.push_back((c + i) % 3 == 0 ? x : ((c + i) % 3 == 1 ? hi[c] + 2.5f * (hi[c] - lo[c]) + 1e-3f * std::fabs(hi[c])
                                                                  : lo[c] - 0.75f * (hi[c] - lo[c])));
        }
    q.insert(q.end(), lo.begin(), lo.end());
    q.insert(q.end(), hi.begin(), hi.end());
    q.insert(q.end(), extra_q.begin(), extra_q.end());
    const size_t nq = q.size() / dim;
    std::vector<uint8_t> qb(nq * dim);
    long double worst = 0;
    for (size_t iq = 0; iq < nq; ++iq) {
        double X = 0, E = 0;
        const float* qq = q.data() + iq * dim;
        l1q::query(qq, lo.data(), hi.data(), rmax.data(), dim, s, qb.data() + iq * dim, &X, &E);
        CHECK(X >= 0 && E >= 0, "%s: X %g E %g", name, X, E);
        for (size_t i = 0; i < n; ++i) {
            long double l1 = 0;
            uint32_t sad = 0;
            for (size_t c = 0; c < dim; ++c) {
                l1 += std::fabs((long double)qq[c] - (long double)rows[i * dim + c]);
                const int d = (int)qb[iq * dim + c] - (int)bytes[i * dim + c];
                sad += (uint32_t)(d < 0 ? -d : d);
            }
            const long double gap = std::fabs(l1 - (long double)X - (long double)s * sad);
            // (X is an f64 sum: its own rounding, far below 2^-45 X, is covered by filter_floor's slack, not by E)
            CHECK(gap <= (long double)E + (long double)X * 2.8e-14L, "%s: q %zu row %zu gap %Lg > E %g", name, iq, i, gap, E);
            if (E > 0 && gap / E > worst) worst = gap / E;
            const float d32 = wave_l1(rows.data() + i * dim, qq, dim);
            CHECK(l1q::filter_floor(X, E, s, sad) <= (double)d32, "%s: q %zu row %zu floor %g above f32 distance %g", name, iq, i,
                  l1q::filter_floor(X, E, s, sad), (double)d32);
        }
    }
    std::printf("%s: n %zu dim %zu nq %zu step %g worst gap/E %Lg\n", name, n, dim, nq, s, worst);
    const uint32_t head[3] = {(uint32_t)n, (uint32_t)dim, (uint32_t)nq};
    put(dump, head, sizeof head);
    put(dump, lo.data(), dim * 4);
    put(dump, &s, 8);
    put(dump, rows.data(), rows.size() * 4);
    put(dump, bytes.data(), bytes.size());
    put(dump, q.data(), q.size() * 4);
    put(dump, qb.data(), qb.size());
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* dump = std::fopen(argv[1], "wb");
    if (!dump) return 2;
    std::mt19937 rng(7);
    std::normal_distribution<float> gauss(0.f, 1.f);
    auto random_rows = [&](size_t n, size_t dim, float scale, float offset) {
        std::vector<float> r(n * dim);
        for (float& x : r) x = offset + scale * gauss(rng);
        return r;
    };
    int accepted = 0;
    {
        const size_t n = 300, dim = 21;
        accepted += run_case("random", random_rows(n, dim, 1.f, 0.f), n, dim, {}, dump);
    }
    {
        const size_t n = 200, dim = 130;   // more than two terms per lane of the f32 sum
        accepted += run_case("random130", random_rows(n, dim, 3.f, 10.f), n, dim, {}, dump);
    }
    {
        const size_t n = 120, dim = 9;
        std::vector<float> r = random_rows(n, dim, 1.f, 0.f);
        for (size_t i = 0; i < n; ++i) r[i * dim + 4] = 2.5f;
        accepted += run_case("one constant column", r, n, dim, {}, dump);
    }
    {
        const size_t n = 50, dim = 6;
        std::vector<float> r(n * dim, 0.f);
        for (size_t i = 0; i < n; ++i)
            for (size_t c = 0; c < dim; ++c) r[i * dim + c] = (float)c;
        CHECK(!run_case("all columns constant", r, n, dim, {}, dump), "constant data accepted");
    }
    for (const float bad : {INFINITY, -INFINITY, NAN}) {
        const size_t n = 40, dim = 5;
        std::vector<float> r = random_rows(n, dim, 1.f, 0.f);
        r[17 * dim + 3] = bad;
        CHECK(!run_case("non-finite row", r, n, dim, {}, dump), "a non-finite element was accepted");
    }
    {
        const size_t n = 150, dim = 12;   // every element scaled by 1e-30 / by 1e30: the step scales along
        accepted += run_case("tiny", random_rows(n, dim, 1e-30f, 0.f), n, dim, {}, dump);
        accepted += run_case("huge", random_rows(n, dim, 1e30f, 0.f), n, dim, {}, dump);
    }
    {
        const size_t n = 150, dim = 12;   // 1e-30 and 1e30 side by side: the step follows the widest column
        std::vector<float> r = random_rows(n, dim, 1.f, 0.f);
        for (size_t i = 0; i < n; ++i) {
            r[i * dim + 1] *= 1e-30f;
            r[i * dim + 2] *= 1e30f;
        }
        std::vector<float> extra(2 * dim, 0.f);
        for (size_t c = 0; c < dim; ++c) extra[c] = 3.0e38f, extra[dim + c] = -1e-38f;
        accepted += run_case("mixed scales", r, n, dim, extra, dump);
    }
    {
        // a query with a NaN: excess and bound are NaN, so that the proof's comparison fails; the bytes stay defined
        const float lo[2] = {0.f, 0.f}, hi[2] = {1.f, 1.f}, rmax[2] = {0.f, 0.f}, q[2] = {NAN, 0.5f};
        uint8_t b[2] = {9, 9};
        double X = 0, E = 0;
        l1q::query(q, lo, hi, rmax, 2, 1.0 / 255, b, &X, &E);
        CHECK(std::isnan(X) && !(l1q::filter_floor(X, E, 1.0 / 255, 100) > 0.0), "NaN query: X %g", X);
        CHECK(b[1] == 128 || b[1] == 127, "byte of 0.5: %d", b[1]);
        CHECK(l1q::round_up_f32(1.0 + 1e-12) == std::nextafterf(1.f, 2.f) && l1q::round_up_f32(0.5) == 0.5f, "round_up_f32");
    }
    std::fclose(dump);
    CHECK(accepted == 6, "accepted %d cases", accepted);
    if (failures) return 1;
    std::printf("l1 quant ok\n");
    return 0;
}
