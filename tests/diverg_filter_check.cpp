// Stand-alone check of nmslib_zig_amd/csrc/diverg_filter.hpp (no HIP), built with the host sanitizers by
// tests/test_diverg_filter_cpu.py.  For each of the five forms and every (row, query) pair of its inputs:
// dvf::filter_floor(key, C_q, E_q) is not above the f32 distance in the exact scan's summation order (DivAcc restated
// here: four lanes, the contracted tail), where key is the filter's key with the chain summed in f32; queries with a zero,
// a NaN or an infinity get no proof; the plan's gates on either side of each edge.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../nmslib_zig_amd/csrc/diverg_filter.hpp"

using namespace gfxknn;

static int failures = 0;
#define CHECK(c, ...) do { if (!(c)) { ++failures; std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); } } while (0)

static float flog(float x) { return x > 0 ? logf(x) : -1e5f; }

// formula(obj1 = (x, lx), obj2 = (y, ly, iy)) in DivAcc's order; gen: generalized KL; is: Itakura-Saito
static float divacc(int kind, const float* x, const float* lx, const float* y, const float* ly, size_t D) {
    float s[4] = {0, 0, 0, 0};
    const size_t G4 = D / 4;
    for (size_t g = 0; g < G4; ++g)
        for (int i = 0; i < 4; ++i) {
            const size_t j = 4 * g + i;
            if (kind == 0) s[i] = s[i] + x[j] * (lx[j] - ly[j]);
            else if (kind == 1) s[i] = (s[i] + x[j] * (lx[j] - ly[j])) + (y[j] - x[j]);
            else s[i] = s[i] + (x[j] * (1.0f / y[j]) - (lx[j] - ly[j]));
        }
    float r = ((s[0] + s[1]) + s[2]) + s[3];
    for (size_t j = 4 * G4; j < D; ++j) {
        if (kind == 0) r = fmaf(x[j], lx[j] - ly[j], r);
        else if (kind == 1) r = r + (fmaf(x[j], lx[j] - ly[j], y[j]) - x[j]);
        else r = r + (x[j] * (1.0f / y[j]) - (lx[j] - ly[j]));
    }
    return kind == 2 ? r - (float)D : r;
}

static void run(const char* name, int form, const std::vector<float>& rows, const std::vector<float>& qs, size_t D) {
    const size_t n = rows.size() / D, nq = qs.size() / D, dpad = (D + 15) / 16 * 16;
    std::vector<uint16_t> rh(n * dpad), rl(n * dpad), qh(dpad), ql(dpad);
    std::vector<float> lr(rows.size()), R32(n), lq(D), iq(D);
    dvf::RowMax m{0, 0, 0, 0, 0};
    for (size_t r = 0; r < n; ++r) {
        for (size_t j = 0; j < D; ++j) lr[r * D + j] = flog(rows[r * D + j]);
        R32[r] = (float)dvf::row(form, &rows[r * D], &lr[r * D], D, dpad, &rh[r * dpad], &rl[r * dpad], &m);
    }
    const int kind = form == dvf::IS ? 2 : (form == dvf::KLGEN || form == dvf::KLGEN_RQ ? 1 : 0);
    size_t proven = 0;
    for (size_t iq_ = 0; iq_ < nq; ++iq_) {
        const float* q = &qs[iq_ * D];
        for (size_t j = 0; j < D; ++j) lq[j] = flog(q[j]), iq[j] = 1.0f / q[j];
        double C, E;
        dvf::query(form, q, lq.data(), iq.data(), 4, D, dpad, m, qh.data(), ql.data(), &C, &E);
        bool clean = true;
        double bb = 0;
        for (size_t j = 0; j < D; ++j) {
            clean = clean && q[j] > 0 && std::isfinite(q[j]);
            const double b = dvf::query_operand(form, q[j], lq[j], iq[j]);
            bb += b * b;
        }
        // (a clean query goes without a proof only where the chain could leave f32's range and give a key no list holds)
        const bool range = (double)m.a * std::sqrt(bb) + (double)m.r_abs < 5e36;
        CHECK(clean ? (std::isfinite(E) || !range) : !std::isfinite(E), "%s: query %zu clean %d in range %d but E %g", name,
              iq_, (int)clean, (int)range, E);
        if (!std::isfinite(E)) {
            CHECK(!(dvf::filter_floor(0.f, C, E) > -INFINITY), "%s: a floor without a proof", name);
            continue;
        }
        ++proven;
        for (size_t r = 0; r < n; ++r) {
            float acc = 0.f;   // the chain, here in column order with every addition rounded to nearest
            for (size_t j = 0; j < dpad; ++j) {
                const float ah = dvf::bf16_f32(rh[r * dpad + j]), al = dvf::bf16_f32(rl[r * dpad + j]);
                const float bh = dvf::bf16_f32(qh[j]), bl = dvf::bf16_f32(ql[j]);
                acc = acc + ah * bh;
                acc = acc + ah * bl;
                acc = acc + al * bh;
            }
            const float key = fmaf((float)dvf::sign_of(form), acc, R32[r]);
            CHECK(std::isfinite(key), "%s: q %zu row %zu has a proof and the key %g", name, iq_, r, (double)key);
            const float* x = &rows[r * D];
            const float d = dvf::row_is_log(form) ? divacc(kind, q, lq.data(), x, &lr[r * D], D)
                                                  : divacc(kind, x, &lr[r * D], q, lq.data(), D);
            const double fl = dvf::filter_floor(key, C, E);
            // (the proof asks for floor > d_k: an overflowed key, whose floor is NaN, proves nothing)
            CHECK(!(fl > (double)d), "%s: q %zu row %zu floor %.9g above the f32 distance %.9g (E %g)", name, iq_, r, fl, (double)d, E);
            if (std::isfinite(key) && std::isfinite(d))
                CHECK(std::fabs((double)key + C - (double)d) <= E, "%s: q %zu row %zu |key + C - d| %g above E %g", name, iq_,
                      r, std::fabs((double)key + C - (double)d), E);
        }
    }
    std::printf("%s D=%zu: %zu rows, %zu of %zu queries with a proof\n", name, D, n, proven, nq);
}

int main() {
    static const char* names[5] = {"kl", "kl_rq", "klgen", "klgen_rq", "is"};
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> uni(1e-3f, 1.0f);
    const size_t dims[5] = {1, 15, 16, 17, 256};
    for (int form = 0; form < 5; ++form)
        for (size_t D : dims) {
            const size_t n = 40, nq = 12;
            std::vector<float> rows(n * D), qs(nq * D);
            for (auto& v : rows) v = uni(rng);
            for (auto& v : qs) v = uni(rng);
            for (size_t j = 0; j < D; ++j) {
                rows[1 * D + j] = 1e-30f * (1 + j % 3);                   // tiny and huge elements
                rows[2 * D + j] = 1e30f;
                rows[3 * D + j] = j % 2 ? 0.f : 0.5f;                     // zeros: the sentinel logarithm
                rows[4 * D + j] = qs[0 * D + j];                          // a copy of query 0 and near-copies of it
                rows[5 * D + j] = std::nextafterf(qs[0 * D + j], 2.f);
                rows[6 * D + j] = qs[0 * D + j] * (1 + 1e-4f * (j % 5));
                qs[1 * D + j] = 1e-20f;
                qs[2 * D + j] = 1e20f;
            }
            qs[3 * D + D / 2] = 0.f;            // no proof: a zero, a NaN, an infinity
            qs[4 * D] = NAN;
            qs[5 * D + D - 1] = INFINITY;
            run(names[form], form, rows, qs, D);
        }
    // the plan's gates, either side of each edge
    auto use = [](int form, int n, int dim, int nq, int k, bool have) { return dvf::plan(form, n, dim, nq, k, have).use; };
    CHECK(use(dvf::KL, 65536, 128, 256, 10, true), "gates: the base case");
    CHECK(!use(dvf::KL, 65535, 128, 256, 10, true) && !use(dvf::KL, 65536, 128, 255, 10, true), "gates: n, nq");
    CHECK(use(dvf::IS, 65536, 256, 256, 128, true) && !use(dvf::IS, 65536, 257, 256, 128, true), "gates: D");
    CHECK(!use(dvf::IS, 65536, 256, 256, 129, true) && !use(dvf::IS, 65536, 256, 256, 0, true), "gates: k");
    CHECK(!use(dvf::KL, 65536, 128, 256, 10, false) && !use(-1, 65536, 128, 256, 10, true), "gates: copy, space");
    const dvf::Plan p = dvf::plan(dvf::KL, 65536 + 37, 100, 300, 10, true);
    CHECK(p.ksteps == 7 && p.ksteps_max == 8 && p.nqt == 3 && p.qpad == 384 && p.ngroups == 19, "plan: padding");
    CHECK(p.nsplit * p.rows_per_split >= 65536 + 37 && p.rows_per_split % 32 == 0 && p.nblocks == 2050, "plan: splits");
    CHECK(dvf::bf16_rn(1.0f) == 0x3F80 && dvf::bf16_rn(1.00390625f) == 0x3F80 && dvf::bf16_rn(1.01171875f) == 0x3F82,
          "bf16 rounds to nearest even");
    if (failures == 0) std::printf("diverg filter ok\n");
    return failures ? 1 : 0;
}
