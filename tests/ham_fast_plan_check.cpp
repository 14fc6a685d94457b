// Stand-alone check of nmslib_zig_amd/csrc/ham_fast_plan.hpp (no HIP), built and run by tests/test_ham_fast_plan_cpu.py:
// the gate at its edges, and for every served plan that the splits cover every row once, within 65 536 rows each, in whole
// row blocks, with nsplit * k <= 8192 and a workgroup's LDS within the 160 KiB of a compute unit.
#include <cstdio>
#include <initializer_list>

#include "../nmslib_zig_amd/csrc/ham_fast_plan.hpp"

using namespace gfxknn::hamfast;

static int failures = 0;
#define CHECK(c)                                        \
    do {                                                \
        if (!(c)) {                                     \
            ++failures;                                 \
            std::printf("FAIL line %d: %s\n", __LINE__, #c); \
        }                                               \
    } while (0)

int main() {
    CHECK(plan(true, 65536, 256, 10, 40).use);
    CHECK(plan(true, 65536, 256, 128, 1024).use);
    CHECK(plan(true, 65536, 256, 1, 1).use);
    CHECK(!plan(false, 65536, 256, 10, 40).use);   // HNSW
    CHECK(!plan(true, 65535, 256, 10, 40).use);
    CHECK(!plan(true, 65536, 255, 10, 40).use);
    CHECK(!plan(true, 65536, 256, 129, 40).use);
    CHECK(!plan(true, 65536, 256, 0, 40).use);
    CHECK(!plan(true, 65536, 256, 10, 1025).use);
    CHECK(!plan(true, 5000000, 1024, 128, 256).use);   // 77 splits of 65 536 rows x 128 keys do not merge in LDS
    const long long ns[] = {65536, 65536 + 77, 1000000, 5000000}, nqs[] = {256, 257, 1024, 32768}, ks[] = {1, 10, 100, 128};
    for (long long n : ns)
        for (long long nq : nqs)
            for (long long k : ks)
                for (long long bits : {40ll, 256ll, 1024ll}) {
                    const Plan p = plan(true, n, nq, k, bits);
                    if (n == 5000000 && k > 100) {
                        CHECK(!p.use);
                        continue;
                    }
                    CHECK(p.use);
                    CHECK(p.W == (bits + 31) / 32 && p.tile == 32 * p.qb && (long long)p.ntiles * p.tile >= nq);
                    CHECK(p.rows_per_split % kRowBlock == 0 && p.rows_per_split <= 65536);
                    CHECK((long long)p.nsplit * p.rows_per_split >= n && (long long)(p.nsplit - 1) * p.rows_per_split < n);
                    CHECK((long long)p.nsplit * k <= 8192);
                    CHECK(p.cap >= k + 32 && p.tile == 64);
                    CHECK(p.lds == ((size_t)p.W + p.cap + 1) * 256 && p.lds <= 160 * 1024);
                    CHECK(p.sample_nsplit >= 1 && p.sample_nsplit <= p.nsplit);
                    CHECK(p.sample_rows <= n && p.sample_rows >= k && p.sample_rows % (p.sample_nsplit * kRowBlock) == 0);
                }
    if (!failures) std::printf("ham fast plan ok\n");
    return failures != 0;
}
