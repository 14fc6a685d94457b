// Stand-alone print-out of the HNSW search planners (nmslib_zig_amd/csrc/hnsw_plan.cpp and kernels/kernels.hpp, compiled
// as they are): built by tests/test_hnsw_plan_cpu.py with the host sanitizers.  One line per grid point and planner,
//   L u8 n ldv maxM maxM0 k ef force | cap table_size table_shift bitset_words lds_bytes nbcap big_lds wide emax
//   O u8 n ldv maxM maxM0 k ef force heap_cap_asked | cap table_size table_shift bitset_words lds_bytes heap_lds heap_cap
//     a_in_lds r_in_lds ws_a ws_r ws_heap
// which the test compares with the Python restatement (tests/hnsw_plan_ref.py).
#include <cstdio>

#include "../nmslib_zig_amd/csrc/kernels/kernels.hpp"

using namespace gfxknn;

int main() {
    const int caps[] = {1, 56, 57, 64, 65, 113, 114, 128, 129, 227, 228, 256, 257, 1024, 1025, 2048, 2049, 8192, 8193};
    const int m0s[] = {4, 12, 16, 17, 32, 62, 63, 64, 126, 127, 128, 191, 192, 254, 255, 256, 300};
    const int more_m[][2] = {{70, 20}, {62, 20}, {63, 20}, {255, 100}, {256, 100}, {0, 0}};   // maxM, maxM0
    const int ldvs[] = {8, 128, 768, 1664, 4096, 5760, 5768, 6000, 9000, 13968, 13976, 14000, 14056, 14064, 16120, 16128, 16384,
                        40584, 40592, 40696, 40704};
    const int ns[] = {1, 2, 2046, 2047, 2048, 100000};
    static_assert(HNSW_NBCAP_LDS == 256 && HNSW_LDS_LIMIT == 160 * 1024, "the limits the restatement holds");
    long lines = 0;
    auto point = [&](int u8, int n, int ldv, int maxM, int maxM0, int k, int ef) {
        HnswDeviceGraph g{};
        g.space = u8 ? SP_L2SQR_SIFT : SP_L2SQR;
        g.n = n;
        g.ldv = ldv;
        g.dim = ldv;
        g.maxM = maxM;
        g.maxM0 = maxM0;
        for (int force = 0; force < 2; ++force) {
            const HnswSearchPlan p = hnsw_make_plan(g, 7, k, ef, force != 0);
            if (p.nq != 7 || p.k != k || p.ef != ef || p.rows_f16 != 0) {
                std::printf("FAIL the plan does not carry its batch: k=%d ef=%d\n", k, ef);
                return false;
            }
            std::printf("L %d %d %d %d %d %d %d %d | %d %d %d %zu %zu %d %zu %d %d\n", u8, n, ldv, maxM, maxM0, k, ef, force, p.cap,
                        p.table_size, p.table_shift, p.bitset_words, p.lds_bytes, hnsw_nbcap(g), hnsw_big_lds(g),
                        (int)hnsw_wide(g), hnsw_emax(p.cap));
            ++lines;
            for (int heap_cap : {0, n + 1}) {
                const HnswSearchPlan o = hnsw_make_plan_old(g, 7, k, ef, force != 0, heap_cap);
                std::printf("O %d %d %d %d %d %d %d %d %d | %d %d %d %zu %zu %d %d %d %d %zu %zu %zu\n", u8, n, ldv, maxM, maxM0,
                            k, ef, force, heap_cap, o.cap, o.table_size, o.table_shift, o.bitset_words, o.lds_bytes, o.heap_lds,
                            o.heap_cap, o.a_in_lds, o.r_in_lds, hnsw_old_ws_a(o), hnsw_old_ws_r(o), hnsw_old_ws_heap(o));
                ++lines;
            }
        }
        return true;
    };
    for (int u8 = 0; u8 < 2; ++u8)
        for (int n : ns)
            for (int ldv : ldvs)
                for (int cap : caps) {
                    // (n moves the bitset and SearchOld's heap only: crossed with one row length)
                    if (n != 100000 && ldv != 128) continue;
                    // the cap reached through ef and through k > ef
                    const int efk[][2] = {{cap, cap < 10 ? cap : 10}, {cap < 5 ? cap : 5, cap}};
                    for (const auto& e : efk) {
                        for (int m0 : m0s)
                            if (!point(u8, n, ldv, m0 / 2, m0, e[1], e[0])) return 1;
                        for (const auto& m : more_m)
                            if (!point(u8, n, ldv, m[0], m[1], e[1], e[0])) return 1;
                    }
                }
    std::printf("%ld lines\nhnsw plan ok\n", lines);
    return 0;
}
