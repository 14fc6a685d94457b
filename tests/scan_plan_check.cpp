// Stand-alone print-out of scan_make_plan (nmslib_zig_amd/csrc/kernels/kernels.hpp, included as it is): built by
// tests/test_scan_plan_cpu.py with the host sanitizers.  One line per grid point,
//   n nq k tq_asked nsplit rows_per_split kl P tq
// which the test compares with the Python restatement (tests/scan_plan_ref.py).
#include <cstdio>

#include "../nmslib_zig_amd/csrc/kernels/kernels.hpp"

using namespace gfxknn;

int main() {
    const int ns[] = {1, 63, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 12289, 100000};
    const int nqs[] = {1, 7, 8, 9, 15, 16, 17, 16376, 16377, 32752, 32753};
    const int ks[] = {1, 256, 257, 768, 769, 1024, 1025, 2730, 2731, 4096, 4097, 8192, 8193};
    const int tqs[] = {1, 8, 16};
    static_assert(kScanMaxKl == 4096, "the split list limit the restatement holds");
    static_assert(kStrTileQ == 8 && kSparseTileQ == 8 && kDivergTileQ == 16, "the tiles the grid asks for");
    long cases = 0;
    for (int n : ns)
        for (int nq : nqs)
            for (int k : ks)
                for (int tq : tqs) {
                    const ScanPlan p = scan_make_plan(n, nq, k, tq);
                    if (p.n != n || p.nq != nq || p.k != k) {
                        std::printf("FAIL the plan does not carry its batch: n=%d nq=%d k=%d\n", n, nq, k);
                        return 1;
                    }
                    std::printf("%d %d %d %d %d %d %d %d %d\n", n, nq, k, tq, p.nsplit, p.rows_per_split, p.kl, p.P, p.tq);
                    ++cases;
                }
    std::printf("%ld cases\nscan plan ok\n", cases);
    return 0;
}
