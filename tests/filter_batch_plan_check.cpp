// Stand-alone driver of nmslib_zig_amd/csrc/filter_batch_plan.hpp (no HIP, nothing of the engine): reads cases from the file
// named on the command line and prints every plan, for tests/test_filter_each_cpu.py to compare with numpy's stable argsort.
//   file:   <cases>, then per case "<nq> <n_filters>", a line of nq entries of filter_of_query, a line of n_filters segments
//   output: per case five lines -- "perm ...", "inv ...", "seg s0 s1 s2 s3", "groups f b e ...", "identity 0|1" -- then
//           "filter batch plan ok".
// It also checks what needs no second opinion: filter_batch_first_bad on entries at and beyond both ends of the range.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <vector>

#include "../nmslib_zig_amd/csrc/filter_batch_plan.hpp"

using namespace gfxknn;

static void require(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        std::exit(1);
    }
}

int main(int argc, char** argv) {
    const int32_t ok3[] = {-1, 0, 2, 1}, low[] = {0, -2, 5}, high[] = {0, 1, 3}, none[] = {-1, 0};
    require(filter_batch_first_bad(ok3, 4, 3) == 4, "entries in range");
    require(filter_batch_first_bad(low, 3, 3) == 1, "an entry below -1");
    require(filter_batch_first_bad(high, 3, 3) == 2, "an entry at n_filters");
    require(filter_batch_first_bad(none, 2, 0) == 1, "n_filters = 0 takes only -1");
    require(filter_batch_first_bad(nullptr, 0, 0) == 0, "an empty batch");

    require(argc == 2, "usage: filter_batch_plan_check <cases file>");
    std::ifstream in(argv[1]);
    size_t cases = 0;
    in >> cases;
    for (size_t c = 0; c < cases; ++c) {
        size_t nq = 0, nf = 0;
        in >> nq >> nf;
        std::vector<int32_t> fq(nq);
        std::vector<int> seg(nf);
        for (auto& v : fq) in >> v;
        for (auto& v : seg) in >> v;
        require((bool)in, "the cases file is complete");
        const FilterBatchPlan p = filter_batch_plan(fq.data(), nq, seg.data(), nf);
        require(p.perm.size() == nq && p.inv.size() == nq, "one entry per query");
        std::printf("perm");
        for (int32_t v : p.perm) std::printf(" %d", v);
        std::printf("\ninv");
        for (int32_t v : p.inv) std::printf(" %d", v);
        std::printf("\nseg %zu %zu %zu %zu\ngroups", p.seg[0], p.seg[1], p.seg[2], p.seg[3]);
        for (const FilterBatchGroup& g : p.groups) std::printf(" %d %zu %zu", g.filter, g.begin, g.end);
        std::printf("\nidentity %d\n", p.identity ? 1 : 0);
    }
    std::printf("filter batch plan ok\n");
    return 0;
}
