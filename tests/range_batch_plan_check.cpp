// Stand-alone check of csrc/range_batch_plan.hpp (no HIP, nothing of the engine): prints the plan on the grid of
// tests/range_batch_plan_ref.py, one line per point, and asserts the plan's invariants on every point.
//   g++ -std=c++17 -fsanitize=address,undefined tests/range_batch_plan_check.cpp && ./a.out
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../nmslib_zig_amd/csrc/range_batch_plan.hpp"

using namespace gfxknn;

#define CHECK(c)                                                                          \
    do {                                                                                  \
        if (!(c)) {                                                                       \
            std::printf("FAILED %s at line %d (n %zu dim %zu elem %zu nq %zu budget %zu)\n", #c, __LINE__, n, dim, elem, nq, \
                        budget);                                                          \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

int main() {
    const size_t N[] = {0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 262144, 263173, 1000000};
    const size_t DIM[][2] = {{4, 1}, {4, 5}, {4, 64}, {4, 65}, {4, 128}, {4, 129}, {4, 256}, {4, 257}, {4, 768}, {1, 128}, {1, 64}};
    const size_t Q[] = {0, 1, 31, 32, 33, 64, 65, 1024, 32768, 32769};
    const size_t CAP[] = {0, 128};
    const size_t HALVES[] = {1, 2, 4, 5};
    size_t cases = 0;
    for (size_t n : N) {
        std::vector<size_t> budgets{kRangeBatchWsBytes};
        for (size_t h : HALVES) budgets.push_back(range_batch_query_bytes(n) * h / 2);
        for (auto& ed : DIM)
            for (size_t nq : Q)
                for (size_t cap : CAP)
                    for (size_t budget : budgets) {
                        const size_t elem = ed[0], dim = ed[1];
                        const RangeBatchPlan p = range_batch_plan(n, dim, elem, nq, cap, budget);
                        std::printf("%zu %zu %zu %zu %zu %zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d\n", n, dim, elem, nq, cap,
                                    budget, p.route, p.rows_per_wg, p.chunks, p.query_tile, p.grid_x, p.grid_y, p.mask_words,
                                    p.blocks, p.slice_queries, p.slices, p.workspace_bytes, (int)p.count_only);
                        ++cases;
                        CHECK(p.route == 10 || p.route == 11);
                        CHECK(p.count_only == (cap == 0));
                        if (p.route == 11) {
                            CHECK(p.slices == 0 && p.slice_queries == 0 && p.workspace_bytes == 0 && p.grid_x == 0);
                            // what the batched kernels do not serve: long rows, no room for one query's masks, nothing to do
                            CHECK(nq == 0 || (elem == 4 && (dim == 0 || dim > kRangeBatchMaxDim)) || (elem == 1 && dim != 128) ||
                                  range_batch_query_bytes(n) > budget);
                            continue;
                        }
                        // a slice holds at least one query and its workspace stays within the bound
                        CHECK(p.slice_queries >= 1 && p.slice_queries <= kRangeBatchMaxSliceQueries);
                        CHECK(p.workspace_bytes <= budget);
                        CHECK(p.workspace_bytes == p.slice_queries * (p.mask_words * 8 + (p.blocks + 1) * 4));
                        // the slices cover every query once
                        size_t covered = 0;
                        for (size_t s = 0; s < p.slices; ++s) {
                            const size_t m = range_batch_slice_size(p, nq, s);
                            CHECK(m >= 1 && m <= p.slice_queries && s * p.slice_queries == covered);
                            covered += m;
                        }
                        CHECK(covered == nq && range_batch_slice_size(p, nq, p.slices) == 0);
                        // the grid covers every row once: one workgroup per 256 rows, none without a row
                        CHECK(p.rows_per_wg == 256 && p.grid_x * p.rows_per_wg >= n && (p.grid_x == 0 || (p.grid_x - 1) * p.rows_per_wg < n));
                        CHECK(p.mask_words * 64 >= n && (p.mask_words == 0 || (p.mask_words - 1) * 64 < n));
                        CHECK(p.blocks * 1024 >= n && (p.blocks == 0 || (p.blocks - 1) * 1024 < n));
                        // every query tile belongs to one query split
                        const size_t tiles = (p.slice_queries + p.query_tile - 1) / p.query_tile;
                        CHECK(p.grid_y >= 1 && p.grid_y <= tiles);
                        CHECK(p.chunks >= 1 && p.chunks <= 4 && (elem == 1 || p.chunks * 64 >= dim));
                    }
    }
    std::printf("%zu cases\nrange batch plan ok\n", cases);
    return 0;
}
