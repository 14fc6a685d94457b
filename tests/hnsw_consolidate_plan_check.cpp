// Stand-alone check of nmslib_zig_amd/csrc/hnsw_consolidate_plan.hpp (no HIP, nothing of the engine): built by
// tests/test_hnsw_consolidate_plan_cpu.py with the host sanitizers.  Cases: new positions at the word edges 0 / 31 / 32 /
// 63 / 64 / n - 1 with n % 32 != 0, a bitset shorter than the rows, all dead, none dead; the upper-level offsets of nodes
// that move past removed upper-level nodes; a deleted entry point with ties on the top level; a live one that stays.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../nmslib_zig_amd/csrc/hnsw_consolidate_plan.hpp"

using namespace gfxknn;

static long failures = 0, cases = 0;
#define CHECK(c, ...)                             \
    do {                                          \
        if (!(c)) {                               \
            if (++failures <= 20) {               \
                std::printf("FAIL " __VA_ARGS__); \
                std::printf("\n");                \
            }                                     \
        }                                         \
    } while (0)

static std::vector<uint32_t> bitset_of(const std::vector<size_t>& dead, size_t n) {
    std::vector<uint32_t> t((n + 31) / 32, 0);
    for (size_t p : dead) t[p >> 5] |= 1u << (p & 31);
    return t;
}

// positions, levels, offsets and entry point against a restatement that walks the rows one by one
static void check_case(const std::vector<uint32_t>& tomb, const std::vector<int32_t>& levels, int maxM, int enter,
                       const char* what) {
    ++cases;
    const size_t n = levels.size();
    std::vector<int32_t> newpos;
    const size_t live = consolidate_positions(tomb, n, newpos);
    CHECK(newpos.size() == n, "%s: newpos size", what);
    size_t rank = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool dead = (i >> 5) < tomb.size() && ((tomb[i >> 5] >> (i & 31)) & 1u);
        CHECK(tomb_bit(tomb, i) == dead, "%s: tomb_bit(%zu)", what, i);
        if (dead) CHECK(newpos[i] == -1, "%s: dead row %zu has position %d", what, i, newpos[i]);
        else CHECK(newpos[i] == (int32_t)rank++, "%s: live row %zu at %d", what, i, newpos[i]);
    }
    CHECK(live == rank, "%s: live count %zu != %zu", what, live, rank);

    std::vector<int32_t> nl, up_nodes;
    std::vector<int64_t> noff;
    const size_t up_ints = consolidate_up_offsets(levels, newpos, maxM, nl, noff, up_nodes);
    CHECK(nl.size() == live && noff.size() == live, "%s: sizes of the new levels / offsets", what);
    size_t at = 0, k = 0;
    for (size_t i = 0; i < n; ++i) {
        if (newpos[i] < 0) continue;
        const size_t p = (size_t)newpos[i];
        CHECK(nl[p] == levels[i], "%s: level of row %zu", what, i);
        if (levels[i] > 0) {
            CHECK(noff[p] == (int64_t)at, "%s: offset of row %zu is %lld, expected %zu", what, i, (long long)noff[p], at);
            CHECK(k < up_nodes.size() && up_nodes[k] == (int32_t)i, "%s: up_nodes[%zu]", what, k);
            ++k;
            at += (size_t)levels[i] * (size_t)(maxM + 1);
        } else {
            CHECK(noff[p] == -1, "%s: a level-0 row %zu has an offset", what, i);
        }
    }
    CHECK(k == up_nodes.size() && at == up_ints, "%s: %zu upper nodes, %zu ints", what, up_nodes.size(), up_ints);

    int e = enter, top = enter >= 0 ? levels[(size_t)enter] : 0;
    const int top_before = top;
    consolidate_entry(levels, newpos, e, top);
    if (enter >= 0 && newpos[(size_t)enter] >= 0) {
        CHECK(e == enter && top == top_before, "%s: a live entry point moved", what);
    } else {
        int be = -1, bl = 0;
        for (size_t i = 0; i < n; ++i)
            if (newpos[i] >= 0 && (be < 0 || levels[i] > bl)) be = (int)i, bl = levels[i];
        CHECK(e == be && top == bl, "%s: entry %d level %d, expected %d level %d", what, e, top, be, bl);
        for (size_t i = 0; i < n && e >= 0; ++i)
            if (newpos[i] >= 0)
                CHECK(levels[i] < top || (levels[i] == top && (int)i >= e), "%s: row %zu beats the entry point", what, i);
    }
}

int main() {
    std::mt19937 rng(20260419);
    for (size_t n : {1u, 31u, 33u, 65u, 70u, 1000u + 7u}) {
        std::vector<int32_t> levels(n);
        for (auto& l : levels) {
            l = 0;
            while (rng() % 4 == 0 && l < 5) ++l;
        }
        const int tall = (int)(n / 2);
        levels[(size_t)tall] = 6;
        if (n > 40) levels[n - 3] = 6, levels[5] = 6;   // ties on the top level
        // the word edges
        std::vector<size_t> edges;
        for (size_t p : {(size_t)0, (size_t)31, (size_t)32, (size_t)63, (size_t)64, n - 1})
            if (p < n) edges.push_back(p);
        check_case(bitset_of(edges, n), levels, 16, tall, "word edges");
        check_case(bitset_of({}, n), levels, 16, tall, "none dead");
        check_case(std::vector<uint32_t>{}, levels, 16, tall, "no bitset at all");
        std::vector<size_t> all(n);
        for (size_t i = 0; i < n; ++i) all[i] = i;
        check_case(bitset_of(all, n), levels, 16, tall, "all dead");
        // the entry point and, step by step, every node of the top level
        std::vector<size_t> tops{(size_t)tall};
        check_case(bitset_of(tops, n), levels, 16, tall, "entry point dead");
        if (n > 40) {
            tops.push_back(5);
            check_case(bitset_of(tops, n), levels, 5, tall, "entry point and the first tie dead");
            tops.push_back(n - 3);
            check_case(bitset_of(tops, n), levels, 5, tall, "the whole top level dead");
        }
        // a bitset shorter than the rows: the rows beyond it are live
        if (n > 40) {
            std::vector<uint32_t> shorter{0x80000001u};
            check_case(shorter, levels, 16, 0, "short bitset, entry point 0 dead");
        }
        // random shares, among them upper-level nodes that go so that later blocks move down
        for (int share : {10, 30, 50, 90}) {
            std::vector<size_t> dead;
            for (size_t i = 0; i < n; ++i)
                if ((int)(rng() % 100) < share) dead.push_back(i);
            check_case(bitset_of(dead, n), levels, 1 + (int)(rng() % 40), (int)(rng() % n), "random");
        }
    }
    // one explicit case: rows 1 and 2 (levels 2 and 1) go, row 3 (level 1) moves to offset 0 + nothing before it but row 0's block
    {
        const std::vector<int32_t> levels{1, 2, 1, 1, 0, 3};
        std::vector<int32_t> newpos, nl, up;
        std::vector<int64_t> off;
        const size_t live = consolidate_positions(bitset_of({1, 2}, 6), 6, newpos);
        const size_t ints = consolidate_up_offsets(levels, newpos, 4, nl, off, up);
        CHECK(live == 4 && newpos == (std::vector<int32_t>{0, -1, -1, 1, 2, 3}), "explicit: positions");
        CHECK(off == (std::vector<int64_t>{0, 5, -1, 10}) && ints == 25, "explicit: offsets");
        CHECK(nl == (std::vector<int32_t>{1, 1, 0, 3}) && up == (std::vector<int32_t>{0, 3, 5}), "explicit: levels, up_nodes");
        ++cases;
    }
    if (failures) {
        std::printf("%ld failures\n", failures);
        return 1;
    }
    std::printf("hnsw consolidate plan ok: %ld cases\n", cases);
    return 0;
}
