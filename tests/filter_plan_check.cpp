// Stand-alone check of nmslib_zig_amd/csrc/filter_plan.hpp (no HIP, nothing of the engine): built by
// tests/test_filter_plan_cpu.py with the host sanitizers.  The route of a filtered HNSW batch at m = 0, k', k' + 1,
// scan_rows, scan_rows + 1, 4096 and 4097, for ef < k and ef > k, with and without a scan_rows; the LDS the scan takes, and
// that a scan which does not fit into LDS is left to the walk.
#include <cstdio>

#include "../nmslib_zig_amd/csrc/filter_plan.hpp"

using namespace gfxknn;

static long failures = 0, cases = 0;

static void expect(size_t m, size_t ef, size_t k, size_t scan_rows, FilterRoute want, size_t query_bytes = 512) {
    ++cases;
    if (filter_route(m, ef, k, scan_rows, query_bytes) != want) {
        ++failures;
        std::printf("FAIL m=%zu ef=%zu k=%zu scan_rows=%zu query_bytes=%zu: want %s\n", m, ef, k, scan_rows, query_bytes,
                    want == FilterRoute::Subset ? "subset" : "walk");
    }
}

int main() {
    const FilterRoute S = FilterRoute::Subset, W = FilterRoute::Walk;
    static_assert(kFilterSubsetMax == 4096, "the capacity the interface documents");
    // (ef, k): ef > k, ef < k, ef = k
    const size_t efk[][2] = {{128, 10}, {10, 100}, {64, 64}};
    for (const auto& c : efk) {
        const size_t ef = c[0], k = c[1], kp = ef > k ? ef : k;
        if (filter_walk_results(ef, k) != kp) {
            ++failures;
            std::printf("FAIL walk results ef=%zu k=%zu\n", ef, k);
        }
        // no scan_rows: the bound is k'
        expect(0, ef, k, 0, S);
        expect(1, ef, k, 0, S);
        expect(kp, ef, k, 0, S);
        expect(kp + 1, ef, k, 0, W);
        expect(4096, ef, k, 0, W);
        expect(4097, ef, k, 0, W);
        // scan_rows below k' changes nothing
        expect(kp, ef, k, kp / 2, S);
        expect(kp + 1, ef, k, kp / 2, W);
        // scan_rows above k' moves the bound there
        const size_t sr = 1000;
        expect(0, ef, k, sr, S);
        expect(kp + 1, ef, k, sr, S);
        expect(sr, ef, k, sr, S);
        expect(sr + 1, ef, k, sr, W);
        expect(4096, ef, k, sr, W);
        // scan_rows at the capacity: up to 4096, never beyond
        expect(sr + 1, ef, k, 4096, S);
        expect(4096, ef, k, 4096, S);
        expect(4097, ef, k, 4096, W);
    }
    // k' beyond the capacity (a large efSearch or k): the capacity still holds
    expect(4096, 5000, 10, 0, S);
    expect(4097, 5000, 10, 0, W);
    expect(4097, 10, 5000, 0, W);
    expect(5000, 10, 5000, 4096, W);
    // LDS: keys padded to a power of two (at least 64) of 8 bytes, the query, 2 KB of per-wave scratch, 16 bytes
    static_assert(kFilterLdsMax == 160 * 1024, "the LDS of a gfx950 workgroup");
    const size_t keys[][2] = {{0, 64}, {1, 64}, {64, 64}, {65, 128}, {1000, 1024}, {2048, 2048}, {2049, 4096}, {4096, 4096}};
    for (const auto& c : keys) {
        ++cases;
        if (filter_subset_keys(c[0]) != c[1] || filter_subset_lds_bytes(c[0], 512) != c[1] * 8 + 512 + 2048 + 16) {
            ++failures;
            std::printf("FAIL lds m=%zu\n", c[0]);
        }
    }
    // the longest query beside 4096 keys: 160 KB - 32 KB - 2 KB - 16 = 129008 bytes (32 252 floats)
    const size_t qmax = kFilterLdsMax - 4096 * 8 - 2048 - 16;
    expect(4096, 64, 10, 4096, S, qmax);
    expect(4096, 64, 10, 4096, W, qmax + 4);
    expect(2049, 64, 10, 4096, W, qmax + 4);
    expect(2048, 64, 10, 4096, S, qmax + 4);   // half the keys: the same query fits
    expect(64, 64, 10, 0, S, qmax + 4);
    expect(64, 64, 10, 0, W, kFilterLdsMax);   // no room for any key
    std::printf("%ld cases, %ld failures\n", cases, failures);
    if (failures == 0) std::printf("filter plan ok\n");
    return failures == 0 ? 0 : 1;
}
