// Stand-alone check of nmslib_zig_amd/csrc/hnsw_inwalk_plan.hpp (no HIP, nothing of the engine): built by
// tests/test_hnsw_inwalk_cpu.py with the host sanitizers.  Which batches the in-walk kernel serves -- cap = max(ef, k) at 1,
// 1024 and 1025 reached through ef and through k, frontier arrays of 64 .. 256 entries and beyond -- the LDS bytes of a
// workgroup, and that a query which does not fit into LDS beside the arrays is left to the two-stage route.
#include <cstdio>

#include "../nmslib_zig_amd/csrc/hnsw_inwalk_plan.hpp"

using namespace gfxknn;

static long failures = 0, cases = 0;

static void expect(size_t ef, size_t k, size_t nbcap, size_t query_bytes, bool want) {
    ++cases;
    if (inwalk_served(ef, k, nbcap, query_bytes) != want) {
        ++failures;
        std::printf("FAIL ef=%zu k=%zu nbcap=%zu query_bytes=%zu: want %s\n", ef, k, nbcap, query_bytes,
                    want ? "served" : "not served");
    }
}

static void expect_lds(size_t cap, size_t nbcap, size_t query_bytes, size_t want) {
    ++cases;
    const size_t got = inwalk_lds_bytes(cap, nbcap, query_bytes);
    if (got != want || got % 16 != 0) {
        ++failures;
        std::printf("FAIL lds cap=%zu nbcap=%zu query_bytes=%zu: %zu, want %zu\n", cap, nbcap, query_bytes, got, want);
    }
}

int main() {
    static_assert(kInwalkCapMax == 1024 && kInwalkCandCap == 1024 && kInwalkNbcapMax == 256, "what the interface documents");
    static_assert((kInwalkCandCap & (kInwalkCandCap - 1)) == 0, "C is a ring");
    static_assert(kInwalkLdsMax == 160 * 1024, "the LDS of a gfx950 workgroup");
    // cap = max(ef, k)
    const size_t efk[][3] = {{128, 10, 128}, {10, 100, 100}, {64, 64, 64}, {1, 1, 1}, {1024, 1, 1024}, {1, 1024, 1024}};
    for (const auto& c : efk) {
        ++cases;
        if (inwalk_cap(c[0], c[1]) != c[2]) {
            ++failures;
            std::printf("FAIL cap ef=%zu k=%zu\n", c[0], c[1]);
        }
    }
    // the edges of cap, through ef and through k
    expect(1, 1, 64, 512, true);
    expect(32, 10, 64, 512, true);
    expect(32, 40, 64, 512, true);
    expect(1024, 10, 64, 512, true);
    expect(1025, 10, 64, 512, false);
    expect(10, 1024, 64, 512, true);
    expect(10, 1025, 64, 512, false);
    expect(1024, 1024, 256, 512, true);
    expect(0, 0, 64, 512, false);
    // the frontier arrays: multiples of 64 up to 256 (maxM0 <= 254)
    expect(128, 10, 128, 512, true);
    expect(128, 10, 192, 512, true);
    expect(128, 10, 256, 512, true);
    expect(128, 10, 320, 512, false);
    expect(128, 10, 100, 512, false);
    // LDS: the query in units of 16 bytes, positions and distances, 64 sort keys, W with an even number of keys, C
    expect_lds(128, 64, 512, 512 + 64 * 8 + 512 + 128 * 8 + 8192);
    expect_lds(1, 64, 128, 128 + 64 * 8 + 512 + 16 + 8192);
    expect_lds(33, 64, 64, 64 + 64 * 8 + 512 + 34 * 8 + 8192);
    expect_lds(1024, 256, 520, 528 + 256 * 8 + 512 + 8192 + 8192);   // the largest arrays: 19 456 bytes and the query
    expect_lds(10, 128, 4, 16 + 128 * 8 + 512 + 80 + 8192);
    // the longest query beside the largest arrays
    const size_t qmax = kInwalkLdsMax - (256 * 8 + 512 + 8192 + 8192);
    expect(1024, 10, 256, qmax, true);
    expect(1024, 10, 256, qmax + 1, false);
    expect(32, 10, 64, qmax + 1, true);                              // smaller arrays: the same query fits
    expect(32, 10, 64, kInwalkLdsMax, false);
    std::printf("%ld cases, %ld failures\n", cases, failures);
    if (failures == 0) std::printf("inwalk plan ok\n");
    return failures == 0 ? 0 : 1;
}
