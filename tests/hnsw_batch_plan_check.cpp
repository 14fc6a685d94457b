// Stand-alone check of nmslib_zig_amd/csrc/hnsw_batch_plan.hpp (no HIP, nothing of the engine): built by
// tests/test_hnsw_batch_plan_cpu.py with the host sanitizers.  It drives the header the way the GPU builder's batch loop does
// (batch_end, plan_pairs, raise_top from the state that node 0 leaves) over four level streams, forward and in reverse
// order, and checks the tiling of [first, n), the rule that ends a batch, the contents of every batch, the append property
//  for every `first`, and that assign_up_offsets may be called in two parts.
//
// A batch's pairs are a function of (next, end, top) and the levels.  The runs that the append property compares meet the
// same triples thousands of times, so each kind of run (the pass over everything with its reused BatchPairs, as the engine
// has it; the run started at `first` with a BatchPairs of its own) plans a triple once and remembers a hash of pts, src
// and base; that the two runs reach the same triples is asserted batch by batch for every `first`.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include "../nmslib_zig_amd/csrc/hnsw_batch_plan.hpp"

using namespace gfxknn;

static long failures = 0;
#define CHECK(c, ...)                         \
    do {                                      \
        if (!(c)) {                           \
            if (++failures <= 20) {           \
                std::printf("FAIL " __VA_ARGS__); \
                std::printf("\n");            \
            }                                 \
        }                                     \
    } while (0)

struct Step {  // one batch of a run, and the state it leaves
    size_t next, end;
    int top, maxlevel, enterpoint;
    uint64_t pairs;  // hash of pts, src, base
    bool operator==(const Step& o) const {
        return next == o.next && end == o.end && top == o.top && maxlevel == o.maxlevel && enterpoint == o.enterpoint &&
               pairs == o.pairs;
    }
};

static uint64_t hash_pairs(const BatchPairs& p) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) { h = (h ^ v) * 1099511628211ull; };
    mix((uint64_t)p.top);
    mix(p.pts.size());
    for (int32_t v : p.pts) mix((uint32_t)v);
    for (int32_t v : p.src) mix((uint32_t)v);
    for (size_t v : p.base) mix(v);
    return h;
}

// pts is level-major from top down to 0, a node appears at levels 0 .. min(level, top) in position order, src names the same
// node one level up (-1 at its highest slice), and the slices cover pts without remainder
static void check_pairs(const BatchSchedule& s, const std::vector<int32_t>& levels, size_t next, size_t end, int top,
                        const BatchPairs& p) {
    CHECK(p.top == top && p.base.size() == (size_t)top + 2 && p.src.size() == p.pts.size(), "pairs header at %zu", next);
    CHECK(p.slice_begin(top) == 0 && p.slice_begin(0) + p.slice_size(0) == p.pts.size(), "slices do not span pts at %zu", next);
    size_t at = 0;
    for (int l = top; l >= 0; --l) {
        CHECK(p.slice_begin(l) == at, "slice %d of batch %zu begins at %zu, not %zu", l, next, p.slice_begin(l), at);
        for (size_t i = next; i < end; ++i) {
            const size_t node = s.node_at(i);
            const int hi = std::min(levels[node], top);
            if (hi < l) continue;
            if (at >= p.pts.size()) {
                CHECK(false, "pts of batch %zu is short", next);
                return;
            }
            CHECK(p.pts[at] == (int32_t)node, "pts[%zu] of batch %zu", at, next);
            const int32_t up = p.src[at];
            if (l == hi) CHECK(up == -1, "src[%zu] of batch %zu is not -1 at the node's highest slice", at, next);
            else
                CHECK(up >= 0 && (size_t)up >= p.slice_begin(l + 1) && (size_t)up < p.slice_begin(l + 1) + p.slice_size(l + 1) &&
                          p.pts[(size_t)up] == (int32_t)node,
                      "src[%zu] of batch %zu is not the node one level up", at, next);
            ++at;
        }
        CHECK(at == p.slice_begin(l) + p.slice_size(l), "slice %d of batch %zu has the wrong size", l, next);
    }
    CHECK(at == p.pts.size(), "pts of batch %zu has a remainder", next);
}

// the size rule clamp(next / div, 1, max_batch), the cut, and "the first position above the running top level ends the batch"
static void check_batch_end(const BatchSchedule& s, const std::vector<int32_t>& levels, size_t next, size_t end, int top) {
    CHECK(end > next && end <= s.n && end - next <= (size_t)s.max_batch, "batch [%zu, %zu) is empty or too long", next, end);
    CHECK(!(next < s.cut && s.cut < end), "batch [%zu, %zu) spans the cut %zu", next, end, s.cut);
    size_t rule = std::min<size_t>(std::max<size_t>(next / (size_t)s.batch_div, 1), (size_t)s.max_batch);
    rule = std::min(s.n, next + rule);
    if (next < s.cut) rule = std::min(rule, s.cut);
    size_t riser = next;
    while (riser < rule && levels[s.node_at(riser)] <= top) ++riser;
    CHECK(end == (riser < rule ? riser + 1 : rule), "batch [%zu, %zu): the rule says %zu", next, end, riser < rule ? riser + 1 : rule);
}

struct Runner {
    const std::vector<int32_t>& levels;
    BatchPairs pairs;  // reused from batch to batch, as in the builder
    // planned triples: by next, (end, hash); top is a function of next (asserted in run)
    std::vector<std::vector<std::pair<size_t, uint64_t>>> seen;
    std::vector<int> top_at;

    Runner(const std::vector<int32_t>& lv, size_t n) : levels(lv), seen(n), top_at(n, -1) {}

    std::vector<Step> run(const BatchSchedule& s, size_t first, int maxlevel, int enterpoint) {
        std::vector<Step> steps;
        steps.reserve(s.n - std::min(first, s.n));
        for (size_t next = first, end; next < s.n; next = end) {
            end = s.batch_end(next, levels, maxlevel);
            const int top = maxlevel;
            check_batch_end(s, levels, next, end, top);
            if (end <= next) break;  // (reported above)
            CHECK(top_at[next] < 0 || top_at[next] == top, "top level at %zu differs between runs", next);
            top_at[next] = top;
            uint64_t h = 0;
            bool known = false;
            for (const auto& e : seen[next])
                if (e.first == end) {
                    h = e.second;
                    known = true;
                    break;
                }
            if (!known) {
                plan_pairs(s, levels, next, end, top, pairs);
                check_pairs(s, levels, next, end, top, pairs);
                h = hash_pairs(pairs);
                seen[next].push_back({end, h});
            }
            const int enter_before = enterpoint;
            raise_top(s, levels, next, end, maxlevel, enterpoint);
            const size_t last = s.node_at(end - 1);  // only a batch's last position can lie above the top level
            if (levels[last] > top)
                CHECK(maxlevel == levels[last] && enterpoint == (int)last, "promotion after batch [%zu, %zu)", next, end);
            else
                CHECK(maxlevel == top && enterpoint == enter_before, "batch [%zu, %zu) moved the top level", next, end);
            steps.push_back({next, end, top, maxlevel, enterpoint, h});
        }
        return steps;
    }
};

static void check_tiling(const std::vector<Step>& steps, size_t first, size_t n, const char* what) {
    size_t at = first;
    for (const Step& b : steps) {
        CHECK(b.next == at && b.end > b.next, "%s: gap, overlap or empty batch at %zu", what, at);
        at = b.end;
    }
    CHECK(at == std::max(first, n), "%s: batches end at %zu, not %zu", what, at, n);
}

// level of the node at insertion position pos
static int stream_level(int stream, size_t pos, size_t n, std::mt19937& rng) {
    switch (stream) {
        case 0: {  // geometric, p = 1/4
            int l = 0;
            while (l < 12 && (rng() & 3u) == 0) ++l;
            return l;
        }
        case 1: return 0;
        case 2: return (int)pos;  // strictly increasing: every node promotes
        default: return pos == n / 2 ? 5 : 0;  // one tall node in the middle
    }
}

static long batches_checked = 0, firsts_checked = 0;

static void check_shape(int stream, size_t n, bool reverse, int div, int max_batch) {
    BatchSchedule sch{n, reverse, div, max_batch, 0};
    CHECK(sch.node_at(0) == 0, "position 0 is not node 0");
    for (size_t i = 1; i < n; ++i) CHECK(sch.node_at(i) == (reverse ? n - i : i), "node_at(%zu)", i);
    std::vector<int32_t> levels(n);
    std::mt19937 rng(12345u + (unsigned)stream);
    for (size_t pos = 0; pos < n; ++pos) levels[sch.node_at(pos)] = stream_level(stream, pos, n, rng);

    Runner whole(levels, n), started(levels, n);
    const std::vector<Step> plain = whole.run(sch, 1, levels[0], 0);  // the pass: node 0 is in the graph
    check_tiling(plain, 1, n, "pass");
    batches_checked += (long)plain.size();
    for (size_t first = 1; first < n; ++first) {
        sch.cut = first;
        const std::vector<Step> full = whole.run(sch, 1, levels[0], 0);
        check_tiling(full, 1, n, "pass with a cut");
        size_t b = 0;
        while (b < full.size() && full[b].next != first) ++b;
        if (b == full.size()) {
            CHECK(false, "the cut %zu is no batch boundary", first);
            continue;
        }
        // the append: started at `first` with the top level and entry point the pass had there
        const int level0 = b ? full[b - 1].maxlevel : levels[0], enter0 = b ? full[b - 1].enterpoint : 0;
        const std::vector<Step> tail = started.run(sch, first, level0, enter0);
        check_tiling(tail, first, n, "run from the cut");
        CHECK(tail.size() == full.size() - b, "run from %zu: %zu batches, the pass has %zu from there", first, tail.size(),
              full.size() - b);
        for (size_t i = 0; i < tail.size() && b + i < full.size(); ++i)
            CHECK(tail[i] == full[b + i], "run from %zu: batch %zu differs from the pass", first, i);
        // ... and the rows before it, built when there were no others (forward order: reverse positions depend on n)
        if (!reverse) {
            BatchSchedule before{first, false, div, max_batch, 0};
            const std::vector<Step> head = whole.run(before, 1, levels[0], 0);
            CHECK(head.size() == b, "build of %zu rows: %zu batches, the pass has %zu before the cut", first, head.size(), b);
            for (size_t i = 0; i < head.size() && i < b; ++i)
                CHECK(head[i] == full[i], "build of %zu rows: batch %zu differs from the pass", first, i);
        }
        ++firsts_checked;
    }
}

static void check_up_offsets(int stream, size_t n, int maxM) {
    std::vector<int32_t> levels(n);
    std::mt19937 rng(999u + (unsigned)stream);
    for (size_t i = 0; i < n; ++i) levels[i] = stream_level(stream, i, n, rng);
    size_t all_ints = 0;
    std::vector<int64_t> all;
    assign_up_offsets(levels, 0, n, maxM, all_ints, all);
    size_t want = 0;
    CHECK(all.size() == n, "up_off has %zu entries", all.size());
    for (size_t i = 0; i < n && i < all.size(); ++i) {
        CHECK(all[i] == (levels[i] > 0 ? (int64_t)want : -1), "up_off[%zu]", i);
        want += (size_t)levels[i] * (size_t)(maxM + 1);
    }
    CHECK(all_ints == want, "up_ints %zu, not %zu", all_ints, want);
    for (size_t n0 = 0; n0 <= n; ++n0) {
        size_t ints = 0;
        std::vector<int64_t> a, b;
        assign_up_offsets(levels, 0, n0, maxM, ints, a);
        assign_up_offsets(levels, n0, n, maxM, ints, b);
        a.insert(a.end(), b.begin(), b.end());
        CHECK(ints == all_ints && a == all, "up offsets in two parts at %zu differ", n0);
    }
}

int main() {
    const size_t sizes[] = {1, 2, 17, 1000};
    const int divs[] = {1, 16}, max_batches[] = {1, 7, 4096};
    for (int stream = 0; stream < 4; ++stream)
        for (size_t n : sizes) {
            for (int reverse = 0; reverse < 2; ++reverse)
                for (int div : divs)
                    for (int mb : max_batches) check_shape(stream, n, reverse != 0, div, mb);
            check_up_offsets(stream, n, 16);
            check_up_offsets(stream, n, 1);
        }
    std::printf("%ld batches of plain passes, %ld cuts\n", batches_checked, firsts_checked);
    if (failures) {
        std::printf("%ld failures\n", failures);
        return 1;
    }
    std::printf("hnsw batch plan ok\n");
    return 0;
}
