// The GPU HNSW builder's schedule (hnsw_gpu_build.cpp): which positions make a batch, the batch's
// (node, level) pairs and where a node's upper-level lists start.  Integer arithmetic on the level stream only -- no HIP,
// nothing of the engine -- so that tests/hnsw_batch_plan_check.cpp can check it without a GPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gfxknn {

// out_up_off[i - first]: offset (ints) of node i's upper-level lists in up_links, -1 for a node of level 0, for nodes
// [first, n).  up_ints: the ints in use before `first` on entry, after n on return (a later call goes on from there).
inline void assign_up_offsets(const std::vector<int32_t>& levels, size_t first, size_t n, int maxM, size_t& up_ints,
                              std::vector<int64_t>& out_up_off) {
    out_up_off.assign(n - first, -1);
    for (size_t i = first; i < n; ++i)
        if (levels[i] > 0) {
            out_up_off[i - first] = (int64_t)up_ints;
            up_ints += (size_t)levels[i] * (size_t)(maxM + 1);
        }
}

// Insertion order and batch sizes of one pass over n rows.  Nothing here looks beyond the batch it is asked about: the
// schedule from a batch boundary on is the same whatever came before it and however many rows follow.
struct BatchSchedule {
    size_t n;
    bool reverse;              // position 0 is node 0; position i > 0 is node i, or node n - i in reverse order
    int batch_div, max_batch;  // a batch is at most 1/div of the positions before it, at most max_batch, at least one
    size_t cut;                // no batch spans this position (0: off)

    size_t node_at(size_t pos) const { return reverse && pos ? n - pos : pos; }
    // end of the batch that starts at `next`; a node that raises the top level closes its batch
    size_t batch_end(size_t next, const std::vector<int32_t>& levels, int maxlevel) const {
        size_t end = std::min(n, next + std::min<size_t>(std::max<size_t>(next / (size_t)batch_div, 1), (size_t)max_batch));
        if (next < cut) end = std::min(end, cut);
        for (size_t i = next; i < end; ++i)
            if (levels[node_at(i)] > maxlevel) return i + 1;
        return end;
    }
};

// (node, level) pairs of one batch, level-major (top level first); src = the same node's pair one level up, -1 at the node's
// highest slice.  Level l's slice is pairs [base[l], base[l - 1]) (to the end for l == 0).
struct BatchPairs {
    std::vector<int32_t> pts, src, slot;  // (slot: scratch of plan_pairs)
    std::vector<size_t> base;
    int top = 0;
    size_t slice_begin(int l) const { return base[(size_t)l]; }
    size_t slice_size(int l) const { return (l == 0 ? pts.size() : base[(size_t)l - 1]) - base[(size_t)l]; }
};

// positions [next, end) against a graph whose top level is `top`; the vectors of `out` are reused from batch to batch
inline void plan_pairs(const BatchSchedule& sch, const std::vector<int32_t>& levels, size_t next, size_t end, int top,
                       BatchPairs& out) {
    out.top = top;
    out.pts.clear();
    out.src.clear();
    out.base.assign((size_t)top + 2, 0);
    out.slot.assign(end - next, -1);  // a node's pair at the level above (its levels are contiguous from its highest down)
    for (int l = top; l >= 0; --l) {
        out.base[(size_t)l] = out.pts.size();
        for (size_t i = next; i < end; ++i) {
            if (std::min(levels[sch.node_at(i)], top) < l) continue;
            out.src.push_back(out.slot[i - next]);
            out.slot[i - next] = (int32_t)out.pts.size();
            out.pts.push_back((int32_t)sch.node_at(i));
        }
    }
}

// after positions [next, end) are linked: the tallest of them above the top level becomes the entry point
inline void raise_top(const BatchSchedule& sch, const std::vector<int32_t>& levels, size_t next, size_t end, int& maxlevel,
                      int& enterpoint) {
    for (size_t i = next; i < end; ++i)
        if (levels[sch.node_at(i)] > maxlevel) {
            maxlevel = levels[sch.node_at(i)];
            enterpoint = (int)sch.node_at(i);
        }
}

}  // namespace gfxknn
