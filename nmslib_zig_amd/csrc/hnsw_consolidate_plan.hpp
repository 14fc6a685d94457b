// Host arithmetic of nmslib_gpu_consolidate (hnsw_consolidate.cpp): where the live rows go, where their
// upper-level lists start afterwards, and which node the search enters at.  Integer arithmetic on the tombstone bitset and
// the level array only -- no HIP, nothing of the engine -- so that tests/hnsw_consolidate_plan_check.cpp can check it
// without a GPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gfxknn {

// bit = position; positions beyond the last word are live
inline bool tomb_bit(const std::vector<uint32_t>& tomb, size_t pos) {
    return (pos >> 5) < tomb.size() && ((tomb[pos >> 5] >> (pos & 31)) & 1u);
}

// newpos[i] = rank of row i among the live rows of [0, n), -1 for a deleted row; returns the number of live rows
inline size_t consolidate_positions(const std::vector<uint32_t>& tomb, size_t n, std::vector<int32_t>& newpos) {
    newpos.assign(n, -1);
    size_t live = 0;
    for (size_t i = 0; i < n; ++i)
        if (!tomb_bit(tomb, i)) newpos[i] = (int32_t)live++;
    return live;
}

// The live nodes' levels and upper-level offsets at their new positions: the blocks keep their order and close up (a node
// of level L > 0 owns L * (maxM + 1) ints, a node of level 0 has offset -1).  up_nodes: the OLD positions of the live
// nodes with upper levels, ascending.  Returns the ints in use.
inline size_t consolidate_up_offsets(const std::vector<int32_t>& levels, const std::vector<int32_t>& newpos, int maxM,
                                     std::vector<int32_t>& new_levels, std::vector<int64_t>& new_up_off,
                                     std::vector<int32_t>& up_nodes) {
    new_levels.clear();
    new_up_off.clear();
    up_nodes.clear();
    size_t up_ints = 0;
    for (size_t i = 0; i < levels.size(); ++i) {
        if (newpos[i] < 0) continue;
        new_levels.push_back(levels[i]);
        if (levels[i] > 0) {
            new_up_off.push_back((int64_t)up_ints);
            up_ints += (size_t)levels[i] * (size_t)(maxM + 1);
            up_nodes.push_back((int32_t)i);
        } else {
            new_up_off.push_back(-1);
        }
    }
    return up_ints;
}

// Entry point and top level after the deleted nodes are gone, as OLD positions.  A live entry point stays.  A deleted
// one is replaced by the live node of the highest level, the smallest position among equals.  No live node: -1, level 0.
inline void consolidate_entry(const std::vector<int32_t>& levels, const std::vector<int32_t>& newpos, int& enterpoint,
                              int& maxlevel) {
    if (enterpoint >= 0 && (size_t)enterpoint < levels.size() && newpos[(size_t)enterpoint] >= 0) return;
    enterpoint = -1;
    maxlevel = 0;
    for (size_t i = 0; i < levels.size(); ++i)
        if (newpos[i] >= 0 && (enterpoint < 0 || levels[i] > maxlevel)) {
            enterpoint = (int)i;
            maxlevel = levels[i];
        }
}

}  // namespace gfxknn
