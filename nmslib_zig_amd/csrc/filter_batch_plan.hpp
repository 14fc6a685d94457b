// Host arithmetic of a batch in which every query names its own filter (filter.cpp): the order the batch is
// run in and where its parts begin.  Integer arithmetic only -- no HIP, nothing of the engine -- so that
// tests/filter_batch_plan_check.cpp can check it without a GPU.
//
// Plan order: the unfiltered queries (-1) first, then the queries of the walk-route filters, then those of the subset-route
// filters; by filter index within each of the two, and in the caller's order within a filter (the permutation is stable).
// The queries of one route are then one contiguous segment, which costs one launch chain whatever the number of filters in
// it, and the queries of one filter are one contiguous group inside it.  The exact scan has one route ("child": every filter
// is segment kSegWalk) and runs one call per group.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace gfxknn {

enum : int { kSegUnfiltered = 0, kSegWalk = 1, kSegSubset = 2, kSegCount = 3 };

// the queries of one filter: plan positions [begin, end), never empty
struct FilterBatchGroup {
    int32_t filter;
    size_t begin, end;
};

struct FilterBatchPlan {
    std::vector<int32_t> perm;             // perm[p] = the caller's index of the query at plan position p
    std::vector<int32_t> inv;              // inv[q] = the plan position of the caller's query q
    size_t seg[kSegCount + 1] = {0, 0, 0, 0};  // segment s = plan positions [seg[s], seg[s + 1])
    std::vector<FilterBatchGroup> groups;  // the filters that have queries, in plan order (the unfiltered segment is no group)
    bool identity = true;                  // the batch is in plan order already: perm[p] == p
};

// the first query whose entry is outside [-1, n_filters), or nq when there is none
inline size_t filter_batch_first_bad(const int32_t* filter_of_query, size_t nq, size_t n_filters) {
    for (size_t q = 0; q < nq; ++q) {
        const int32_t v = filter_of_query[q];
        if (v < -1 || (v >= 0 && (size_t)v >= n_filters)) return q;
    }
    return nq;
}

// filter_of_query [nq]: entries in [-1, n_filters) (filter_batch_first_bad); segment_of_filter [n_filters]: kSegWalk or
// kSegSubset.  A counting sort on the key (segment, filter): one pass to count, one over the filters, one to place.
inline FilterBatchPlan filter_batch_plan(const int32_t* filter_of_query, size_t nq, const int* segment_of_filter,
                                         size_t n_filters) {
    FilterBatchPlan p;
    std::vector<size_t> at(n_filters + 1, 0);  // [0]: the unfiltered queries; [f + 1]: filter f -- counts, then places
    for (size_t q = 0; q < nq; ++q) at[(size_t)(filter_of_query[q] + 1)]++;
    size_t pos = at[0];
    at[0] = 0;
    p.seg[kSegUnfiltered] = 0;
    p.seg[kSegWalk] = pos;
    for (int s = kSegWalk; s <= kSegSubset; ++s) {
        for (size_t f = 0; f < n_filters; ++f) {
            if (segment_of_filter[f] != s) continue;
            const size_t c = at[f + 1];
            if (c > 0) p.groups.push_back({(int32_t)f, pos, pos + c});
            at[f + 1] = pos;
            pos += c;
        }
        p.seg[s + 1] = pos;
    }
    p.perm.resize(nq);
    p.inv.resize(nq);
    for (size_t q = 0; q < nq; ++q) {
        const size_t to = at[(size_t)(filter_of_query[q] + 1)]++;
        p.perm[to] = (int32_t)q;
        p.inv[q] = (int32_t)to;
        p.identity = p.identity && to == q;
    }
    return p;
}

}  // namespace gfxknn
