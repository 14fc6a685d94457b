// The dense HNSW search of one slice of a batch (knn_device cuts the batch and owns its HnswOut): which kernels answer it --
// the LDS kernels, the fp16 walk with its f32 re-rank, the HBM-array kernel, SearchOld -- and, for an index with deleted rows
// or a filtered batch, the two stages around them or, under gpu_inwalk=1, the search that filters
// inside the walk (4.6e).  The workspaces are HnswSearchWs; the resident side of the graph stays in engine.cpp.
#include <algorithm>
#include <climits>
#include <cstdlib>

#include "engine.hpp"
#include "filter_plan.hpp"
#include "hnsw_inwalk_plan.hpp"

namespace gfxknn {

// what the per-query workspaces of one launch may take together
constexpr size_t kHnswWsBudget = (size_t)4 << 30;

// body(q0, m) for every slice of nq queries whose workspaces, per_q bytes a query (0: none), stay within the budget.
// NMSLIB_HNSW_SLICE_MAXQ (tests; read at every call): at most that many queries per slice.
template <typename Body>
static void hnsw_for_slices(size_t nq, size_t per_q, Body body) {
    size_t slice = std::max<size_t>(1, std::min<size_t>(nq, per_q ? kHnswWsBudget / per_q : nq));
    const char* e = getenv("NMSLIB_HNSW_SLICE_MAXQ");
    const long maxq = e ? atol(e) : 0;
    if (maxq > 0) slice = std::min(slice, (size_t)maxq);
    for (size_t q0 = 0; q0 < nq; q0 += slice) body(q0, std::min(slice, nq - q0));
}

size_t Engine::hnsw_redone() {
    if (!shards_.empty()) return shards_[0]->hnsw_redone();
    if ((stats_path() != 4 && stats_path() != 5) || !hnsw_fix_valid_) return 0;
    if (hnsw_fix_valid_ == kRedoneOnHost) return hnsw_old_redone_;
    int32_t v = 0;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipStreamSynchronize(last_stream_ ? last_stream_ : stream_), "stats");
    hip_check(hipMemcpy(&v, sw_.fix.ptr(), 4, hipMemcpyDeviceToHost), "stats redo count");
    return (size_t)v;
}

// m visited bitsets of `words` words each in sw_.bitset, cleared on the stream
uint32_t* Engine::cleared_bitset(size_t m, size_t words, hipStream_t stream) {
    sw_.bitset.ensure(m * words * 4);
    hip_check(hipMemsetAsync(sw_.bitset.ptr(), 0, m * words * 4, stream), "clear visited bitset");
    return sw_.bitset.as<uint32_t>();
}

void Engine::knn_hnsw(const void* d_queries, size_t nq, size_t k, const HnswOut& out, hipStream_t stream) {
    if (n_dead_ > 0 && inwalk_serves(k)) knn_hnsw_inwalk(d_queries, nq, k, nullptr, 0, out, stream);
    else if (n_dead_ > 0) knn_hnsw_two_stage(d_queries, nq, k, nullptr, 0, out, stream);
    else hnsw_walk(false, d_queries, nq, k, out, stream);
}

// gpu_inwalk=1 and a batch the kernel serves; any other takes the two stages below
bool Engine::inwalk_serves(size_t k) const {
    return inwalk_ && inwalk_served((size_t)ef_, k, (size_t)hnsw_nbcap(dg_), hnsw_subset_query_bytes(dg_));
}

// Deleted rows and the walk route of a filtered batch with the tests inside the walk: one launch per slice on
// the f32 rows, whatever algoType and gpu_rows say.  The visited sets are HBM bitsets, so the batch is cut where they would
// outgrow the budget; all slices are one timed interval.
void Engine::knn_hnsw_inwalk(const void* d_queries, size_t nq, size_t k, const uint32_t* allow, size_t n_allow,
                             const HnswOut& out, hipStream_t stream, const FilterEach* each) {
    const uint32_t* tomb = n_dead_ > 0 ? d_tomb_.as<uint32_t>() : nullptr;
    const size_t words = (d_n_ + 31) / 32, qbytes = dim_ * elem_bytes();
    last_path = 8;
    have_counters_ = true;
    hnsw_fix_valid_ = false;
    hnsw_for_slices(nq, words * 4, [&](size_t q0, size_t m) {
        uint32_t* bitset = cleared_bitset(m, words, stream);
        if (q0 == 0) prof_begin(stream);
        const void* qs = static_cast<const char*>(d_queries) + q0 * qbytes;
        // (a slice's queries start at q0: so do their slots)
        hip_check(each ? launch_hnsw_inwalk_each(dg_, (int)m, (int)k, ef_, qs, bitset, words, {each->table, each->slot + q0}, tomb,
                                                 out.at(q0, k), stream)
                       : launch_hnsw_inwalk(dg_, (int)m, (int)k, ef_, qs, bitset, words, allow, (int)n_allow, tomb, out.at(q0, k),
                                            stream),
                  "hnsw_inwalk");
        if (q0 + m == nq) prof_end(stream);
    });
}

// Deleted rows and the walk route of a filtered batch (4.6d; allow: the filter's bits over n_allow positions).
// Stage 1: the search as it would run anyway, asked for cap = max(ef, k) results as positions, into a workspace.  Stage 2:
// hnsw_keep_topk_kernel writes the first k allowed live ones of them to the caller's buffers.  The counters are the walk's,
// at the slice's place in the batch's arrays; the timed interval ends behind the filter.
void Engine::knn_hnsw_two_stage(const void* d_queries, size_t nq, size_t k, const uint32_t* allow, size_t n_allow,
                                const HnswOut& out, hipStream_t stream, const FilterEach* each) {
    const size_t cap = filter_walk_results((size_t)ef_, k);
    const uint32_t* tomb = n_dead_ > 0 ? d_tomb_.as<uint32_t>() : nullptr;
    const size_t qbytes = dim_ * elem_bytes();
    // cap is unbounded on the SearchOld path: the slices of the batch are cut further where their results would not fit the
    // budget its own workspaces keep to
    hnsw_for_slices(nq, cap * 8, [&](size_t q0, size_t m) {
        sw_.live_ids.ensure(m * cap * 4);  // (the first slice is the largest)
        sw_.live_d.ensure(m * cap * 4);
        sw_.live_cnt.ensure(m * 4);
        const HnswOut fin = out.at(q0, k);
        HnswOut walk = fin;
        walk.ids = sw_.live_ids.as<int32_t>();
        walk.dists = sw_.live_d.as<float>();
        walk.cnt = sw_.live_cnt.as<int32_t>();
        hnsw_walk(true, static_cast<const char*>(d_queries) + q0 * qbytes, m, cap, walk, stream);
        hip_check(each ? launch_hnsw_keep_topk_each(walk.ids, walk.dists, walk.cnt, (int)m, (int)cap,
                                                    {each->table, each->slot + q0}, tomb, (int)d_n_, dg_.ext_ids, (int)k, fin, stream)
                       : launch_hnsw_keep_topk(walk.ids, walk.dists, walk.cnt, (int)m, (int)cap, allow, (int)n_allow, tomb,
                                               (int)d_n_, dg_.ext_ids, (int)k, fin, stream),
                  "hnsw_keep_topk");
        prof_end(stream);  // (the interval the walk opened: its end moves behind the filter)
    });
}

// positions: the launches get the graph without ext_ids, so that every kernel emits internal positions (the builder and the
// fp16 walk rely on the same)
void Engine::hnsw_walk(bool positions, const void* d_queries, size_t nq, size_t k, const HnswOut& out, hipStream_t stream) {
    const int ef = ef_;
    // every search kernel stages the query row in LDS; the HBM-array kernel keeps the least next to it.  Rows that leave
    // no workgroup room for that are refused by name (the launch functions refuse a plan beyond the limit too)
    if (hnsw_big_lds(dg_) > HNSW_LDS_LIMIT)
        throw EngineError(Err::QueryTooLarge, "HNSW search: rows of this dimension do not fit a workgroup's LDS");
    last_path = 4;
    hnsw_fix_valid_ = false;
    auto graph = [&] {  // (read where a path is taken: ensure_rows16 below names the fp16 copy in dg_)
        HnswDeviceGraph g = dg_;
        if (positions) g.ext_ids = nullptr;
        return g;
    };
    if (search_old()) {
        knn_hnsw_old(graph(), d_queries, nq, k, out, stream);
        return;
    }
    if (std::max<size_t>(ef, k) > 1024 || hnsw_nbcap(dg_) > HNSW_NBCAP_LDS) {
        const HnswDeviceGraph g = graph();
        // beyond the LDS kernels' sorted array, or adjacency lists longer than their frontier arrays (maxM0 or maxM > 255:
        // hnsw_nbcap sends a longest list of 255 to the 256-entry arrays): the same algorithm with the array in HBM and
        // lists walked in chunks (slices of bounded workspace)
        const size_t cap = std::max<size_t>(ef, k), words = (d_n_ + 31) / 32;
        const size_t qbytes = dim_ * elem_bytes();
        have_counters_ = true;
        hnsw_for_slices(nq, cap * 8 + words * 4, [&](size_t q0, size_t m) {
            sw_.old_a.ensure(m * cap * 4);
            sw_.old_r.ensure(m * cap * 4);
            uint32_t* bitset = cleared_bitset(m, words, stream);
            if (q0 == 0) prof_begin(stream);
            hip_check(launch_hnsw_search_big(g, (int)m, (int)k, ef, static_cast<const char*>(d_queries) + q0 * qbytes,
                                             bitset, sw_.old_a.as<float>(), sw_.old_r.as<int32_t>(), out.at(q0, k), stream),
                      "hnsw_search(big)");
            if (q0 + m == nq) prof_end(stream);
        });
        return;
    }
    // (SearchOld and the HBM-array kernel above stay on the f32 rows whatever gpu_rows says)
    if (rows_f16_ && ensure_rows16()) {
        knn_hnsw_f16(graph(), d_queries, nq, k, out, stream);
        return;
    }
    hnsw_search_lds(graph(), false, d_queries, nq, k, ef, out, true, stream);
}

void Engine::hnsw_search_lds(const HnswDeviceGraph& g, bool rows_f16, const void* d_queries, size_t nq, size_t k, int ef,
                             const HnswOut& out, bool timed, hipStream_t stream) {
    const HnswQueries queries = HnswQueries::external(d_queries);
    HnswSearchPlan p = hnsw_make_plan(g, (int)nq, (int)k, ef, false);
    p.rows_f16 = rows_f16 ? 1 : 0;
    // (rows the HBM-array kernel still stages can leave no room for this family's sorted array)
    if (p.lds_bytes > HNSW_LDS_LIMIT)
        throw EngineError(Err::QueryTooLarge, "HNSW search: rows of this dimension leave a workgroup's LDS no room for the "
                                              "sorted array; ef and k above 1024 take the kernel that keeps it in HBM");
    have_counters_ = true;
    if (p.table_size == 0) {
        uint32_t* bitset = cleared_bitset(nq, p.bitset_words, stream);
        prof_begin(stream);
        hip_check(launch_hnsw_search(g, p, queries, bitset, HnswOverflow{}, out, stream), "hnsw_search");
        if (timed) prof_end(stream);
        return;
    }
    // The LDS visited table is exact but finite.  Queries that fill it append themselves to a list on the device and
    // are re-run by a second, small launch of the bitset variant that walks that list -- the host never looks at it,
    // so the call only enqueues work (include/nmslib_gpu.h).
    const int fix_slots = (int)std::min<size_t>(nq, 128);
    HnswSearchPlan pb = hnsw_make_plan(g, (int)nq, (int)k, ef, true);
    pb.rows_f16 = p.rows_f16;
    sw_.fix.ensure((nq + 16) * 4);
    // (not cleared_bitset: the workgroups that walk the list clear their own slot on the device)
    sw_.bitset.ensure((size_t)fix_slots * pb.bitset_words * 4);
    int32_t* fix_count = sw_.fix.as<int32_t>();
    int32_t* fix_list = fix_count + 16;
    hip_check(hipMemsetAsync(fix_count, 0, 4, stream), "clear overflow count");
    hnsw_fix_valid_ = true;
    prof_begin(stream);
    hip_check(launch_hnsw_search(g, p, queries, nullptr, HnswOverflow{0, fix_list, fix_count}, out, stream), "hnsw_search");
    if (timed) prof_end(stream);
    hip_check(launch_hnsw_search(g, pb, queries, sw_.bitset.as<uint32_t>(), HnswOverflow{fix_slots, fix_list, fix_count},
                                 out, stream),
              "hnsw_search(bitset)");
}

// The walk reads the fp16 copy; what it ends with is re-ranked against the f32 rows, so every distance returned is the f32
// distance.  The walk is the search launch asked for cap = max(ef, k) results: the fp16 kernels then write their whole sorted
// array, in array order and as internal positions.  ndc / hops / hops_up describe the walk; the timed interval is walk +
// overflow launch + re-rank.
void Engine::knn_hnsw_f16(const HnswDeviceGraph& g, const void* d_queries, size_t nq, size_t k, const HnswOut& fin,
                          hipStream_t stream) {
    const int ef = ef_;
    const size_t cap = std::max<size_t>(ef, k);
    last_path = 5;
    sw_.rr_ids.ensure(nq * cap * 4);
    sw_.rr_d.ensure(nq * cap * 4);
    sw_.rr_cnt.ensure(nq * 4);
    HnswOut walk = fin;
    walk.ids = sw_.rr_ids.as<int32_t>();
    walk.dists = sw_.rr_d.as<float>();
    walk.cnt = sw_.rr_cnt.as<int32_t>();
    hnsw_search_lds(g, true, d_queries, nq, cap, ef, walk, false, stream);
    const size_t rerank = rerank_ > 0 ? std::min(cap, std::max<size_t>(k, (size_t)rerank_)) : cap;
    hip_check(launch_hnsw_rerank(g, (int)nq, (int)k, (int)cap, (int)rerank, d_queries, walk.ids, walk.cnt, fin, stream),
              "hnsw_rerank");
    prof_end(stream);
}

// Hnsw::SearchOld (hnsw_distfunc_opt.cc:46-150) on the GPU: no limit on ef or k.  Queues that outgrow LDS live in
// per-query HBM workspaces, so very large batches go through in slices of bounded workspace.
void Engine::knn_hnsw_old(const HnswDeviceGraph& g, const void* d_queries, size_t nq, size_t k, const HnswOut& out,
                          hipStream_t stream) {
    const int ef = ef_;
    const size_t qbytes = dim_ * elem_bytes();
    bool force_bitset = false;
    int heap_cap = 0;
    std::vector<int32_t> status(nq);
    for (int attempt = 0; attempt < 3; ++attempt) {
        HnswSearchPlan p0 = hnsw_make_plan_old(g, 1, (int)k, ef, force_bitset, heap_cap);
        // (the heap's first 2048 entries, the closest queue up to ef 8192 and the result queue up to k 2048 live in LDS next to
        // the query row: long rows with large ef or k outgrow the workgroup; the slices' plans take the same LDS)
        if (p0.lds_bytes > HNSW_LDS_LIMIT)
            throw EngineError(Err::QueryTooLarge, "SearchOld: the query row and the queues of this ef and k do not fit a "
                                                  "workgroup's LDS");
        const size_t per_q = hnsw_old_ws_a(p0) + hnsw_old_ws_r(p0) + hnsw_old_ws_heap(p0) + p0.bitset_words * 4;
        hnsw_for_slices(nq, per_q, [&](size_t q0, size_t m) {
            HnswSearchPlan p = hnsw_make_plan_old(g, (int)m, (int)k, ef, force_bitset, heap_cap);
            uint32_t* bitset = p.table_size == 0 ? cleared_bitset(m, p.bitset_words, stream) : nullptr;
            sw_.old_a.ensure(std::max<size_t>(16, m * hnsw_old_ws_a(p)));
            sw_.old_r.ensure(std::max<size_t>(16, m * hnsw_old_ws_r(p)));
            sw_.old_heap.ensure(std::max<size_t>(16, m * hnsw_old_ws_heap(p)));
            if (q0 == 0) prof_begin(stream);  // all slices of one attempt are one timed interval
            hip_check(launch_hnsw_search_old(g, p, static_cast<const char*>(d_queries) + q0 * qbytes, bitset,
                                             sw_.old_a.ptr(), sw_.old_r.ptr(), sw_.old_heap.ptr(), out.at(q0, k), stream),
                      "hnsw_search_old");
            if (q0 + m == nq) prof_end(stream);
        });
        have_counters_ = true;
        // status 1: the LDS visited table filled up -> HBM bitsets; status 2: the candidate heap outgrew its bound
        hip_check(hipMemcpyAsync(status.data(), out.status, nq * 4, hipMemcpyDeviceToHost, stream), "status");
        hip_check(hipStreamSynchronize(stream), "hnsw_search_old");
        bool any2 = false;
        size_t n1 = 0;
        for (int32_t v : status) {
            n1 += v == 1;
            any2 |= v == 2;
        }
        const bool any1 = n1 > 0;
        if (any1) {  // statistics: the queries whose table filled up (the whole batch runs again with bitsets)
            hnsw_old_redone_ = n1;
            hnsw_fix_valid_ = kRedoneOnHost;
        }
        if (!any1 && !any2) return;
        if (any1) force_bitset = true;
        if (any2) heap_cap = (int)std::min<size_t>(d_n_ + 1, (size_t)INT32_MAX);
    }
    throw EngineError(Err::QueryExecutionFailed, "SearchOld: queue workspaces exhausted");
}

}  // namespace gfxknn
