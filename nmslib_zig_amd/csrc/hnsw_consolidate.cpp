// nmslib_gpu_consolidate: the deleted rows leave the index.  A resident HNSW graph is repaired around
// them and compacted on the device (kernels/hnsw_consolidate_kernels.hip); the host rows, ids and the graph's levels and
// offsets follow at once, the host copies of the lists when the file writer asks (sync_host_graph).  An index without a
// resident graph, and the exact scan, only compact their host side and are built / prepared again at the next use.  The
// positions, offsets and the entry point come from hnsw_consolidate_plan.hpp.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "engine.hpp"
#include "hnsw_consolidate_plan.hpp"

namespace gfxknn {

using clk = std::chrono::steady_clock;

static const char* const kConsolidateServed =
    "consolidating is served for hnsw, brute_force and seq_search over the dense spaces (float rows and l2sqr_sift) on one "
    "device, for graphs built in this process with delaunay_type 0-2, M and maxM <= 127 and maxM0 <= 254";

void Engine::consolidate(size_t* removed, size_t* repaired) {
    if (removed) *removed = 0;
    if (repaired) *repaired = 0;
    if (sparse_ || str_space_ || diverg_)
        throw EngineError(Err::SpaceIncompatible, std::string(sparse_ ? "a sparse" : str_space_ ? "a string" : "a divergence") +
                                                      " index is not consolidated: " + kConsolidateServed);
    if (gpu_shards_ > 1)
        throw EngineError(Err::SpaceIncompatible, "an index with gpu_shards=" + std::to_string(gpu_shards_) +
                                                      " is not consolidated: " + kConsolidateServed);
    if (method_ == Method::Hnsw && loaded_graph_)
        throw EngineError(Err::SpaceIncompatible, std::string("a graph loaded from a file is not consolidated: ") +
                                                      kConsolidateServed);
    if (method_ == Method::Hnsw && created_) {
        if (bp_.delaunay == 3)
            throw EngineError(Err::SpaceIncompatible, std::string("a graph of delaunay_type=3 is not consolidated: ") +
                                                          kConsolidateServed);
        if (bp_.M > 127 || bp_.maxM > 127 || bp_.maxM0 > 254 || graph_.maxM > 127 || graph_.maxM0 > 254)
            throw EngineError(Err::SpaceIncompatible, std::string("lists wider than the GPU builder's are not consolidated: ") +
                                                          kConsolidateServed);
    }
    if (n_dead_ == 0) return;
    ++pos_epoch_;  // positions move: filters made before name other rows now (filter.cpp)
    const size_t n = ids_.size(), dead = n_dead_;
    size_t fixed = 0;
    if (dead == n) {
        drop_all_rows();
    } else {
        // a graph is resident once the index has been finalized on a device; rows added since go into it first, as a
        // query would have it
        const bool resident = created_ && method_ == Method::Hnsw && device_ >= 0 && d_n_ > 0 && shards_.empty();
        if (resident && dirty_) finalize();
        std::vector<int32_t> newpos;
        const size_t live = consolidate_positions(tomb_, ids_.size(), newpos);
        if (resident && !dirty_ && (size_t)graph_.n == ids_.size() && d_n_ == ids_.size()) {
            consolidate_resident(newpos, live, fixed);
        } else {
            if (device_ >= 0 && have_last_) {   // batches in flight read what the next finalize replaces: it orders itself
                check_device();
                order_after_last(stream_);
                hip_check(hipStreamSynchronize(stream_), "consolidate");
            }
            d_tomb_.release();  // (no marks are left; nothing in flight reads it any more)
            compact_host_rows(newpos, live);
            dirty_ = true;
            graph_dirty_ = true;
            built_n_ = 0;
            host_links_stale_ = false;
            save_resident_rows_ = false;
        }
    }
    if (removed) *removed = dead;
    if (repaired) *repaired = fixed;
}

// rows and ids of the live rows close up; the marks go
void Engine::compact_host_rows(const std::vector<int32_t>& newpos, size_t live) {
    const size_t n = ids_.size(), rb = row_bytes();
    char* rows = is_u8() ? reinterpret_cast<char*>(rows_u8_.data()) : reinterpret_cast<char*>(rows_f32_.data());
    for (size_t i = 0; i < n; ++i) {
        if (newpos[i] < 0 || (size_t)newpos[i] == i) continue;
        std::memmove(rows + (size_t)newpos[i] * rb, rows + i * rb, rb);
        ids_[(size_t)newpos[i]] = ids_[i];
    }
    ids_.resize(live);
    if (is_u8()) rows_u8_.resize(live * 128);
    else rows_f32_.resize(live * dim_);
    tomb_.clear();
    n_dead_ = 0;
}

// every row is marked: rows, marks and graph go as with reset(); the index and query parameters stay
void Engine::drop_all_rows() {
    if (device_ >= 0) {
        check_device();
        order_after_last(stream_);
        hip_check(hipStreamSynchronize(stream_), "consolidate");
    }
    ids_.clear();
    rows_f32_.clear();
    rows_u8_.clear();
    tomb_.clear();
    n_dead_ = 0;
    graph_ = HostGraph();
    graph_rows_.clear();
    for (DevBuf* b : {&d_tomb_, &d_rows_, &d_ids_, &d_links0_, &d_up_off_, &d_up_links_, &d_rownorm_, &d_rows16_}) b->release();
    brute_ = BruteDense();
    dg_ = HnswDeviceGraph{};
    d_n_ = 0;
    built_n_ = 0;
    graph_up_ints_ = 0;
    host_links_stale_ = false;
    save_resident_rows_ = false;
    rows16_failed_ = false;
    hnsw_fix_valid_ = false;
    have_counters_ = false;
    fast_flags_ = nullptr;
    fast_nqt_ = 0;
    shards_.clear();
    dirty_ = true;
    graph_dirty_ = true;
}

// The resident graph of all ids_.size() rows (d_tomb_ holds their marks): worklist, repair, compaction.  Returns when the
// device work is done; the host state describes the compacted index then.
void Engine::consolidate_resident(const std::vector<int32_t>& newpos, size_t live, size_t& repaired) {
    check_device();
    hipStream_t s = stream_;
    order_after_last(s);
    HostGraph& g = graph_;
    const size_t n = ids_.size();
    const size_t l0_stride = (size_t)g.maxM0 + 1;

    // NMSLIB_GPU_CONSOLIDATE_TRACE (tools/hnsw_consolidate_time.py): the three parts are waited for one by one and their
    // seconds, the lists repaired and the repair's distance evaluations go to stderr
    const bool trace = getenv("NMSLIB_GPU_CONSOLIDATE_TRACE") != nullptr;
    const auto t0 = clk::now();

    // ---- repair, in place ----
    size_t nlists = n;
    for (size_t i = 0; i < n; ++i) nlists += (size_t)std::max(g.levels[i], 0);
    DevBuf d_levels, d_work, d_nwork;
    d_levels.ensure(n * 4);
    d_work.ensure(nlists * 8);
    d_nwork.ensure(64);
    hip_check(hipMemcpyAsync(d_levels.ptr(), g.levels.data(), n * 4, hipMemcpyHostToDevice, s), "levels");
    hip_check(hipMemsetAsync(d_nwork.ptr(), 0, 4, s), "clear worklist length");
    HnswConsolidate c{};
    c.g = dg_;
    c.g.ext_ids = nullptr;
    c.g.rows16 = nullptr;  // distances are the graph's own: the f32 (u8) rows
    c.links0 = d_links0_.as<int32_t>();
    c.up_links = d_up_links_.as<int32_t>();
    c.tomb = d_tomb_.as<uint32_t>();
    c.levels = d_levels.as<int32_t>();
    c.delaunay = bp_.delaunay;
    c.P = std::min(std::max(bp_.efConstruction, g.maxM0), 1024);  // (the graph's maxM0: post=1 widened it to the longest list)
    DevBuf d_ndist;
    if (trace) {
        d_ndist.ensure(8);
        hip_check(hipMemsetAsync(d_ndist.ptr(), 0, 8, s), "clear distance counter");
        c.ndist = d_ndist.as<unsigned long long>();
    }
    hip_check(launch_hnsw_cons_worklist(c, d_work.as<int32_t>(), (int)nlists, d_nwork.as<int32_t>(), s), "consolidate worklist");
    int32_t nwork = 0;
    hip_check(hipMemcpyAsync(&nwork, d_nwork.ptr(), 4, hipMemcpyDeviceToHost, s), "worklist length");
    hip_check(hipStreamSynchronize(s), "consolidate worklist");
    nwork = (int32_t)std::min<size_t>((size_t)std::max(nwork, 0), nlists);
    const auto t1 = clk::now();
    hip_check(launch_hnsw_cons_repair(c, d_work.as<int32_t>(), nwork, s), "consolidate repair");
    repaired = (size_t)nwork;
    unsigned long long ndist = 0;
    if (trace) {
        hip_check(hipMemcpyAsync(&ndist, d_ndist.ptr(), 8, hipMemcpyDeviceToHost, s), "distance counter");
        hip_check(hipStreamSynchronize(s), "consolidate repair");
    }
    const auto t2 = clk::now();

    // ---- the plan: levels, offsets, entry point ----
    std::vector<int32_t> new_levels, up_nodes;
    std::vector<int64_t> new_up_off;
    const size_t up_ints = consolidate_up_offsets(g.levels, newpos, g.maxM, new_levels, new_up_off, up_nodes);
    int enter = g.enterpoint, top = g.maxlevel;
    consolidate_entry(g.levels, newpos, enter, top);

    // ---- compaction into buffers sized for the live rows ----
    const bool have16 = dg_.rows16 != nullptr;
    const size_t rb = is_u8() ? 128 : (size_t)ldb_ * 4, rb16 = (size_t)dg_.ld16 * 2;
    DevBuf n_rows, n_ids, n_links0, n_up_off, n_up_links, n_norm, n_rows16;
    try {
        DevBuf d_newpos, d_up_nodes;
        d_newpos.ensure(n * 4);
        d_up_nodes.ensure(std::max<size_t>(up_nodes.size(), 1) * 4);
        n_rows.ensure(live * rb);
        n_ids.ensure(live * 4);
        n_links0.ensure(live * l0_stride * 4);
        n_up_off.ensure(live * 8);
        n_up_links.ensure(std::max<size_t>(up_ints, 1) * 4);
        if (is_u8()) n_norm.ensure(live * 4);
        if (have16) n_rows16.ensure(live * rb16);
        const uint32_t* tomb = d_tomb_.as<uint32_t>();
        const int32_t* np = d_newpos.as<int32_t>();
        hip_check(hipMemcpyAsync(d_newpos.ptr(), newpos.data(), n * 4, hipMemcpyHostToDevice, s), "new positions");
        hip_check(hipMemcpyAsync(n_up_off.ptr(), new_up_off.data(), live * 8, hipMemcpyHostToDevice, s), "up_off");
        if (!up_nodes.empty())
            hip_check(hipMemcpyAsync(d_up_nodes.ptr(), up_nodes.data(), up_nodes.size() * 4, hipMemcpyHostToDevice, s),
                      "upper nodes");
        hip_check(launch_hnsw_cons_scatter_rows(d_rows_.ptr(), n_rows.ptr(), rb, (int)n, tomb, np, s), "compact rows");
        hip_check(launch_hnsw_cons_scatter_rows(d_ids_.ptr(), n_ids.ptr(), 4, (int)n, tomb, np, s), "compact ids");
        if (is_u8())
            hip_check(launch_hnsw_cons_scatter_rows(d_rownorm_.ptr(), n_norm.ptr(), 4, (int)n, tomb, np, s), "compact norms");
        if (have16)
            hip_check(launch_hnsw_cons_scatter_rows(d_rows16_.ptr(), n_rows16.ptr(), rb16, (int)n, tomb, np, s),
                      "compact fp16 rows");
        hip_check(launch_hnsw_cons_links0(d_links0_.as<int32_t>(), n_links0.as<int32_t>(), (int)l0_stride, (int)n, tomb, np, s),
                  "compact links0");
        hip_check(hipMemsetAsync(n_up_links.ptr(), 0, std::max<size_t>(up_ints, 1) * 4, s), "clear up_links");
        hip_check(launch_hnsw_cons_up_links(d_up_links_.as<int32_t>(), d_up_off_.as<int64_t>(), d_levels.as<int32_t>(),
                                            n_up_links.as<int32_t>(), n_up_off.as<int64_t>(), d_up_nodes.as<int32_t>(),
                                            (int)up_nodes.size(), g.maxM, (int)n, np, s),
                  "compact up_links");
        hip_check(hipStreamSynchronize(s), "consolidate");  // (the temporaries above are freed here)
    } catch (const EngineError& x) {
        if (x.code != Err::OutOfMemory) throw;
        // old and new blocks did not fit side by side: make room and build in full over the compacted host rows
        (void)hipStreamSynchronize(s);
        for (DevBuf* b : {&n_rows, &n_ids, &n_links0, &n_up_off, &n_up_links, &n_norm, &n_rows16, &d_links0_, &d_up_off_,
                          &d_up_links_, &d_rows16_, &d_tomb_})
            b->release();
        compact_host_rows(newpos, live);
        dg_.rows16 = nullptr;
        dirty_ = graph_dirty_ = true;
        built_n_ = 0;
        host_links_stale_ = false;
        save_resident_rows_ = false;
        repaired = 0;  // (the repaired lists went with the buffers)
        finalize();
        return;
    }
    d_rows_.swap(n_rows);
    d_ids_.swap(n_ids);
    d_links0_.swap(n_links0);
    d_up_off_.swap(n_up_off);
    d_up_links_.swap(n_up_links);
    if (is_u8()) d_rownorm_.swap(n_norm);
    if (have16) d_rows16_.swap(n_rows16);
    d_tomb_.release();
    if (trace) {
        auto secs = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); };
        std::fprintf(stderr, "consolidate: worklist %.6f s, repair %.6f s, compaction %.6f s, %zu lists, %llu distances\n",
                     secs(t0, t1), secs(t1, t2), secs(t2, clk::now()), repaired, ndist);
    }

    // ---- the host side follows ----
    compact_host_rows(newpos, live);
    g.n = (int)live;
    g.levels.swap(new_levels);
    g.up_off.swap(new_up_off);
    g.maxlevel = top;
    g.enterpoint = enter >= 0 ? newpos[(size_t)enter] : 0;
    g.links0.clear();    // (behind the device's: fetched when the file writer asks)
    g.up_links.clear();
    graph_up_ints_ = up_ints;
    built_n_ = live;
    host_links_stale_ = true;
    save_resident_rows_ = true;
    d_n_ = live;
    dg_.rows = d_rows_.ptr();
    dg_.row_norm = d_rownorm_.as<int32_t>();
    dg_.ext_ids = d_ids_.as<int32_t>();
    dg_.n = (int)live;
    dg_.maxlevel = g.maxlevel;
    dg_.enterpoint = g.enterpoint;
    if (have16) dg_.rows16 = d_rows16_.ptr();
    bind_graph_buffers();
    hnsw_fix_valid_ = false;
    have_counters_ = false;
}

// The index file of a consolidated graph describes what is resident: lists (sync_host_graph) and, where the rows were prepared
// on the device (cosine on the optimized index: normalised by a kernel, whose sums round differently from the host's), the
// rows too -- the index loaded from the file then holds the bits the device holds.
bool Engine::fetch_resident_rows(std::vector<float>& rows) {
    if (!save_resident_rows_ || !dg_.normalize_query || is_u8() || d_n_ != ids_.size() || built_n_ != d_n_ || dirty_) return false;
    check_device();
    order_after_last(stream_);
    rows.resize(d_n_ * dim_);
    if (d_n_)
        hip_check(hipMemcpy2DAsync(rows.data(), dim_ * 4, d_rows_.ptr(), (size_t)ldb_ * 4, dim_ * 4, d_n_, hipMemcpyDeviceToHost,
                                   stream_),
                  "resident rows D2H");
    hip_check(hipStreamSynchronize(stream_), "resident rows D2H");
    return true;
}

}  // namespace gfxknn
