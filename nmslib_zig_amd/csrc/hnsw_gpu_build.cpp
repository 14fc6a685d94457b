// Batched HNSW construction on the GPU (kernels/hnsw_build_kernels.hip): the full build with its
// optional second pass, the insertion of rows added later into the resident graph, and the construction workspaces
// (HnswBuildWs).  Which positions make a batch and the batch's (node, level) pairs are decided by hnsw_batch_plan.hpp.
#include <algorithm>
#include <chrono>

#include "engine.hpp"
#include "f16_pack.hpp"
#include "hnsw_batch_plan.hpp"

namespace gfxknn {

using clk = std::chrono::steady_clock;
using u64 = unsigned long long;

void HnswBuildWs::reserve_batches(int max_batch, int M, size_t n) {
    // reverse-link requests of one level of one batch: M slots per new node, sorted on the device
    const size_t req_max = (size_t)max_batch * (size_t)M;
    for (DevBuf* b : {&req_key, &req_key2}) b->ensure(req_max * 8);
    for (DevBuf* b : {&req_dist, &req_dist2, &active}) b->ensure(req_max * 4);
    sort_tmp_bytes = hnsw_build_sort_temp_bytes((int)req_max, (int)n);
    sort_tmp.ensure(sort_tmp_bytes);
    nactive.ensure(64);
    for (DevBuf* b : {&extra_ids, &extra_d}) b->ensure((size_t)max_batch * 64 * 4);  // batch-mates: 64 per new node of a slice
    extra_n.ensure((size_t)max_batch * 4);
}

void HnswBuildWs::reserve_pairs(size_t npairs, int efC) {
    for (DevBuf* b : {&pts, &src, &starts, &cand_n, &status}) b->ensure(npairs * 4);
    for (DevBuf* b : {&cand_ids, &cand_d}) b->ensure(npairs * (size_t)efC * 4);
}

bool Engine::use_gpu_build() const {
    if (loaded_graph_ || method_ != Method::Hnsw) return false;
    // what only the host builder does (the reference's "no limits"): lists beyond four words per lane and selection
    // heuristic 3 (its candidate pool is an unordered set of node addresses) -- also when gpu_build=1 asks for the
    // GPU.  A new node's M links must fit its own lists (the select kernel writes them without a shrink step).
    if (bp_.M > 127 || bp_.maxM > 127 || bp_.maxM0 > 254 || bp_.M > bp_.maxM || bp_.M > bp_.maxM0 || bp_.delaunay == 3)
        return false;
    if (bp_.gpu_build >= 0) return bp_.gpu_build != 0;
    // auto: indexThreadQty=1 asks for the reference's sequential insertion order (bit-identical graph,
    // host builder); anything else is the concurrent build, whose schedule is free -> the GPU, unless the
    // parameters exceed what its kernels hold in LDS (the host builder has the reference's "no limits")
    if (bp_.efConstruction > 1024) return false;
    return bp_.threads != 1;
}

// graph_.links0 / up_links <- the device's lists
void Engine::download_graph_links() {
    HostGraph& g = graph_;
    if (g.n == 0) return;
    const size_t l0_ints = (size_t)g.n * (size_t)(g.maxM0 + 1);
    g.links0.resize(l0_ints);
    g.up_links.resize(graph_up_ints_);
    hipStream_t s = stream_;
    hip_check(hipMemcpyAsync(g.links0.data(), d_links0_.ptr(), l0_ints * 4, hipMemcpyDeviceToHost, s), "links0 D2H");
    if (graph_up_ints_)
        hip_check(hipMemcpyAsync(g.up_links.data(), d_up_links_.ptr(), graph_up_ints_ * 4, hipMemcpyDeviceToHost, s), "up_links D2H");
    hip_check(hipStreamSynchronize(s), "graph download");
}

// Insertion order, level stream and per-node algorithm are the reference's (Hnsw::add, hnsw.cc:534-609); what differs is
// visibility: the nodes of one batch are searched against the graph as it was before the batch, then linked (batches:
// hnsw_batch_plan.hpp).  All searches of a batch (every level, top down) precede all link updates.
// post = 1, 2 (hnsw.cc:251-330): a second pass inserts the rows in reverse order (node 0, then n-1 .. 1, levels drawn
// on from the same stream, as hnsw_build.cpp does); the result is the second graph with level-0 lists made from both
// (hnsw_build_post_kernel).
void Engine::build_graph_gpu() {
    auto t0 = clk::now();
    const size_t n = size();
    hnsw_check_params(bp_);
    const int maxM0 = bp_.maxM0, efC = bp_.efConstruction;
    if (efC < 1 || efC > 1024)
        throw EngineError(Err::IndexBuildFailed, "HNSW: efConstruction must be in [1, 1024] for the GPU builder");
    graph_builder_ = 2;
    built_n_ = 0;  // (set again below: a build that throws leaves no graph to append to)
    host_links_stale_ = false;
    save_resident_rows_ = false;
    const bool post = bp_.post != 0 && n > 1;
    const std::vector<int32_t> draws = hnsw_random_levels(post ? 2 * n : n, bp_);
    build_graph_gpu_pass(std::vector<int32_t>(draws.begin(), draws.begin() + (ptrdiff_t)n), false);
    HostGraph& g = graph_;
    hipStream_t s = stream_;
    if (post) {
        DevBuf first;
        first.swap(d_links0_);
        std::vector<int32_t> levels2(n);
        levels2[0] = draws[n];
        for (size_t pos = 1; pos < n; ++pos) levels2[n - pos] = draws[n + pos];
        build_graph_gpu_pass(levels2, true);
        // post = 1 keeps whole unions (up to 2 * maxM0) and then widens maxM0 to the longest list
        const int wide = (bp_.post == 1 ? 2 * maxM0 : maxM0) + 1;
        DevBuf out;
        out.ensure(n * (size_t)wide * 4);
        bw_.nactive.ensure(64);
        hip_check(hipMemsetAsync(out.ptr(), 0, n * (size_t)wide * 4, s), "clear post lists");
        hip_check(hipMemsetAsync(bw_.nactive.ptr(), 0, 4, s), "clear post length");
        HnswDeviceGraph pg = dg_;
        pg.ext_ids = nullptr;
        hip_check(launch_hnsw_build_post(pg, d_links0_.as<int32_t>(), first.as<int32_t>(), maxM0, bp_.post, bp_.delaunay,
                                         out.as<int32_t>(), wide, bw_.nactive.as<int32_t>(), s),
                  "build post");
        if (bp_.post == 1) {
            int32_t longest = 0;
            hip_check(hipMemcpyAsync(&longest, bw_.nactive.ptr(), 4, hipMemcpyDeviceToHost, s), "post length");
            hip_check(hipStreamSynchronize(s), "build post");
            g.maxM0 = std::max(longest, 1);
            d_links0_.release();
            d_links0_.ensure(n * (size_t)(g.maxM0 + 1) * 4);
            hip_check(launch_hnsw_build_repack(out.as<int32_t>(), wide, d_links0_.as<int32_t>(), g.maxM0 + 1, (int)n, s),
                      "build post repack");
            hip_check(hipStreamSynchronize(s), "build post repack");  // `out` is freed below
        } else {
            d_links0_.swap(out);
        }
        dg_.links0 = d_links0_.as<int32_t>();
        dg_.maxM0 = g.maxM0;
    }
    download_graph_links();
    bw_.release();
    built_n_ = n;
    build_seconds = n ? std::chrono::duration<double>(clk::now() - t0).count() : 0;
}

// One insertion pass over all rows (BatchSchedule has the order).  Leaves the graph in d_links0_ / d_up_off_ / d_up_links_ (dg_) and its levels, offsets and entry point in graph_.
// This part allocates and clears the graph with node 0 in it; build_graph_gpu_insert adds the other positions.
void Engine::build_graph_gpu_pass(const std::vector<int32_t>& levels, bool reverse) {
    const size_t n = size();
    const int maxM = bp_.maxM, maxM0 = bp_.maxM0;
    HostGraph& g = graph_;
    g = HostGraph{(int)n, bp_.M, maxM, maxM0, bp_.efConstruction, bp_.delaunay};
    g.levels = levels;
    size_t up_ints = 0;
    assign_up_offsets(g.levels, 0, n, maxM, up_ints, g.up_off);
    const size_t l0_ints = n * (size_t)(maxM0 + 1);
    d_links0_.ensure(std::max<size_t>(l0_ints, 1) * 4);
    d_up_off_.ensure(std::max<size_t>(n, 1) * 8);
    d_up_links_.ensure(std::max<size_t>(up_ints, 1) * 4);
    if (!reverse) prepare_graph_rows();  // (once: it normalises the cosine rows in place)
    bind_graph_buffers();
    dg_.maxM = maxM;
    dg_.maxM0 = maxM0;
    graph_up_ints_ = up_ints;
    if (n == 0) return;
    hipStream_t s = stream_;
    hip_check(hipMemsetAsync(d_links0_.ptr(), 0, l0_ints * 4, s), "clear links0");
    hip_check(hipMemsetAsync(d_up_links_.ptr(), 0, std::max<size_t>(up_ints, 1) * 4, s), "clear up_links");
    hip_check(hipMemcpyAsync(d_up_off_.ptr(), g.up_off.data(), n * 8, hipMemcpyHostToDevice, s), "up_off");
    g.maxlevel = dg_.maxlevel = g.levels[0];
    g.enterpoint = dg_.enterpoint = 0;
    build_graph_gpu_insert(1, reverse);
}

// Inserts positions [first, n) into the graph of positions [0, first) that dg_ / graph_ describe (lists on the device, cleared
// for the new nodes; levels, offsets, top level and entry point in graph_), batch by batch.  The schedule of a batch depends
// on the positions before it only, never on n (hnsw_batch_plan.hpp): inserting [first, n) into a finished graph of `first`
// nodes is what a pass over all n does from its batch boundary at `first` on (gpu_build_cut puts one there).
void Engine::build_graph_gpu_insert(size_t first, bool reverse) {
    HostGraph& g = graph_;
    hipStream_t s = stream_;
    HnswDeviceGraph bgraph = dg_;
    bgraph.ext_ids = nullptr;  // construction works on internal positions
    int &maxlevel = bgraph.maxlevel, &enterpoint = bgraph.enterpoint;  // the running state: what the next batch searches from
    const BatchSchedule sch{size(), reverse, bp_.gpu_build_div > 0 ? bp_.gpu_build_div : 16,
                            bp_.gpu_build_batch > 0 ? bp_.gpu_build_batch : 4096,
                            bp_.gpu_build_cut > 0 ? (size_t)bp_.gpu_build_cut : 0};
    bw_.reserve_batches(sch.max_batch, bp_.M, sch.n);
    BatchPairs pairs;
    for (size_t next = first, end; next < sch.n; next = end) {
        end = sch.batch_end(next, g.levels, maxlevel);
        plan_pairs(sch, g.levels, next, end, maxlevel, pairs);
        const size_t npairs = pairs.pts.size();
        bw_.reserve_pairs(npairs, bp_.efConstruction);
        for (DevBuf* b : {&ws_ndc_, &ws_hops_, &ws_hops_up_}) b->ensure(npairs * 4);
        hip_check(hipMemcpyAsync(bw_.pts.ptr(), pairs.pts.data(), npairs * 4, hipMemcpyHostToDevice, s), "batch nodes");
        hip_check(hipMemcpyAsync(bw_.src.ptr(), pairs.src.data(), npairs * 4, hipMemcpyHostToDevice, s), "batch sources");
        search_batch(bgraph, pairs);
        link_batch(bgraph, pairs, next);
        raise_top(sch, g.levels, next, end, maxlevel, enterpoint);
        // the pairs are reused by the next batch: the copies above must have been consumed
        hip_check(hipStreamSynchronize(s), "build batch");
    }
    g.maxlevel = dg_.maxlevel = maxlevel;
    g.enterpoint = dg_.enterpoint = enterpoint;
}

// efConstruction candidates for every pair of the batch, top level first: a pair starts where the same node's pair one
// level up ended.  A second attempt with HBM bitsets follows if an LDS visited table overflowed anywhere in the first.
void Engine::search_batch(const HnswDeviceGraph& bgraph, const BatchPairs& pairs) {
    const int efC = bp_.efConstruction;
    const size_t npairs = pairs.pts.size();
    hipStream_t s = stream_;
    int32_t *pts = bw_.pts.as<int32_t>(), *src = bw_.src.as<int32_t>(), *starts = bw_.starts.as<int32_t>();
    const HnswOut out{bw_.cand_ids.as<int32_t>(), bw_.cand_d.as<float>(), bw_.cand_n.as<int32_t>(), ws_ndc_.as<int32_t>(),
                      ws_hops_.as<int32_t>(), ws_hops_up_.as<int32_t>(), bw_.status.as<int32_t>()};
    std::vector<int32_t> status;
    for (int attempt = 0; attempt < 2; ++attempt) {
        bool used_table = false;
        for (int l = pairs.top; l >= 0; --l) {
            const size_t b0 = pairs.slice_begin(l), m = pairs.slice_size(l);
            if (m == 0) continue;
            hip_check(launch_hnsw_build_starts(src + b0, out.ids, out.cnt, efC, starts + b0, (int)m, s), "build starts");
            HnswSearchPlan p = hnsw_make_plan(bgraph, (int)m, efC, efC, /*force_bitset=*/attempt == 1);
            uint32_t* bitset = nullptr;
            if (p.table_size == 0) bitset = cleared_bitset(m, p.bitset_words, s);
            else used_table = true;
            hip_check(launch_hnsw_search(bgraph, p, HnswQueries::stored(pts + b0, starts + b0, l), bitset, HnswOverflow{},
                                         out.at(b0, efC), s),
                      "build search");
        }
        if (!used_table) break;
        status.resize(npairs);
        hip_check(hipMemcpyAsync(status.data(), bw_.status.ptr(), npairs * 4, hipMemcpyDeviceToHost, s), "status");
        hip_check(hipStreamSynchronize(s), "build search");
        // any flag set: the LDS visited table overflowed somewhere -> redo with HBM bitsets
        if (std::none_of(status.begin(), status.end(), [](int32_t v) { return v != 0; })) break;
    }
}

// Links the batch's nodes level by level from the candidates of search_batch; `linked`: the nodes in the graph before it.
void Engine::link_batch(const HnswDeviceGraph& bgraph, const BatchPairs& pairs, size_t linked) {
    const int M = bp_.M, efC = bp_.efConstruction;
    hipStream_t s = stream_;
    const HnswBuildGraph bg{bgraph, d_links0_.as<int32_t>(), d_up_links_.as<int32_t>(), M, bp_.delaunay};
    int32_t *x_ids = bw_.extra_ids.as<int32_t>(), *x_n = bw_.extra_n.as<int32_t>(), *active = bw_.active.as<int32_t>(),
            *nactive = bw_.nactive.as<int32_t>();
    float *x_d = bw_.extra_d.as<float>(), *rd = bw_.req_dist.as<float>(), *rd2 = bw_.req_dist2.as<float>();
    u64 *rk = bw_.req_key.as<u64>(), *rk2 = bw_.req_key2.as<u64>();
    for (int l = pairs.top; l >= 0; --l) {
        const size_t b0 = pairs.slice_begin(l), m = pairs.slice_size(l);
        if (m == 0) continue;
        const int total = (int)(m * (size_t)M);
        const int32_t *pts = bw_.pts.as<int32_t>() + b0, *cand_ids = bw_.cand_ids.as<int32_t>() + b0 * efC;
        float* cand_d = bw_.cand_d.as<float>() + b0 * efC;
        int32_t* cand_n = bw_.cand_n.as<int32_t>() + b0;
        hip_check(launch_hnsw_build_mates(bg, l, pts, (int)m, cand_d, cand_n, efC, x_ids, x_d, x_n, s), "build batch-mates");
        hip_check(launch_hnsw_build_select(bg, l, pts, (int)m, cand_ids, cand_d, cand_n, efC, x_ids, x_d, x_n, rk, rd, s),
                  "build select");
        hip_check(launch_hnsw_build_sort_requests(rk, rd, total, rk2, rd2, bw_.sort_tmp.ptr(), bw_.sort_tmp_bytes, active, nactive, s),
                  "build sort");
        // distinct targets: the nodes linked before the batch and the slice's own nodes (batch-mates select each
        // other); a smaller grid would drop whichever targets the head scan numbered last
        const size_t max_active = std::min<size_t>(linked + m, (size_t)total);
        hip_check(launch_hnsw_build_link(bg, l, active, nactive, (int)max_active, rk2, rd2, total, s), "build link");
    }
}

// gpu_append=1: the resident graph is the GPU builder's over rows [0, built_n_), complete and not post-processed, and all that
// happened since is add_row.  (finalize() has dealt with shards and checked use_gpu_build() before it asks.)
bool Engine::can_append() const {
    return bp_.gpu_append == 1 && graph_builder_ == 2 && built_n_ >= 1 && size() > built_n_ && d_n_ == built_n_ &&
           (size_t)graph_.n == built_n_ && bp_.post == 0 && !parent_ && shards_.empty() && !loaded_graph_;
}

// Rows [n0, n1) added after a GPU build go into the resident graph: the buffers grow to n1 rows keeping
// their contents, only the new rows are uploaded and prepared, the new rows take the level stream's draws [n0, n1), and the
// builder's batch loop is entered at position n0.  On a graph that was never consolidated the result is the graph a build of
// all n1 rows makes with a batch boundary at n0 (gpu_build_cut).  false: a buffer could not grow or the insertion ran out of memory; the caller builds in full from
// the host rows.
bool Engine::append_rows_gpu() {
    const auto t0 = clk::now();
    const size_t n0 = built_n_, n1 = size(), added = n1 - n0;
    const size_t l0_row = (size_t)(bp_.maxM0 + 1) * 4, ld16 = f16pack::row_stride(dim_);
    HostGraph& g = graph_;
    hipStream_t s = stream_;
    built_n_ = 0;  // (set again at the end: an append that throws leaves no graph to append to)
    // one stream per index, read by position: the new rows take its draws [n0, n1).  Its first n0 draws are g.levels only
    // while the graph was never consolidated; afterwards n0 is the live count, so draws that rows in front took before
    // are taken again
    const std::vector<int32_t> levels = hnsw_random_levels(n1, bp_);
    size_t up_ints = graph_up_ints_;
    std::vector<int64_t> up_off;
    assign_up_offsets(levels, n0, n1, bp_.maxM, up_ints, up_off);
    const bool have16 = dg_.rows16 != nullptr;  // (upload_rows takes the copy out of dg_ until the new rows are in it)
    try {
        upload_rows(n0);
        prepare_graph_rows(n0);
        d_links0_.grow_keep(n1 * l0_row, n0 * l0_row, s);
        d_up_off_.grow_keep(n1 * 8, n0 * 8, s);
        d_up_links_.grow_keep(std::max<size_t>(up_ints, 1) * 4, graph_up_ints_ * 4, s);
        if (have16) d_rows16_.grow_keep(n1 * ld16 * 2, n0 * ld16 * 2, s);
        bind_graph_buffers();
        // the graph's host side and the new nodes' empty lists
        g.n = (int)n1;
        g.levels.insert(g.levels.end(), levels.begin() + (ptrdiff_t)n0, levels.end());
        g.up_off.insert(g.up_off.end(), up_off.begin(), up_off.end());
        hip_check(hipMemsetAsync(d_links0_.as<char>() + n0 * l0_row, 0, added * l0_row, s), "clear links0");
        if (up_ints > graph_up_ints_)
            hip_check(hipMemsetAsync(d_up_links_.as<int32_t>() + graph_up_ints_, 0, (up_ints - graph_up_ints_) * 4, s),
                      "clear up_links");
        hip_check(hipMemcpyAsync(d_up_off_.as<int64_t>() + n0, up_off.data(), added * 8, hipMemcpyHostToDevice, s), "up_off");
        graph_up_ints_ = up_ints;
        host_links_stale_ = true;
        hnsw_fix_valid_ = false;
        build_graph_gpu_insert(n0, false);
    } catch (const EngineError& x) {
        if (x.code != Err::OutOfMemory) throw;
        // a buffer could not grow, or the insertion's workspaces did not fit beside the grown index: make room, build in full
        (void)hipStreamSynchronize(s);
        bw_.release();
        for (DevBuf* b : {&d_links0_, &d_up_off_, &d_up_links_, &d_rows16_}) b->release();
        host_links_stale_ = false;
        return false;
    }
    bw_.release();
    // the fp16 copy: the new rows at the copy's scale; all rows again (on the device) if the new ones move the scale
    if (have16) {
        rows16_max_ = std::max(rows16_max_, rows_max_abs(n0, n1));
        const int e = f16pack::scale_exp(rows16_max_);
        pack_rows16(e == rows16_exp_ ? n0 : 0, n1, e);
        rows16_exp_ = e;
        dg_.rows16 = d_rows16_.ptr();
        dg_.inv_scale16 = f16pack::scale_of(-e);
    } else if (rows_f16_index_) {
        (void)ensure_rows16();
    }
    built_n_ = n1;
    rows_appended = added;
    build_seconds = std::chrono::duration<double>(clk::now() - t0).count() - upload_seconds;
    return true;
}

// After an append the adjacency lists of graph_ are behind the device's (old nodes got new links too), after a consolidate
// (hnsw_consolidate.cpp; a host-built graph too) the host has none at all; the file writer reads them, so they are fetched
// when it asks.
void Engine::sync_host_graph() {
    if (!host_links_stale_) return;
    host_links_stale_ = false;
    if (built_n_ != (size_t)graph_.n) return;  // (graph_ is no longer the graph on the device)
    check_device();
    download_graph_links();
}

}  // namespace gfxknn
