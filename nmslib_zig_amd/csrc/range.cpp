// Dense range search: the selection behind every space's range entry (range_select), the single
// query on the exact scan, and the batched query, whose rows are read once per slice of queries instead of once per query.
// The workspaces are RangeWs and ws_rdist_ (shared with the big-k scan).
#include "engine.hpp"
#include "range_batch_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

namespace gfxknn {

static const char* const kRangeBatchOneDevice =
    "the device-resident batched range query is served on one device; a sharded index goes through "
    "nmslib_gpu_range_query_batch";

// Range search over all d_n_ rows (RangeQuery::CheckAndAddToResult, src/rangequery.cc:67-76).  launch(filter, report)
// enqueues the distances of every row: the rows with filter[position] <= r are reported in insertion order, the first
// `capacity` of them, each with report[position] (report = filter unless the space has two distances per row).  The
// workspaces are sized before anything is enqueued: an allocation behind a kernel in flight waits for it.
size_t Engine::range_select(bool two_dists, float r, size_t capacity, int32_t* ids, float* dists,
                            const RangeLaunch& launch) {
    const int n = (int)d_n_;
    const size_t cnt_elems = range_count_elems(n);
    ws_rdist_.ensure((two_dists ? 2 : 1) * d_n_ * 4);
    rw_.cnt.ensure(cnt_elems * 4);
    // no more than d_n_ rows can match: a caller's declared capacity beyond that asks HBM for nothing
    capacity = std::min<size_t>(capacity, d_n_);
    ws_ids_.ensure(capacity * 4);
    ws_dists_.ensure(capacity * 4);
    float* filter = ws_rdist_.as<float>();
    float* report = two_dists ? filter + d_n_ : filter;
    launch(filter, report);
    hip_check(launch_range_select(filter, report, n, r, d_ids_.as<int32_t>(), rw_.cnt.as<int>(), (int)capacity,
                                  ws_ids_.as<int32_t>(), ws_dists_.as<float>(), stream_),
              "range select");
    int total = 0;
    hip_check(hipMemcpyAsync(&total, rw_.cnt.as<int>() + (cnt_elems - 1), 4, hipMemcpyDeviceToHost, stream_),
              "range count");
    hip_check(hipStreamSynchronize(stream_), "range search");
    const size_t m = std::min<size_t>((size_t)total, capacity);
    if (m) {
        hip_check(hipMemcpyAsync(ids, ws_ids_.ptr(), m * 4, hipMemcpyDeviceToHost, stream_), "range ids");
        hip_check(hipMemcpyAsync(dists, ws_dists_.ptr(), m * 4, hipMemcpyDeviceToHost, stream_), "range dists");
        hip_check(hipStreamSynchronize(stream_), "range search");
    }
    return m;
}

size_t Engine::range_host(const void* query, size_t elem_count, double radius, size_t capacity, int32_t* ids,
                          float* dists) {
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (diverg_ && !ids_.empty()) check_diverg_query_length(elem_count, dim_);  // refused before any device work
    if (dirty_) finalize();
    check_device();
    const size_t n = d_n_;
    if (diverg_) {
        order_after_last(stream_);
        return range_diverg_host(static_cast<const float*>(query), elem_count, radius, capacity, ids, dists);
    }
    if (n == 0 || capacity == 0) return 0;
    if (elem_count != dim_) throw EngineError(Err::QueryExecutionFailed, "query dimension does not match the index");
    if (!shards_.empty()) {
        // insertion order = shard order; shards report global positions
        DeviceGuard guard(device_);   // (a shard that throws must not leave this thread on its device)
        size_t got = 0;
        for (auto& c : shards_) {
            if (got >= capacity) break;
            got += c->range_host(query, elem_count, radius, capacity - got, ids + got, dists + got);
        }
        for (size_t i = 0; i < got; ++i) ids[i] = ids_[(size_t)ids[i]];
        hip_check(hipSetDevice(device_), "hipSetDevice");
        return got;
    }
    const int ld = is_u8() ? 128 : ldb_;
    const int elem = is_u8() ? 1 : 4;
    ws_qpad_.ensure((size_t)ld * elem);
    ws_q_.ensure(elem_count * elem);
    order_after_last(stream_);
    return range_select(false, range_radius(radius), capacity, ids, dists, [&](float* d, float*) {
        hip_check(hipMemcpyAsync(ws_q_.ptr(), query, elem_count * elem, hipMemcpyHostToDevice, stream_), "query H2D");
        hip_check(launch_pad_rows(ws_q_.ptr(), 1, (int)dim_, ws_qpad_.ptr(), 1, ld, elem, stream_), "pad query");
        hip_check(launch_range_dist(space_, d_rows_.ptr(), ld, (int)n, ws_qpad_.ptr(), (int)dim_, d, stream_),
                  "range distances");
    });
}

// ---- batched range queries ----
void Engine::check_range_batch(size_t elem_count, bool device_entry) const {
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (method_ != Method::Brute)  // the single entry's refusal (Hnsw::Search(RangeQuery*) throws, hnsw.cc:710-715)
        throw EngineError(Err::SpaceIncompatible, "Range query not supported by method: Range search is not supported!");
    if (sparse_ || str_space_ || diverg_)
        throw EngineError(Err::SpaceIncompatible,
                          "the batched range query is served over the dense float spaces (l2, l1, linf, cosinesimil, "
                          "angulardist, negdotprod) and l2sqr_sift; sparse, string and divergence indexes answer one "
                          "query at a time through nmslib_range_query_fill");
    if (device_entry && (gpu_shards_ > 1 || !shards_.empty())) throw EngineError(Err::SpaceIncompatible, kRangeBatchOneDevice);
    if (size() > 0 && elem_count != dim_)
        throw EngineError(Err::InvalidArgument, "query length " + std::to_string(elem_count) +
                                                    " does not match the rows' length " + std::to_string(dim_));
}

// The radii cross as floats through staged upload `turn` (calls take the two in turn: the wait is for the copy of the call
// before the previous one, so back-to-back calls do not meet on the host) into rw_.radii[turn], sized by the caller
const float* Engine::stage_radii(const double* radii, size_t nq, int turn, hipStream_t stream) {
    float* hr = static_cast<float*>(rw_.staged[turn].begin(nq * 4, "range batch"));
    for (size_t q = 0; q < nq; ++q) hr[q] = range_radius(radii[q]);  // as range_host converts it
    order_after_last(stream);
    hip_check(hipMemcpyAsync(rw_.radii[turn].ptr(), hr, nq * 4, hipMemcpyHostToDevice, stream), "radii H2D");
    rw_.staged[turn].sent(stream);
    return hr;
}

// route 10: the batched kernels, slice by slice; w describes the whole batch, a slice starts q0 queries into it
static void range_batch_slices(const RangeBatchPlan& plan, const RangeBatchArgs& w, size_t nq, size_t qbytes, hipStream_t stream) {
    for (size_t s = 0; s < plan.slices; ++s) {
        const size_t q0 = s * plan.slice_queries;
        RangeBatchArgs a = w;
        a.queries = static_cast<const char*>(w.queries) + q0 * qbytes;
        a.nq = (int)range_batch_slice_size(plan, nq, s);
        a.radii = w.radii + q0;
        a.out_ids = w.out_ids ? w.out_ids + q0 * w.capacity : nullptr;
        a.out_dists = w.out_dists ? w.out_dists + q0 * w.capacity : nullptr;
        a.out_counts = w.out_counts ? w.out_counts + q0 : nullptr;
        a.out_totals = w.out_totals ? w.out_totals + q0 : nullptr;
        hip_check(launch_range_batch(a, stream), "range batch");
    }
}

// route 11: the single-query launches, once per query, into the batch's rows: the old code and the old bits.  dist, cnt:
// range_select's workspaces; h_radii: the staging block's copy
static void range_batch_singles(const RangeBatchArgs& w, size_t nq, size_t qbytes, const float* h_radii, float* dist, int* cnt,
                                hipStream_t stream) {
    int* total = cnt + (range_count_elems(w.n) - 1);
    const int cap = (int)std::min(w.capacity, (size_t)w.n);
    for (size_t q = 0; q < nq; ++q) {
        int32_t* oi = w.out_ids ? w.out_ids + q * w.capacity : nullptr;
        float* od = w.out_dists ? w.out_dists + q * w.capacity : nullptr;
        hip_check(launch_range_dist(w.space, w.rows, w.ld, w.n, static_cast<const char*>(w.queries) + q * qbytes, w.dim, dist,
                                    stream),
                  "range distances");
        hip_check(launch_range_select(dist, dist, w.n, h_radii[q], w.ext_ids, cnt, cap, oi, od, stream), "range select");
        hip_check(launch_range_batch_finish(total, w.capacity, oi, od, w.out_counts ? w.out_counts + q : nullptr,
                                            w.out_totals ? w.out_totals + q : nullptr, w.pad, stream),
                  "range batch");
    }
}

void Engine::range_batch_device(const void* d_queries, size_t nq, size_t elem_count, const double* radii, size_t capacity,
                                int32_t* d_ids, float* d_dists, int32_t* d_counts, int32_t* d_totals, hipStream_t stream,
                                bool pad) {
    check_range_batch(elem_count, true);
    if (nq == 0) return;
    if (dirty_) finalize();
    check_device();
    if (!shards_.empty()) throw EngineError(Err::SpaceIncompatible, kRangeBatchOneDevice);  // (automatic sharding shows only now)
    // NMSLIB_GPU_RANGE_WS_BYTES (read per call) lowers the bound of the mask workspace: more, smaller slices
    const char* env = getenv("NMSLIB_GPU_RANGE_WS_BYTES");
    const size_t budget = env && atoll(env) > 0 ? std::min(kRangeBatchWsBytes, (size_t)atoll(env)) : kRangeBatchWsBytes;
    const RangeBatchPlan plan = range_batch_plan(d_n_, dim_, elem_bytes(), nq, capacity, budget);
    // every workspace before the first launch: an allocation behind a kernel in flight waits for it
    const int turn = rw_.turn;
    rw_.turn ^= 1;
    rw_.radii[turn].ensure(nq * 4);
    if (plan.route == 10) {
        rw_.masks.ensure(std::max<size_t>(8, plan.slice_queries * plan.mask_words * 8));
        rw_.counts.ensure(plan.slice_queries * (plan.blocks + 1) * 4);
    } else {
        ws_rdist_.ensure(std::max<size_t>(4, d_n_ * 4));
        rw_.cnt.ensure(range_count_elems((int)d_n_) * 4);
    }
    const float* h_radii = stage_radii(radii, nq, turn, stream);
    // the whole batch, in the field order of RangeBatchArgs: the rows; the queries; the outputs; the workspaces and the grid
    const RangeBatchArgs w{space_, d_rows_.ptr(), is_u8() ? 128 : ldb_, (int)d_n_, (int)dim_,
                           d_queries, (int)nq, rw_.radii[turn].as<float>(), capacity,
                           capacity ? d_ids : nullptr, capacity ? d_dists : nullptr, d_counts, d_totals, d_ids_.as<int32_t>(),
                           rw_.masks.as<unsigned long long>(), plan.mask_words, rw_.counts.as<int>(), (unsigned)plan.grid_x,
                           (unsigned)plan.grid_y, pad};
    const size_t qbytes = elem_count * elem_bytes();
    if (plan.route == 10) range_batch_slices(plan, w, nq, qbytes, stream);
    else range_batch_singles(w, nq, qbytes, h_radii, ws_rdist_.as<float>(), rw_.cnt.as<int>(), stream);
    have_counters_ = false;
    last_path = plan.route;
}

// The shards' answers merged.  Insertion order = shard order: per query the shards' lists back to back up to the capacity,
// the totals summed; shards report global positions.  Nothing is written before every shard has answered.
void Engine::range_batch_merge_shards(const void* queries, size_t nq, size_t elem_count, const double* radii, size_t capacity,
                                      int32_t* ids, float* dists, int32_t* counts, int32_t* totals, std::vector<size_t>& got) {
    DeviceGuard guard(device_);
    const size_t S = shards_.size();
    std::vector<std::vector<int32_t>> sid(S), scnt(S), stot(S);
    std::vector<std::vector<float>> sd(S);
    std::vector<size_t> scap(S);
    for (size_t s = 0; s < S; ++s) {
        Engine& c = *shards_[s];
        scap[s] = std::min(capacity, c.size());
        sid[s].resize(nq * scap[s]);
        sd[s].resize(nq * scap[s]);
        scnt[s].resize(nq);
        stot[s].resize(nq);
        c.range_batch_host(queries, nq, elem_count, radii, scap[s], sid[s].data(), sd[s].data(), scnt[s].data(),
                           stot[s].data());
    }
    hip_check(hipSetDevice(device_), "hipSetDevice");
    last_path = shards_[0]->last_path;
    for (size_t q = 0; q < nq; ++q) {
        long long total = 0;
        for (size_t s = 0; s < S; ++s) {
            total += stot[s][q];
            const size_t m = std::min<size_t>((size_t)scnt[s][q], capacity - got[q]);
            for (size_t i = 0; i < m; ++i) ids[q * capacity + got[q] + i] = ids_[(size_t)sid[s][q * scap[s] + i]];
            std::copy_n(sd[s].data() + q * scap[s], m, dists + q * capacity + got[q]);
            got[q] += m;
        }
        if (counts) counts[q] = (int32_t)got[q];
        if (totals) totals[q] = (int32_t)total;
    }
}

// One device's answer fetched.  No more than d_n_ rows can match: the device side of a row ends there.  The device does not
// pad here: the counts come back first, then only the columns that hold an entry of some query (one strided copy per array);
// the caller pads once, in its own memory.
void Engine::range_batch_fetch(const void* queries, size_t nq, size_t elem_count, const double* radii, size_t capacity,
                               int32_t* ids, float* dists, int32_t* counts, int32_t* totals, std::vector<size_t>& got) {
    const size_t cap = std::min(capacity, d_n_);
    const size_t qbytes = nq * elem_count * elem_bytes();
    ws_q_.ensure(qbytes);
    rw_.res.ensure(2 * nq * cap * 4 + 2 * nq * 4);
    char* hp = static_cast<char*>(pinned(qbytes));
    std::memcpy(hp, queries, qbytes);
    order_after_last(stream_);
    hip_check(hipMemcpyAsync(ws_q_.ptr(), hp, qbytes, hipMemcpyHostToDevice, stream_), "queries H2D");
    int32_t* d_i = rw_.res.as<int32_t>();
    float* d_d = reinterpret_cast<float*>(d_i + nq * cap);
    int32_t* d_c = d_i + 2 * nq * cap;
    range_batch_device(ws_q_.ptr(), nq, elem_count, radii, cap, d_i, d_d, d_c, d_c + nq, stream_, false);
    std::vector<int32_t> h_c(2 * nq);
    hip_check(hipMemcpyAsync(h_c.data(), d_c, 2 * nq * 4, hipMemcpyDeviceToHost, stream_), "counts D2H");
    hip_check(hipStreamSynchronize(stream_), "range batch");
    size_t width = 0;
    for (size_t q = 0; q < nq; ++q) width = std::max(width, got[q] = (size_t)h_c[q]);
    if (width) {
        hp = static_cast<char*>(pinned(2 * nq * width * 4));   // (the queries have left the block)
        const int32_t* h_i = reinterpret_cast<const int32_t*>(hp);
        const float* h_d = reinterpret_cast<const float*>(hp + nq * width * 4);
        hip_check(hipMemcpy2DAsync(hp, width * 4, d_i, cap * 4, width * 4, nq, hipMemcpyDeviceToHost, stream_), "ids D2H");
        hip_check(hipMemcpy2DAsync(hp + nq * width * 4, width * 4, d_d, cap * 4, width * 4, nq, hipMemcpyDeviceToHost, stream_),
                  "dists D2H");
        hip_check(hipStreamSynchronize(stream_), "range batch");
        for (size_t q = 0; q < nq; ++q) {
            std::memcpy(ids + q * capacity, h_i + q * width, got[q] * 4);
            std::memcpy(dists + q * capacity, h_d + q * width, got[q] * 4);
        }
    }
    if (counts) std::copy(h_c.begin(), h_c.begin() + nq, counts);
    if (totals) std::copy(h_c.begin() + nq, h_c.end(), totals);
}

void Engine::range_batch_host(const void* queries, size_t nq, size_t elem_count, const double* radii, size_t capacity,
                              int32_t* ids, float* dists, int32_t* counts, int32_t* totals) {
    check_range_batch(elem_count, false);
    if (nq == 0) return;
    if (dirty_) finalize();
    check_device();
    std::vector<size_t> got(nq, 0);  // what a query gets: row q = got[q] entries, then the padding
    if (!shards_.empty()) range_batch_merge_shards(queries, nq, elem_count, radii, capacity, ids, dists, counts, totals, got);
    else range_batch_fetch(queries, nq, elem_count, radii, capacity, ids, dists, counts, totals, got);
    for (size_t q = 0; q < nq; ++q) {
        std::fill(ids + q * capacity + got[q], ids + (q + 1) * capacity, -1);
        std::fill(dists + q * capacity + got[q], dists + (q + 1) * capacity, INFINITY);
    }
}

}  // namespace gfxknn
