// Filtered k-NN (nmslib_gpu_filter_*): a filter names a subset of an index's positions by a bitset and is
// turned, on the device, into what the index kind needs.
//   exact scan: the index of the allowed live rows alone -- a child engine whose rows and ids are gathered in HBM and
//               prepared by prepare_brute, so that a filtered batch is knn_brute on it, every path included;
//   HNSW:       the walk for max(ef, k) results filtered through the bitset and the tombstones, or (filter_plan.hpp) an exact
//               scan of the listed rows when the subset is no larger than that result array.
// A batch in which every query names its own filter (knn_device_each) is put into plan order
// (filter_batch_plan.hpp) and run there: HNSW one launch chain per route segment, the exact scan one knn_brute per filter.
#include <algorithm>
#include <cstring>

#include "engine.hpp"
#include "filter_batch_plan.hpp"
#include "filter_plan.hpp"

namespace gfxknn {

static_assert(kFilterSubsetMax == (size_t)HNSW_SUBSET_MAX, "the routing rule and the kernel name one capacity");

static const char* const kFilterServed =
    "filtered search is served for hnsw, brute_force and seq_search over the dense spaces (l2, l1, linf, cosinesimil, "
    "angulardist, negdotprod, l2sqr_sift) on one device";

void Engine::check_filter_served() const {
    if (sparse_ || str_space_ || diverg_)
        throw EngineError(Err::SpaceIncompatible, std::string(sparse_ ? "a sparse" : str_space_ ? "a string" : "a divergence") +
                                                      " index takes no filter: " + kFilterServed);
    if (gpu_shards_ > 1)
        throw EngineError(Err::SpaceIncompatible, "an index with gpu_shards=" + std::to_string(gpu_shards_) +
                                                      " takes no filter: " + kFilterServed);
}

void Engine::check_filter(const Filter* f) const {
    if (!f || f->owner != this) throw EngineError(Err::InvalidArgument, "the filter belongs to another index");
    if (f->epoch != pos_epoch_)
        throw EngineError(Err::InvalidArgument, "the filter is stale: positions have moved since it was made (a consolidate "
                                                "that removed rows, or a reset); make a new one");
}

// The rows the filter takes among n_rows device rows (row r at position row_pos[r], or r), ascending, into `list` when there
// are at most list_max of them; count = how many.  Waits for the count.
void Engine::filter_compact(Filter& f, const uint32_t* tomb, const int32_t* row_pos, size_t n_rows, DevBuf& list,
                            size_t list_max, size_t& count) {
    const size_t words = (n_rows + 31) / 32;
    DevBuf mask, prefix, d_count;
    mask.ensure(std::max<size_t>(words, 1) * 4);
    prefix.ensure(std::max<size_t>(words, 1) * 4);
    d_count.ensure(16);
    hip_check(launch_filter_count(f.d_allow.as<uint32_t>(), (int)f.n, tomb, row_pos, (int)n_rows, mask.as<uint32_t>(),
                                  prefix.as<int32_t>(), d_count.as<int32_t>(), stream_),
              "filter count");
    int32_t c = 0;
    hip_check(hipMemcpyAsync(&c, d_count.ptr(), 4, hipMemcpyDeviceToHost, stream_), "filter count");
    hip_check(hipStreamSynchronize(stream_), "filter count");
    count = (size_t)std::max(c, 0);
    if (count == 0 || count > list_max) return;
    list.ensure(count * 4);
    hip_check(launch_filter_write(mask.as<uint32_t>(), prefix.as<int32_t>(), (int)n_rows, list.as<int32_t>(), stream_),
              "filter list");
    hip_check(hipStreamSynchronize(stream_), "filter list");  // (mask and prefix go out of scope)
}

Filter* Engine::filter_create(const uint32_t* bits, size_t words, size_t scan_rows) {
    check_filter_served();
    const size_t n = size(), need = (n + 31) / 32;
    if (words < need)
        throw EngineError(Err::InvalidArgument, "allow_words = " + std::to_string(words) + " is fewer than the " +
                                                    std::to_string(need) + " words that " + std::to_string(n) + " rows take");
    if (scan_rows > kFilterSubsetMax)
        throw EngineError(Err::InvalidArgument, "scan_rows = " + std::to_string(scan_rows) + " is beyond the subset scan's " +
                                                    std::to_string(kFilterSubsetMax) + " rows");
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (dirty_) finalize();
    check_device();
    if (!shards_.empty())
        throw EngineError(Err::SpaceIncompatible, "an index spread over " + std::to_string(shards_.size()) +
                                                      " devices takes no filter: " + kFilterServed);
    std::unique_ptr<Filter> f(new Filter);
    f->owner = this;
    f->epoch = pos_epoch_;
    f->n = n;
    f->scan_rows = scan_rows;
    f->bits.assign(bits, bits + need);
    if (n & 31) f->bits[need - 1] &= (1u << (n & 31)) - 1u;  // bits at or beyond n are ignored
    f->d_allow.ensure(std::max<size_t>(need, 1) * 4);
    order_after_last(stream_);
    hip_check(hipMemcpyAsync(f->d_allow.ptr(), f->bits.data(), need * 4, hipMemcpyHostToDevice, stream_), "filter bits H2D");
    if (method_ == Method::Brute) {
        filter_gather(*f);
    } else {
        const uint32_t* tomb = n_dead_ > 0 ? d_tomb_.as<uint32_t>() : nullptr;
        filter_compact(*f, tomb, nullptr, d_n_, f->d_list, kFilterSubsetMax, f->m);
    }
    hip_check(hipStreamSynchronize(stream_), "filter");  // (the pageable source of the copy above)
    filters_.push_back(std::move(f));
    return filters_.back().get();
}

void Engine::filter_destroy(Filter* f) {
    for (auto it = filters_.begin(); it != filters_.end(); ++it)
        if (it->get() == f) {
            if (device_ >= 0 && have_last_) {  // a batch in flight may read what is freed here
                check_device();
                hip_check(hipStreamSynchronize(last_stream_), "filter destroy");
            }
            filter_forget_flags(*f);
            filters_.erase(it);
            return;
        }
}

void Engine::filter_info(const Filter* f, size_t* allowed_live_rows, size_t* hbm_bytes) const {
    if (!f || f->owner != this) throw EngineError(Err::InvalidArgument, "the filter belongs to another index");
    if (allowed_live_rows) {
        size_t live = 0;
        for (size_t w = 0; w < f->bits.size(); ++w)
            live += (size_t)__builtin_popcount(f->bits[w] & ~(w < tomb_.size() ? tomb_[w] : 0u));
        *allowed_live_rows = f->epoch == pos_epoch_ ? live : 0;
    }
    if (hbm_bytes) *hbm_bytes = f->d_allow.bytes() + f->d_list.bytes() + (f->sub ? f->sub->hbm_bytes() : 0);
}

// Exact scan: the allowed rows among the resident ones (all rows, or the live rows of an index with deleted rows, whose
// positions upload_rows kept) are listed, their rows and ids gathered in HBM, and the child prepared as finalize prepares an
// index: centring decision, aux, fast-path tiles, the l1 byte copy.  No row crosses PCIe.  Waits for the device.
void Engine::filter_gather(Filter& f) {
    order_after_last(stream_);
    DevBuf list;
    size_t m = 0;
    filter_compact(f, nullptr, d_livepos_.bytes() ? d_livepos_.as<int32_t>() : nullptr, d_n_, list, d_n_, m);
    if (!f.sub) {
        f.sub.reset(new Engine(space_name_, method_name_, is_u8() ? 2 : 0, 0));
        f.sub->method_ = method_;
        f.sub->created_ = true;
        f.sub->forced_device_ = device_;
        f.sub->check_device();
    }
    Engine& c = *f.sub;
    filter_forget_flags(f);  // (the child's workspaces are released below)
    c.fast_flags_ = nullptr;
    c.fast_nqt_ = 0;
    const size_t rb = is_u8() ? 128 : (size_t)ldb_ * 4;
    c.dim_ = dim_;
    c.ldb_ = ldb_;
    c.d_rows_.ensure(std::max<size_t>(m, 1) * rb);
    c.d_ids_.ensure(std::max<size_t>(m, 1) * 4);
    hip_check(launch_filter_gather_rows(d_rows_.ptr(), list.as<int32_t>(), (int)m, rb, c.d_rows_.ptr(), stream_), "filter rows");
    hip_check(launch_filter_gather_ids(d_ids_.as<int32_t>(), list.as<int32_t>(), (int)m, c.d_ids_.as<int32_t>(), stream_),
              "filter ids");
    hip_check(hipStreamSynchronize(stream_), "filter gather");  // (`list` goes out of scope; the child prepares on its own stream)
    c.d_n_ = m;
    c.dirty_ = false;
    c.brute_ = BruteDense();
    c.prepare_brute();
    f.m = m;
    f.gathered_at = prepared_;
}

// A filtered batch (knn_device with a filter), before anything is enqueued.  An index spread over several devices since the
// filter was made is refused as at create.  The exact scan's index has been prepared again since the gather (an add, a
// delete): this batch gathers again and waits.
void Engine::filter_begin_batch(Filter& f) {
    if (!shards_.empty())
        throw EngineError(Err::SpaceIncompatible, "an index spread over " + std::to_string(shards_.size()) +
                                                      " devices takes no filter: " + kFilterServed);
    if (method_ == Method::Brute && f.gathered_at != prepared_) filter_gather(f);
}

// One slice of a filtered exact-scan batch (knn_device's slices): knn_brute on the filter's child; the batch is this index's,
// so its timed intervals, path and fast-path flags are read here.
void Engine::knn_filtered_slice(Filter& f, const void* d_queries, size_t nq, size_t k, int32_t* d_ids, float* d_dists,
                                int32_t* d_cnt, hipStream_t stream) {
    Engine& c = *f.sub;
    c.prof_ = prof_;
    c.knn_brute(d_queries, nq, k, d_ids, d_dists, d_cnt, stream);
    prof_events_.insert(prof_events_.end(), c.prof_events_.begin(), c.prof_events_.end());
    c.prof_events_.clear();
    have_counters_ = false;
    last_path = c.last_path;
    fast_flags_ = c.fast_flags_;   // (a workspace of the child: filter_forget_flags before it goes)
    fast_nqt_ = c.fast_nqt_;
    fast_has_precise_ = c.fast_has_precise_;
}

// The statistics of the last batch point into the child's workspace when that batch ran under f: they are dropped before the
// workspace is freed (the filter is destroyed, or its child prepared again), as reset() and the consolidate drop theirs.
void Engine::filter_forget_flags(const Filter& f) {
    if (!f.sub || !fast_flags_ || fast_flags_ != f.sub->fast_flags_) return;
    fast_flags_ = nullptr;
    fast_nqt_ = 0;
}

// One slice of a filtered HNSW batch.  Subset route: hnsw_subset_knn_kernel over the filter's list (last_path 7).  Walk route:
// the two stages of hnsw_search.cpp with the filter's bits, or under gpu_inwalk=1 its in-walk search (last_path 8); the counters
// are the walk's.
void Engine::knn_hnsw_filtered(Filter& f, const void* d_queries, size_t nq, size_t k, const HnswOut& out, hipStream_t stream) {
    if (filter_route(f.m, (size_t)ef_, k, f.scan_rows, hnsw_subset_query_bytes(dg_)) == FilterRoute::Subset) {
        const uint32_t* tomb = n_dead_ > 0 ? d_tomb_.as<uint32_t>() : nullptr;
        HnswDeviceGraph g = dg_;
        g.rows16 = nullptr;  // always the f32 rows: the bits of the f32 walk
        have_counters_ = true;
        hnsw_fix_valid_ = false;
        last_path = 7;
        prof_begin(stream);
        hip_check(launch_hnsw_subset_knn(g, (int)nq, (int)k, d_queries, f.d_list.as<int32_t>(), (int)f.m, tomb, out, stream),
                  "hnsw_subset_knn");
        prof_end(stream);
        return;
    }
    if (inwalk_serves(k)) knn_hnsw_inwalk(d_queries, nq, k, f.d_allow.as<uint32_t>(), f.n, out, stream);
    else knn_hnsw_two_stage(d_queries, nq, k, f.d_allow.as<uint32_t>(), f.n, out, stream);
}

// ---- one filter per query (nmslib_gpu_knn_query_batch_filtered_each) ----------------------------------------

static const char* const kEachSharded = " devices takes no filter: ";

void Engine::check_filters_each(Filter* const* filters, size_t n_filters, const int32_t* filter_of_query, size_t nq) const {
    check_filter_served();
    const size_t bad = filter_batch_first_bad(filter_of_query, nq, n_filters);
    if (bad < nq)
        throw EngineError(Err::InvalidArgument, "filter_of_query[" + std::to_string(bad) + "] = " +
                                                    std::to_string(filter_of_query[bad]) + " is outside [-1, " +
                                                    std::to_string(n_filters) + ")");
    for (size_t j = 0; j < n_filters; ++j) {
        try {
            check_filter(filters[j]);
        } catch (const EngineError& x) {
            throw EngineError(x.code, "filters[" + std::to_string(j) + "]: " + x.what());
        }
    }
}

void Engine::gather_rows(const void* src, const int32_t* list, size_t m, size_t row_bytes, void* dst, hipStream_t stream) {
    const bool wide = row_bytes % 16 == 0 && (reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 16 == 0;
    hip_check(wide ? launch_filter_gather_rows(src, list, (int)m, row_bytes, dst, stream)
                   : launch_filter_gather_words(src, list, (int)m, row_bytes, dst, stream),
              "filter batch gather");
}

void Engine::knn_device_each(Filter* const* filters, size_t n_filters, const int32_t* filter_of_query, const void* d_queries,
                             size_t nq, size_t elem_count, size_t k, int32_t* d_ids, float* d_dists, int32_t* d_cnt,
                             hipStream_t stream, int32_t* routes) {
    check_filters_each(filters, n_filters, filter_of_query, nq);
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (nq == 0) return;
    if (k == 0) throw EngineError(Err::InvalidArgument, "k must be positive");
    if (nq > (size_t)INT32_MAX) throw EngineError(Err::QueryTooLarge, "a batch takes at most 2^31 - 1 queries");
    if (dirty_) finalize();
    check_device();
    const bool hnsw = method_ == Method::Hnsw;
    // the route of every filter, then the batch's order; both host arithmetic
    std::vector<int> segment(n_filters, kSegWalk);
    if (hnsw)
        for (size_t j = 0; j < n_filters; ++j)
            if (filter_route(filters[j]->m, (size_t)ef_, k, filters[j]->scan_rows, hnsw_subset_query_bytes(dg_)) ==
                FilterRoute::Subset)
                segment[j] = kSegSubset;
    const FilterBatchPlan plan = filter_batch_plan(filter_of_query, nq, segment.data(), n_filters);
    if (!shards_.empty()) {  // (automatic sharding of an exact-scan index: only the unfiltered batch is served)
        if (!plan.groups.empty())
            throw EngineError(Err::SpaceIncompatible, "an index spread over " + std::to_string(shards_.size()) + kEachSharded +
                                                          kFilterServed);
        knn_device(d_queries, nq, elem_count, k, d_ids, d_dists, d_cnt, stream);
        if (routes) std::fill(routes, routes + nq, last_path);
        each_path_ = last_path;
        last_path = 9;
        return;
    }
    if (d_n_ > 0 && elem_count != dim_) throw EngineError(Err::QueryExecutionFailed, "query dimension does not match the index");
    // before anything is enqueued: an exact-scan filter whose index was prepared again gathers again (and waits)
    for (const FilterBatchGroup& g : plan.groups) filter_begin_batch(*filters[g.filter]);

    // ---- what the device reads of the plan: one block, staged in pinned memory of our own (the caller's arrays are free
    // when the call returns) ----
    const bool permute = !plan.identity, table = hnsw && !plan.groups.empty();
    const size_t tab_bytes = table ? (n_filters * sizeof(FilterSlot) + 15) & ~(size_t)15 : 0;
    const size_t up_bytes = tab_bytes + (table ? nq * 4 : 0) + (permute ? 2 * nq * 4 : 0);
    const FilterSlot* d_table = nullptr;
    const int32_t *d_slot = nullptr, *d_perm = nullptr, *d_inv = nullptr;
    if (up_bytes > 0) {
        char* hp = static_cast<char*>(each_.staged.begin(up_bytes, "filter batch"));
        each_.tab.ensure(up_bytes);
        const char* dp = static_cast<const char*>(each_.tab.ptr());
        size_t at = 0;
        if (table) {
            FilterSlot* t = reinterpret_cast<FilterSlot*>(hp);
            for (size_t j = 0; j < n_filters; ++j) {
                const Filter& f = *filters[j];
                const bool subset = segment[j] == kSegSubset;
                t[j] = {f.d_allow.as<uint32_t>(), subset && f.m > 0 ? f.d_list.as<int32_t>() : nullptr, (int)f.n,
                        subset ? (int)f.m : 0};
            }
            int32_t* slot = reinterpret_cast<int32_t*>(hp + tab_bytes);
            for (size_t p = 0; p < nq; ++p) slot[p] = std::max(filter_of_query[plan.perm[p]], 0);  // (unfiltered: not read)
            d_table = reinterpret_cast<const FilterSlot*>(dp);
            d_slot = reinterpret_cast<const int32_t*>(dp + tab_bytes);
            at = tab_bytes + nq * 4;
        }
        if (permute) {
            std::memcpy(hp + at, plan.perm.data(), nq * 4);
            std::memcpy(hp + at + nq * 4, plan.inv.data(), nq * 4);
            d_perm = reinterpret_cast<const int32_t*>(dp + at);
            d_inv = d_perm + nq;
        }
    }
    order_after_last(stream);
    if (up_bytes > 0) {
        hip_check(hipMemcpyAsync(each_.tab.ptr(), each_.staged.ptr(), up_bytes, hipMemcpyHostToDevice, stream), "filter batch H2D");
        each_.staged.sent(stream);
    }

    // ---- the batch in plan order: the caller's arrays when it is in that order already, else workspaces ----
    const size_t qbytes = elem_count * elem_bytes(), rb = k * 4;
    const char* q = static_cast<const char*>(d_queries);
    int32_t* ids = d_ids;
    float* dists = d_dists;
    int32_t* cnt = d_cnt;
    if (hnsw) {  // results and work counters of the whole batch, as knn_device keeps them
        for (DevBuf* b : {&ws_ndc_, &ws_hops_, &ws_hops_up_, &sw_.status}) b->ensure(nq * 4);
        if (!d_cnt) sw_.outcnt.ensure(nq * 4);
        if (!cnt) cnt = sw_.outcnt.as<int32_t>();
    }
    int32_t *ndc = ws_ndc_.as<int32_t>(), *hops = ws_hops_.as<int32_t>(), *hops_up = ws_hops_up_.as<int32_t>();
    if (permute) {
        each_.q.ensure(nq * qbytes);
        each_.res.ensure(2 * nq * rb + 4 * nq * 4);
        gather_rows(d_queries, d_perm, nq, qbytes, each_.q.ptr(), stream);
        q = static_cast<const char*>(each_.q.ptr());
        ids = each_.res.as<int32_t>();
        dists = reinterpret_cast<float*>(ids + nq * k);
        cnt = ids + 2 * nq * k;
        ndc = cnt + nq;
        hops = ndc + nq;
        hops_up = hops + nq;
    }
    auto route_of = [&](size_t a, size_t b) {  // plan positions [a, b) took the path last_path names
        if (routes)
            for (size_t p = a; p < b; ++p) routes[plan.perm[p]] = last_path;
    };

    if (hnsw) {
        const HnswOut out{ids, dists, cnt, ndc, hops, hops_up, sw_.status.as<int32_t>()};
        const uint32_t* tomb = n_dead_ > 0 ? d_tomb_.as<uint32_t>() : nullptr;
        // knn_device's slices of the batch, in plan order; a slice runs the part of every segment that lies in it
        for (size_t s0 = 0; s0 < nq; s0 += 65536) {
            const size_t s1 = std::min(nq, s0 + 65536);
            for (int sg = 0; sg < kSegCount; ++sg) {
                const size_t a = std::max(s0, plan.seg[sg]), b = std::min(s1, plan.seg[sg + 1]);
                if (a >= b) continue;
                const void* qs = q + a * qbytes;
                const FilterEach ea{d_table, d_slot ? d_slot + a : nullptr};
                if (sg == kSegUnfiltered) {
                    knn_hnsw(qs, b - a, k, out.at(a, k), stream);
                } else if (sg == kSegWalk) {
                    if (inwalk_serves(k)) knn_hnsw_inwalk(qs, b - a, k, nullptr, 0, out.at(a, k), stream, &ea);
                    else knn_hnsw_two_stage(qs, b - a, k, nullptr, 0, out.at(a, k), stream, &ea);
                } else {
                    size_t m_max = 0;  // the launch's LDS: the largest list among the filters with queries in [a, b)
                    for (const FilterBatchGroup& g : plan.groups)
                        if (g.begin < b && g.end > a && segment[g.filter] == kSegSubset) m_max = std::max(m_max, filters[g.filter]->m);
                    HnswDeviceGraph g = dg_;
                    g.rows16 = nullptr;  // always the f32 rows: the bits of the f32 walk
                    have_counters_ = true;
                    hnsw_fix_valid_ = false;
                    last_path = 7;
                    prof_begin(stream);
                    hip_check(launch_hnsw_subset_knn_each(g, (int)(b - a), (int)k, qs, ea, (int)m_max, tomb, out.at(a, k), stream),
                              "hnsw_subset_knn");
                    prof_end(stream);
                }
                route_of(a, b);
            }
        }
    } else {
        // one knn_brute per part: the index itself for the unfiltered queries, then every filter's child over its group;
        // parts beyond 32768 queries are cut as knn_device cuts them
        auto run = [&](Filter* f, size_t a, size_t b) {
            for (size_t q0 = a; q0 < b; q0 += 32768) {
                const size_t m = std::min<size_t>(32768, b - q0);
                int32_t* c = cnt ? cnt + q0 : nullptr;
                if (f) knn_filtered_slice(*f, q + q0 * qbytes, m, k, ids + q0 * k, dists + q0 * k, c, stream);
                else knn_brute(q + q0 * qbytes, m, k, ids + q0 * k, dists + q0 * k, c, stream);
            }
            route_of(a, b);
        };
        if (plan.seg[kSegWalk] > 0) run(nullptr, 0, plan.seg[kSegWalk]);
        for (const FilterBatchGroup& g : plan.groups) run(filters[g.filter], g.begin, g.end);
        have_counters_ = false;
    }

    if (permute) {  // back to the caller's order: row q of the results is plan row inv[q]
        gather_rows(ids, d_inv, nq, rb, d_ids, stream);
        gather_rows(dists, d_inv, nq, rb, d_dists, stream);
        if (d_cnt) gather_rows(cnt, d_inv, nq, 4, d_cnt, stream);
        if (hnsw) {
            gather_rows(ndc, d_inv, nq, 4, ws_ndc_.ptr(), stream);
            gather_rows(hops, d_inv, nq, 4, ws_hops_.ptr(), stream);
            gather_rows(hops_up, d_inv, nq, 4, ws_hops_up_.ptr(), stream);
        }
    }
    each_path_ = last_path;
    last_path = 9;
}

void Engine::knn_host_each(Filter* const* filters, size_t n_filters, const int32_t* filter_of_query, const void* queries,
                           size_t nq, size_t elem_count, size_t k, const int32_t** ids, const float** dists,
                           const int32_t** cnt, int32_t* routes) {
    check_filters_each(filters, n_filters, filter_of_query, nq);  // (refused before the index is finalized for it)
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    *ids = nullptr;
    *dists = nullptr;
    *cnt = nullptr;
    if (nq == 0) return;
    if (dirty_) finalize();
    check_device();
    const size_t qbytes = nq * elem_count * elem_bytes();
    ws_q_.ensure(qbytes);
    const ResultBlock out = result_block(nq, k);
    char* hp = static_cast<char*>(pinned(std::max(qbytes, 2 * nq * k * 4 + nq * 4)));
    std::memcpy(hp, queries, qbytes);
    order_after_last(stream_);
    hip_check(hipMemcpyAsync(ws_q_.ptr(), hp, qbytes, hipMemcpyHostToDevice, stream_), "queries H2D");
    knn_device_each(filters, n_filters, filter_of_query, ws_q_.ptr(), nq, elem_count, k, out.ids, out.dists, out.cnt, stream_,
                    routes);
    fetch_results(nq, k, "knn", ids, dists, cnt);
}

}  // namespace gfxknn
