// Sparse rows on the engine: the host CSR, its copy in HBM, and the k-NN batch / range / pair entries over
// kernels/sparse_kernels.hip.  A sparse index is a brute-force index on one device.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "engine.hpp"

namespace gfxknn {

// NMSLIB_GPU_SPARSE_FAST=0 turns the inverted-file path off (read at finalize and per batch); unset, it is on
static bool sparse_fast_enabled() {
    const char* env = getenv("NMSLIB_GPU_SPARSE_FAST");
    return !(env && atoi(env) == 0);
}

void Engine::add_sparse_row(const SparseElem* elems, size_t count, int32_t id) {
    if (!sparse_) throw EngineError(Err::SpaceIncompatible, "Not sparse space");
    if (count == 0 || count > (size_t)INT32_MAX)
        throw EngineError(Err::InvalidArgument, "a sparse row holds between 1 and 2^31-1 elements");
    if (ids_.size() >= (size_t)INT32_MAX) throw EngineError(Err::InvalidArgument, "too many rows for one index");
    for (size_t i = 0; i < count; ++i) {  // (push_back: geometric growth; an exact reserve per row would be quadratic)
        sp_ids_.push_back(elems[i].id);
        sp_vals_.push_back(elems[i].value);
    }
    sp_ptr_.push_back((int64_t)sp_ids_.size());
    ids_.push_back(id);
    dirty_ = true;
}

void Engine::sparse_row(size_t pos, SparseElem* dst) const {
    const int64_t b = sp_ptr_[pos], e = sp_ptr_[pos + 1];
    for (int64_t i = b; i < e; ++i) dst[i - b] = SparseElem{sp_ids_[(size_t)i], sp_vals_[(size_t)i]};
}

void Engine::upload_sparse() {
    check_device();
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = ids_.size(), nnz = sp_ids_.size();
    d_sp_ptr_.ensure((n + 1) * sizeof(int64_t));
    d_sp_ids_.ensure(std::max<size_t>(nnz, 1) * sizeof(uint32_t));
    d_sp_vals_.ensure(std::max<size_t>(nnz, 1) * sizeof(float));
    d_ids_.ensure(std::max<size_t>(n, 1) * sizeof(int32_t));
    hip_check(hipMemcpyAsync(d_sp_ptr_.ptr(), sp_ptr_.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, stream_),
              "sparse row_ptr H2D");
    if (nnz) {
        hip_check(hipMemcpyAsync(d_sp_ids_.ptr(), sp_ids_.data(), nnz * 4, hipMemcpyHostToDevice, stream_), "sparse ids H2D");
        hip_check(hipMemcpyAsync(d_sp_vals_.ptr(), sp_vals_.data(), nnz * 4, hipMemcpyHostToDevice, stream_),
                  "sparse vals H2D");
    }
    if (n) hip_check(hipMemcpyAsync(d_ids_.ptr(), ids_.data(), n * 4, hipMemcpyHostToDevice, stream_), "ids H2D");
    hip_check(hipStreamSynchronize(stream_), "sparse upload");
    d_n_ = n;
    rows_uploaded = n;
    rows_appended = 0;
    // the filter's copy: made here unless the path is turned off (a later batch that finds it on makes the copy then)
    sinv_.tried = false;
    sinv_.drop_copy();
    if (sparse_fast_enabled()) make_sparse_inv_copy();
    upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// Stable sort of (term << 32 | posting index) keys by term: 11 bits per pass, passes above the largest term skipped.
// The indexes come in ascending, so inside a term they stay ascending: ascending in row.
static void sort_by_term(std::vector<uint64_t>& keys, std::vector<uint64_t>& tmp, uint32_t max_term) {
    tmp.resize(keys.size());
    for (int shift = 32; shift < 64 && ((uint64_t)max_term >> (shift - 32)) != 0; shift += 11) {
        size_t count[2049] = {0};
        for (const uint64_t key : keys) ++count[((key >> shift) & 2047) + 1];
        for (int d = 0; d < 2048; ++d) count[d + 1] += count[d];
        for (const uint64_t key : keys) tmp[count[(key >> shift) & 2047]++] = key;
        keys.swap(tmp);
    }
}

// The resident side of the inverted-file filter (sparse_filter.hpp, kernels.hpp SparseInvFile).  The
// index declines the copy, and is served by the exact scan alone, when it has fewer than spf::kMinRows rows, a stored
// value is not finite, a row's ids are not strictly ascending (two postings of one segment would hit the same
// accumulator), a cosine-family row's norm is one the proof cannot work with (spf::row_class), or an allocation fails.
// An index finalized with the path turned off pays neither the pass over the rows nor the memory.
void Engine::make_sparse_inv_copy() {
    SparseInv& f = sinv_;
    f.tried = true;
    f.drop_copy();
    const int kind = sparse_fast_kind(space_);
    const size_t n = ids_.size();
    if (kind < 0 || n < (size_t)spf::kMinRows || n > (size_t)INT32_MAX) return;
    // per row: the divisor of its stored values (0: no postings), the norm of the stored values, the checks
    std::vector<double> divisor(n, 1.0);
    double beta2 = 0;
    size_t longest = 0;
    for (size_t r = 0; r < n; ++r) {
        const size_t b = (size_t)sp_ptr_[r], e = (size_t)sp_ptr_[r + 1];
        longest = std::max(longest, e - b);
        double s = 0;
        for (size_t i = b; i < e; ++i) {
            if (!std::isfinite(sp_vals_[i]) || (i > b && sp_ids_[i - 1] >= sp_ids_[i])) return;
            s += (double)sp_vals_[i] * (double)sp_vals_[i];
        }
        const int cls = spf::row_class(kind, s);
        if (cls == spf::ROW_DECLINE) return;
        if (cls == spf::ROW_EMPTY) {
            divisor[r] = 0.0;
            continue;
        }
        if (spf::cosine_kind(kind)) {
            divisor[r] = std::sqrt(s);
            s = 0;
            for (size_t i = b; i < e; ++i) {
                const double v = (double)spf::stored_value(kind, sp_vals_[i], divisor[r]);
                s += v * v;
            }
        }
        beta2 = std::max(beta2, s);
    }
    const float beta = spf::round_up_f32(std::sqrt(beta2) * (1.0 + 9.094947017729282e-13));   // (2^-40: the f64 sum and root)
    if (!std::isfinite(beta)) return;
    const size_t B = (size_t)spf::kBlockRows, nblocks = (n + B - 1) / B;
    std::vector<int64_t> blk_term(nblocks + 1, 0), blk_post(nblocks + 1, 0);
    std::vector<uint32_t> terms, seg;
    std::vector<uint16_t> post_row;
    std::vector<float> post_val;
    post_row.reserve(sp_ids_.size());
    post_val.reserve(sp_ids_.size());
    std::vector<uint64_t> keys, tmp;
    std::vector<uint16_t> row_of;
    for (size_t blk = 0; blk < nblocks; ++blk) {
        const size_t r0 = blk * B, r1 = std::min(n, r0 + B), base = (size_t)sp_ptr_[r0];
        if ((size_t)sp_ptr_[r1] - base > (size_t)UINT32_MAX) return;   // (a segment start is 32 bits)
        keys.clear();
        row_of.assign((size_t)sp_ptr_[r1] - base, 0);   // posting index within the block -> row within the block
        uint32_t max_term = 0;
        for (size_t r = r0; r < r1; ++r) {
            if (divisor[r] == 0.0) continue;
            for (size_t i = (size_t)sp_ptr_[r]; i < (size_t)sp_ptr_[r + 1]; ++i) {
                row_of[i - base] = (uint16_t)(r - r0);
                keys.push_back(((uint64_t)sp_ids_[i] << 32) | (uint64_t)(i - base));
                max_term = std::max(max_term, sp_ids_[i]);
            }
        }
        sort_by_term(keys, tmp, max_term);
        for (size_t j = 0; j < keys.size(); ++j) {
            const uint32_t term = (uint32_t)(keys[j] >> 32);
            const size_t at = (size_t)(uint32_t)keys[j], row = r0 + row_of[at];
            if (j == 0 || term != (uint32_t)(keys[j - 1] >> 32)) {
                terms.push_back(term);
                seg.push_back((uint32_t)j);
            }
            post_row.push_back(row_of[at]);
            post_val.push_back(spf::stored_value(kind, sp_vals_[base + at], divisor[row]));
        }
        seg.push_back((uint32_t)keys.size());
        blk_term[blk + 1] = (int64_t)terms.size();
        blk_post[blk + 1] = (int64_t)post_row.size();
    }
    try {
        f.blk_term.ensure(blk_term.size() * 8);
        f.blk_post.ensure(blk_post.size() * 8);
        f.terms.ensure(std::max<size_t>(terms.size(), 1) * 4);
        f.seg.ensure(seg.size() * 4);
        f.post_row.ensure(std::max<size_t>(post_row.size(), 1) * 2);
        f.post_val.ensure(std::max<size_t>(post_val.size(), 1) * 4);
        hip_check(hipMemcpyAsync(f.blk_term.ptr(), blk_term.data(), blk_term.size() * 8, hipMemcpyHostToDevice, stream_), "inverted file H2D");
        hip_check(hipMemcpyAsync(f.blk_post.ptr(), blk_post.data(), blk_post.size() * 8, hipMemcpyHostToDevice, stream_), "inverted file H2D");
        hip_check(hipMemcpyAsync(f.seg.ptr(), seg.data(), seg.size() * 4, hipMemcpyHostToDevice, stream_), "inverted file H2D");
        if (!terms.empty())
            hip_check(hipMemcpyAsync(f.terms.ptr(), terms.data(), terms.size() * 4, hipMemcpyHostToDevice, stream_), "inverted file H2D");
        if (!post_row.empty()) {
            hip_check(hipMemcpyAsync(f.post_row.ptr(), post_row.data(), post_row.size() * 2, hipMemcpyHostToDevice, stream_), "inverted file H2D");
            hip_check(hipMemcpyAsync(f.post_val.ptr(), post_val.data(), post_val.size() * 4, hipMemcpyHostToDevice, stream_), "inverted file H2D");
        }
        hip_check(hipStreamSynchronize(stream_), "inverted file copy");
        f.beta = beta;
        f.longest = (int)longest;
        f.nblocks = (int)nblocks;
        f.have = true;
    } catch (const EngineError& e) {
        if (e.code != Err::OutOfMemory) throw;
        (void)hipGetLastError();
        f.drop_copy();
    }
}

void Engine::knn_sparse_host(const SparseElem* const* queries, const size_t* counts, size_t nq, size_t k,
                             const int32_t** ids, const float** dists, const int32_t** cnt) {
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (dirty_) finalize();
    check_device();
    order_after_last(stream_);
    if (k == 0) throw EngineError(Err::InvalidArgument, "k must be positive");
    if (k > (size_t)INT32_MAX / 2) throw EngineError(Err::QueryTooLarge, "k is too large");
    size_t total = 0, longest = 0;
    bool ascending = true;   // every query's ids strictly ascending (the filter's gate; the scan takes any order)
    for (size_t i = 0; i < nq; ++i) {
        total += counts[i];
        longest = std::max(longest, counts[i]);
        for (size_t j = 1; j < counts[i] && ascending; ++j) ascending = queries[i][j - 1].id < queries[i][j].id;
    }
    const int kind = sparse_fast_kind(space_);
    const bool opted = sparse_fast_enabled();
    // (an index finalized with the path off: the first batch that finds it on and could take it makes the copy)
    if (opted && !sinv_.tried && spf::plan(kind, (long long)d_n_, (long long)nq, (long long)k, (long long)longest, ascending, true).use)
        make_sparse_inv_copy();
    const spf::Plan fp = spf::plan(kind, (long long)d_n_, (long long)nq, (long long)k, (long long)longest, ascending, sinv_.have);
    pinned(std::max(sparse_pack_bytes(nq, total), 2 * nq * k * 4 + nq * 4));   // (one size for the whole call: a growth keeps nothing)
    const SparseBatch q = upload_sparse_queries(queries, counts, nq, nullptr);
    const ResultBlock out = result_block(nq, k);
    if (!fp.use || !opted) {
        sparse_scan_batch(q, nq, k, out);
        fetch_results(nq, k, "sparse knn", ids, dists, cnt);
        last_path = 0;
        return;
    }
    // the inner-product spaces: inverted-file filter, exact re-rank, proof (kernels/sparse_inv_kernels.hip)
    SparseInv& f = sinv_;
    const SparseInvFile file{f.blk_term.as<int64_t>(), f.terms.as<uint32_t>(), f.seg.as<uint32_t>(), f.blk_post.as<int64_t>(),
                             f.post_row.as<uint16_t>(), f.post_val.as<float>(), (int)d_n_, f.nblocks, f.beta, f.longest};
    // a slice of queries: its grid below 2^31 workgroups, its candidate lists within 256 MiB (one query always fits)
    const size_t per_query = (size_t)fp.nblocks * fp.keep * 4;
    const size_t slice = std::max<size_t>(1, std::min({nq, (size_t)INT32_MAX / (size_t)fp.nblocks, ((size_t)256 << 20) / per_query}));
    SparseInvWs ws{};
    ws.cand = static_cast<int32_t*>(f.ws_cand.ensure(slice * per_query));
    ws.tblock = static_cast<float*>(f.ws_tblock.ensure(slice * fp.nblocks * 4));
    ws.flags = static_cast<int*>(f.ws_flags.ensure(nq * 4));
    prof_begin(stream_);
    for (size_t q0 = 0; q0 < nq; q0 += slice)
        hip_check(launch_sparse_inv(space_, fp, file, (int)q0, (int)std::min(slice, nq - q0), (int)k, d_sp_ptr_.as<int64_t>(),
                                    d_sp_ids_.as<uint32_t>(), d_sp_vals_.as<float>(), q.q_ptr, q.q_ids, q.q_vals, q.q_norm, ws,
                                    d_ids_.as<int32_t>(), out.dists, out.ids, out.cnt, stream_),
                  "sparse inverted-file scan");
    prof_end(stream_);
    std::vector<int> flags(nq);
    hip_check(hipMemcpyAsync(flags.data(), ws.flags, nq * 4, hipMemcpyDeviceToHost, stream_), "sparse flags D2H");
    hip_check(hipStreamSynchronize(stream_), "sparse inverted-file scan");
    last_path = 15;
    fast_flags_ = ws.flags;
    fast_nqt_ = (int)nq;
    fast_has_precise_ = false;
    // queries without a proof: again, as one compacted batch through the exact scan
    std::vector<size_t> redo;
    for (size_t q1 = 0; q1 < nq; ++q1)
        if (flags[q1]) redo.push_back(q1);
    std::vector<char> sub_host;
    if (!redo.empty()) {
        const size_t m = redo.size();
        const SparseBatch sq = upload_sparse_queries(queries, counts, m, &redo);
        int32_t* sub_ids = static_cast<int32_t*>(f.ws_sub.ensure(2 * m * k * 4 + m * 4));
        const ResultBlock sub{sub_ids, reinterpret_cast<float*>(sub_ids + m * k), sub_ids + 2 * m * k};
        sparse_scan_batch(sq, m, k, sub);
        sub_host.resize(2 * m * k * 4 + m * 4);
        hip_check(hipMemcpyAsync(sub_host.data(), sub_ids, sub_host.size(), hipMemcpyDeviceToHost, stream_), "sparse redo D2H");
    }
    fetch_results(nq, k, "sparse knn", ids, dists, cnt);
    if (!redo.empty()) {   // the redone rows over the filter's
        const size_t m = redo.size(), row = k * 4;
        char* hp = static_cast<char*>(pinned_.ptr());
        for (size_t i = 0; i < m; ++i) {
            std::memcpy(hp + redo[i] * row, sub_host.data() + i * row, row);
            std::memcpy(hp + nq * row + redo[i] * row, sub_host.data() + m * row + i * row, row);
            std::memcpy(hp + 2 * nq * row + redo[i] * 4, sub_host.data() + 2 * m * row + i * 4, 4);
        }
    }
}

// the batch's queries as the kernels read them: q_ptr int64 [nq+1] | ids u32 [total] | vals f32 [total] | 2-norms f64 [nq],
// packed in the pinned block (sized by the caller) and copied to ws_bq_.  pick: the batch is queries[(*pick)[i]], i < nq
Engine::SparseBatch Engine::upload_sparse_queries(const SparseElem* const* queries, const size_t* counts, size_t nq,
                                                  const std::vector<size_t>* pick) {
    size_t total = 0;
    for (size_t i = 0; i < nq; ++i) total += counts[pick ? (*pick)[i] : i];
    const size_t ptr_b = (nq + 1) * 8, ids_b = align8(total * 4), qbytes = sparse_pack_bytes(nq, total);
    char* hp = static_cast<char*>(pinned_.ptr());
    int64_t* hptr = reinterpret_cast<int64_t*>(hp);
    uint32_t* hids = reinterpret_cast<uint32_t*>(hp + ptr_b);
    float* hvals = reinterpret_cast<float*>(hp + ptr_b + ids_b);
    double* hnorm = reinterpret_cast<double*>(hp + ptr_b + 2 * ids_b);
    size_t at = 0;
    for (size_t i = 0; i < nq; ++i) {
        const size_t src = pick ? (*pick)[i] : i;
        hptr[i] = (int64_t)at;
        double s = 0;
        for (size_t j = 0; j < counts[src]; ++j) {
            hids[at + j] = queries[src][j].id;
            hvals[at + j] = queries[src][j].value;
            s += (double)queries[src][j].value * (double)queries[src][j].value;
        }
        hnorm[i] = std::sqrt(s);
        at += counts[src];
    }
    hptr[nq] = (int64_t)at;
    ws_bq_.ensure(qbytes);
    hip_check(hipMemcpyAsync(ws_bq_.ptr(), hp, qbytes, hipMemcpyHostToDevice, stream_), "sparse queries H2D");
    const char* d = ws_bq_.as<char>();
    return SparseBatch{reinterpret_cast<const int64_t*>(d), reinterpret_cast<const uint32_t*>(d + ptr_b),
                       reinterpret_cast<const float*>(d + ptr_b + ids_b), reinterpret_cast<const double*>(d + ptr_b + 2 * ids_b)};
}

// the exact scan of a batch into `out` (enqueued)
void Engine::sparse_scan_batch(const SparseBatch& q, size_t nq, size_t k, const ResultBlock& out) {
    scan_slices(nq, k, kSparseTileQ, out, [&](const ScanPlan& p, size_t q0, float* split_d, int32_t* split_pos) {
        hip_check(launch_sparse_knn(space_, p, d_sp_ptr_.as<int64_t>(), d_sp_ids_.as<uint32_t>(), d_sp_vals_.as<float>(),
                                    q.q_ptr + q0, q.q_ids, q.q_vals, split_d, split_pos, stream_),
                  "sparse scan");
    });
}

size_t Engine::range_sparse_host(const SparseElem* query, size_t count, double radius, size_t capacity, int32_t* ids,
                                 float* dists) {
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (dirty_) finalize();
    check_device();
    order_after_last(stream_);
    const size_t n = d_n_;
    if (n == 0 || capacity == 0) return 0;
    // RangeQuery<dist_t>(space, obj, static_cast<dist_t>(radius)), nmslib_c.cpp:1092-1093
    const float r = (float)radius;
    std::vector<uint32_t> qi(count);
    std::vector<float> qv(count);
    for (size_t i = 0; i < count; ++i) {
        qi[i] = query[i].id;
        qv[i] = query[i].value;
    }
    const size_t ids_b = align8(count * 4);
    ws_q_.ensure(ids_b + count * 4);
    uint32_t* d_qi = ws_q_.as<uint32_t>();
    float* d_qv = reinterpret_cast<float*>(ws_q_.as<char>() + ids_b);
    hip_check(hipMemcpyAsync(d_qi, qi.data(), count * 4, hipMemcpyHostToDevice, stream_), "query H2D");
    hip_check(hipMemcpyAsync(d_qv, qv.data(), count * 4, hipMemcpyHostToDevice, stream_), "query H2D");
    // the filter uses d(row, query), the reported distance is d(query, row)
    return range_select(true, r, capacity, ids, dists, [&](float* filter, float* report) {
        hip_check(launch_sparse_dist(space_, d_sp_ptr_.as<int64_t>(), d_sp_ids_.as<uint32_t>(), d_sp_vals_.as<float>(),
                                     (int)n, d_qi, d_qv, (int)count, filter, report, stream_),
                  "sparse range distances");
    });
}

float Engine::pair_distance_sparse(size_t p1, size_t p2) {
    // IndexTimeDistance(data[p1], data[p2]) (nmslib_c.cpp:1166) from the host rows: no finalize needed
    check_device();
    order_after_last(stream_);
    const size_t n1 = sparse_row_len(p1), n2 = sparse_row_len(p2), tot = n1 + n2;
    const size_t ids_b = align8(tot * 4);
    std::vector<char> h(32 + ids_b + tot * 4);
    int64_t* ptr = reinterpret_cast<int64_t*>(h.data());
    ptr[0] = 0;
    ptr[1] = (int64_t)n1;
    ptr[2] = (int64_t)tot;
    uint32_t* hi = reinterpret_cast<uint32_t*>(h.data() + 32);
    float* hv = reinterpret_cast<float*>(h.data() + 32 + ids_b);
    std::memcpy(hi, &sp_ids_[(size_t)sp_ptr_[p1]], n1 * 4);
    std::memcpy(hi + n1, &sp_ids_[(size_t)sp_ptr_[p2]], n2 * 4);
    std::memcpy(hv, &sp_vals_[(size_t)sp_ptr_[p1]], n1 * 4);
    std::memcpy(hv + n1, &sp_vals_[(size_t)sp_ptr_[p2]], n2 * 4);
    ws_pair_.ensure(h.size() + 16);
    char* base = ws_pair_.as<char>();
    float* out = reinterpret_cast<float*>(base + align8(h.size()));
    hip_check(hipMemcpyAsync(base, h.data(), h.size(), hipMemcpyHostToDevice, stream_), "pair H2D");
    hip_check(launch_sparse_pair(space_, reinterpret_cast<const int64_t*>(base), reinterpret_cast<const uint32_t*>(base + 32),
                                 reinterpret_cast<const float*>(base + 32 + ids_b), 0, 1, out, stream_),
              "sparse pair distance");
    return read_float(out, "sparse pair distance");
}

}  // namespace gfxknn
