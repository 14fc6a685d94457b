// Sparse rows on the engine: the host CSR, its copy in HBM, and the k-NN batch / range / pair entries over
// kernels/sparse_kernels.hip.  A sparse index is a brute-force index on one device.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstring>

#include "engine.hpp"

namespace gfxknn {

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
    upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

void Engine::knn_sparse_host(const SparseElem* const* queries, const size_t* counts, size_t nq, size_t k,
                             const int32_t** ids, const float** dists, const int32_t** cnt) {
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (dirty_) finalize();
    check_device();
    order_after_last(stream_);
    if (k == 0) throw EngineError(Err::InvalidArgument, "k must be positive");
    if (k > (size_t)INT32_MAX / 2) throw EngineError(Err::QueryTooLarge, "k is too large");
    size_t total = 0;
    for (size_t i = 0; i < nq; ++i) total += counts[i];
    // device / pinned layout of the batch: q_ptr int64 [nq+1] | ids u32 [total] | vals f32 [total]
    const size_t ptr_b = (nq + 1) * 8, ids_b = align8(total * 4), qbytes = ptr_b + ids_b + total * 4;
    char* hp = static_cast<char*>(pinned(std::max(qbytes, 2 * nq * k * 4 + nq * 4)));
    int64_t* hptr = reinterpret_cast<int64_t*>(hp);
    uint32_t* hids = reinterpret_cast<uint32_t*>(hp + ptr_b);
    float* hvals = reinterpret_cast<float*>(hp + ptr_b + ids_b);
    size_t at = 0;
    for (size_t i = 0; i < nq; ++i) {
        hptr[i] = (int64_t)at;
        for (size_t j = 0; j < counts[i]; ++j) {
            hids[at + j] = queries[i][j].id;
            hvals[at + j] = queries[i][j].value;
        }
        at += counts[i];
    }
    hptr[nq] = (int64_t)at;
    ws_bq_.ensure(qbytes);
    hip_check(hipMemcpyAsync(ws_bq_.ptr(), hp, qbytes, hipMemcpyHostToDevice, stream_), "sparse queries H2D");
    const int64_t* d_qptr = ws_bq_.as<int64_t>();
    const uint32_t* d_qids = reinterpret_cast<const uint32_t*>(ws_bq_.as<char>() + ptr_b);
    const float* d_qvals = reinterpret_cast<const float*>(ws_bq_.as<char>() + ptr_b + ids_b);

    const ResultBlock out = result_block(nq, k);
    scan_slices(nq, k, kSparseTileQ, out, [&](const ScanPlan& p, size_t q0, float* split_d, int32_t* split_pos) {
        hip_check(launch_sparse_knn(space_, p, d_sp_ptr_.as<int64_t>(), d_sp_ids_.as<uint32_t>(), d_sp_vals_.as<float>(),
                                    d_qptr + q0, d_qids, d_qvals, split_d, split_pos, stream_),
                  "sparse scan");
    });
    fetch_results(nq, k, "sparse knn", ids, dists, cnt);
    last_path = 0;
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
