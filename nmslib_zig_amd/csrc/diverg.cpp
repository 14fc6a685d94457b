// The divergence spaces on the engine (KL, generalized KL, Itakura-Saito, Jensen-Shannon over dense float rows): the
// logarithms an object carries, the rows' copy in HBM, and the k-NN batch / range / pair entries over
// kernels/diverg_kernels.hip.  A divergence index is a brute-force index on one device.
//
// Every logarithm and reciprocal the kernels read is taken HERE, on the host, whichever entry a query comes through:
// the bits of a distance then do not depend on the entry.  (This file is compiled without contraction.)
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>

#include "engine.hpp"

namespace gfxknn {

// The logarithm stored beside a value: PrecompLogarithms (include/distcomp.h:149-154) for the spaces whose objects
// carry their logarithms; the guard of JSStandard (src/distcomp_js.cc:53-54) for jsdivslow / jsmetrslow, whose
// per-object logarithms are the same for every pair.  kldivgenslow takes log(x / y) per pair on the device.
static inline float diverg_log(int space, float x) {
    if (space == SP_JSDIV_SLOW || space == SP_JSMETR_SLOW) return x < std::numeric_limits<float>::min() ? 0.0f : logf(x);
    return x > 0 ? logf(x) : -1e5f;
}

bool Engine::diverg_stores_logs() const { return diverg_ && space_ != SP_KLDIVGEN_SLOW && space_ != SP_JSDIV_SLOW && space_ != SP_JSMETR_SLOW; }

void Engine::diverg_logs(const float* x, size_t count, float* out) const {
    for (size_t i = 0; i < count; ++i) out[i] = diverg_log(space_, x[i]);
}

// `count` objects of dim_ floats at src (object i at src + i * dim_) -> the kernels' query planes with `stride`
// queries per group: vals | logs | inv, each [G][stride][4], zero where there is no element
static void pack_queries(int space, const float* src, size_t count, size_t dim, size_t stride, float* vals, float* logs,
                         float* inv) {
    const size_t G = (size_t)diverg_groups((int)dim);
    std::memset(vals, 0, G * stride * 16);
    std::memset(logs, 0, G * stride * 16);
    if (inv) std::memset(inv, 0, G * stride * 16);
    for (size_t q = 0; q < count; ++q)
        for (size_t j = 0; j < dim; ++j) {
            const float x = src[q * dim + j];
            const size_t at = ((j >> 2) * stride + q) * 4 + (j & 3);
            vals[at] = x;
            logs[at] = diverg_log(space, x);
            if (inv) inv[at] = 1.0f / x;
        }
}

void Engine::upload_diverg() {
    check_device();
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = ids_.size();
    const int D = (int)dim_;
    const size_t G = (size_t)diverg_groups(D), plane = diverg_row_plane_floats(n, D);
    std::vector<float> h(2 * std::max<size_t>(plane, 4), 0.f);
    float* hv = h.data();
    float* hl = h.data() + plane;
    for (size_t r = 0; r < n; ++r) {
        const float* x = &rows_f32_[r * dim_];
        const size_t base = ((r >> 6) * G) * 256 + (r & 63) * 4;
        for (size_t j = 0; j < dim_; ++j) {
            const size_t at = base + (j >> 2) * 256 + (j & 3);
            hv[at] = x[j];
            hl[at] = diverg_log(space_, x[j]);
        }
    }
    d_rows_.ensure(h.size() * 4);
    d_ids_.ensure(std::max<size_t>(n, 1) * sizeof(int32_t));
    hip_check(hipMemcpyAsync(d_rows_.ptr(), h.data(), h.size() * 4, hipMemcpyHostToDevice, stream_), "diverg rows H2D");
    if (n) hip_check(hipMemcpyAsync(d_ids_.ptr(), ids_.data(), n * 4, hipMemcpyHostToDevice, stream_), "ids H2D");
    hip_check(hipStreamSynchronize(stream_), "diverg upload");
    d_n_ = n;
    rows_uploaded = n;
    rows_appended = 0;
    upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

DivergRows Engine::diverg_rows() const {
    const size_t plane = diverg_row_plane_floats(d_n_, (int)dim_);
    return DivergRows{d_rows_.as<float>(), d_rows_.as<float>() + plane, (int)d_n_, (int)dim_, diverg_groups((int)dim_)};
}

void Engine::knn_diverg_host(const float* queries, size_t nq, size_t elem_count, size_t k, const int32_t** ids,
                             const float** dists, const int32_t** cnt) {
    if (k == 0) throw EngineError(Err::InvalidArgument, "k must be positive");
    if (k > (size_t)INT32_MAX / 2) throw EngineError(Err::QueryTooLarge, "k is too large");
    const size_t D = d_n_ > 0 ? dim_ : elem_count;
    // a tile of the scan reads kDivergTileQ queries from its first one: the pack is that much longer than the batch
    const size_t stride = nq + kDivergTileQ, G = (size_t)diverg_groups((int)D), plane = G * stride * 4;
    const bool with_inv = space_ == SP_ITAKURASAITO;
    const size_t qbytes = (with_inv ? 3 : 2) * plane * 4;
    float* hp = static_cast<float*>(pinned(std::max(qbytes, 2 * nq * k * 4 + nq * 4)));
    pack_queries(space_, queries, nq, D, stride, hp, hp + plane, with_inv ? hp + 2 * plane : nullptr);
    ws_bq_.ensure(qbytes);
    hip_check(hipMemcpyAsync(ws_bq_.ptr(), hp, qbytes, hipMemcpyHostToDevice, stream_), "diverg queries H2D");
    const float* dq = ws_bq_.as<float>();
    const DivergQueries q{dq, dq + plane, with_inv ? dq + 2 * plane : nullptr, (int)stride};
    const DivergRows rows = diverg_rows();
    const ResultBlock out = result_block(nq, k);
    scan_slices(nq, k, kDivergTileQ, out, [&](const ScanPlan& p, size_t q0, float* split_d, int32_t* split_pos) {
        hip_check(launch_diverg_knn(space_, p, rows, q, (int)q0, split_d, split_pos, stream_), "diverg scan");
    });
    fetch_results(nq, k, "diverg knn", ids, dists, cnt);
    last_path = 0;
}

size_t Engine::range_diverg_host(const float* query, size_t elem_count, double radius, size_t capacity, int32_t* ids,
                                 float* dists) {
    const size_t n = d_n_;
    if (n == 0 || capacity == 0) return 0;  // (the query's length was checked by range_host)
    // RangeQuery<dist_t>(space, obj, static_cast<dist_t>(radius)), nmslib_c.cpp:1092-1093
    const float r = (float)radius;
    const size_t plane = (size_t)diverg_groups((int)dim_) * 4;
    std::vector<float> h(2 * plane);
    pack_queries(space_, query, 1, dim_, 1, h.data(), h.data() + plane, nullptr);
    ws_q_.ensure(h.size() * 4);
    const float* dq = ws_q_.as<float>();
    // the filter uses d(row, query), the reported distance is d(query, row)
    return range_select(true, r, capacity, ids, dists, [&](float* filter, float* report) {
        hip_check(hipMemcpyAsync(ws_q_.ptr(), h.data(), h.size() * 4, hipMemcpyHostToDevice, stream_), "query H2D");
        hip_check(launch_diverg_dist(space_, diverg_rows(), DivergQueries{dq, dq + plane, nullptr, 1}, filter, report,
                                     stream_),
                  "diverg range distances");
    });
}

float Engine::pair_distance_diverg(size_t p1, size_t p2) {
    // IndexTimeDistance(data[p1], data[p2]) (nmslib_c.cpp:1166) from the host rows: no finalize needed
    check_device();
    order_after_last(stream_);
    const size_t plane = (size_t)diverg_groups((int)dim_) * 2 * 4;
    std::vector<float> two(2 * dim_), h(2 * plane);
    std::memcpy(two.data(), &rows_f32_[p1 * dim_], dim_ * 4);
    std::memcpy(two.data() + dim_, &rows_f32_[p2 * dim_], dim_ * 4);
    pack_queries(space_, two.data(), 2, dim_, 2, h.data(), h.data() + plane, nullptr);
    ws_pair_.ensure(h.size() * 4 + 16);
    float* base = ws_pair_.as<float>();
    float* out = base + h.size();
    hip_check(hipMemcpyAsync(base, h.data(), h.size() * 4, hipMemcpyHostToDevice, stream_), "pair H2D");
    hip_check(launch_diverg_pair(space_, DivergQueries{base, base + plane, nullptr, 2}, (int)dim_, out, stream_),
              "diverg pair distance");
    return read_float(out, "diverg pair distance");
}

}  // namespace gfxknn
