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
#include <cstdlib>
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

// NMSLIB_GPU_DIVERG_FAST=0 turns the MFMA filter path off (read at finalize and per batch); unset, it is on
static bool diverg_fast_enabled() {
    const char* env = getenv("NMSLIB_GPU_DIVERG_FAST");
    return !(env && atoi(env) == 0);
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
    // the Jensen-Shannon filter's side of the pass (diverg_js_filter.hpp): R_row in f64, kept as one float
    // per row (+inf in the padding of the last 64-row block), and the rows' maxima
    const bool js = diverg_js_space(space_) && n >= (size_t)dvf::kMinRows;
    std::vector<float> r32(js ? (n + 63) / 64 * 64 : 0, INFINITY);
    djs::RowMax jm{0.f, 0.f, 0.f};
    bool js_ok = js;
    for (size_t r = 0; r < n; ++r) {
        const float* x = &rows_f32_[r * dim_];
        const size_t base = ((r >> 6) * G) * 256 + (r & 63) * 4;
        for (size_t j = 0; j < dim_; ++j) {
            const size_t at = base + (j >> 2) * 256 + (j & 3);
            hv[at] = x[j];
            hl[at] = diverg_log(space_, x[j]);
        }
        if (js) {
            r32[r] = (float)djs::row(x, dim_, &jm, &js_ok);
            js_ok = js_ok && std::isfinite(r32[r]);
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
    // the filter's copy: made here unless the path is turned off (a later batch that finds it on makes the copy then)
    dfast_.have = dfast_.tried = false;
    dfast_.frags.release();
    dfast_.rrow.release();
    if (diverg_fast_enabled()) make_diverg_fast_copy();
    // a negative or non-finite element, a figure beyond f32 and a failed allocation leave the index to the exact scan
    dfast_.js_have = false;
    dfast_.js_r32.release();
    if (js_ok && std::isfinite(jm.lam) && std::isfinite(jm.sum) && std::isfinite(jm.xlnx)) {
        try {
            dfast_.js_r32.ensure(r32.size() * 4);
            hip_check(hipMemcpyAsync(dfast_.js_r32.ptr(), r32.data(), r32.size() * 4, hipMemcpyHostToDevice, stream_), "diverg row constants H2D");
            hip_check(hipStreamSynchronize(stream_), "diverg row constants");
            dfast_.js_max = jm;
            dfast_.js_have = true;
        } catch (const EngineError& e) {
            if (e.code != Err::OutOfMemory) throw;
            (void)hipGetLastError();
            dfast_.js_r32.release();
        }
    }
    upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The resident side of the MFMA filter scan (diverg_filter.hpp): the row operand as bf16 hi / lo
// fragments in the scan's layout, R_row and the rows' largest figures.  A non-finite element or figure and a failed
// allocation leave the path off and the index served by the exact scan alone.  An index finalized with the path turned
// off pays neither the pass over the rows nor the memory.
void Engine::make_diverg_fast_copy() {
    DivergFast& f = dfast_;
    f.have = false;
    f.tried = true;
    const int form = diverg_fast_form(space_);
    const size_t n = ids_.size(), D = dim_;
    if (form < 0 || n < (size_t)dvf::kMinRows || D < 1 || D > (size_t)dvf::kMaxDim) {
        f.frags.release();
        f.rrow.release();
        return;
    }
    const size_t ks = (D + 15) / 16, dpad = 16 * ks, n_pad = (n + 31) / 32 * 32;
    std::vector<uint16_t> frags(diverg_fast_frag_elems(n, (int)D), 0);
    std::vector<float> rrow(n_pad, INFINITY), lx(D);
    std::vector<uint16_t> hl(2 * dpad);
    dvf::RowMax m{0.f, 0.f, 0.f, 0.f, 0.f};
    bool finite = true;
    for (size_t r = 0; r < n && finite; ++r) {
        const float* x = &rows_f32_[r * D];
        for (size_t j = 0; j < D; ++j) {
            lx[j] = diverg_log(space_, x[j]);
            finite = finite && std::isfinite(x[j]);
        }
        const double R = dvf::row(form, x, lx.data(), D, dpad, hl.data(), hl.data() + dpad, &m);
        rrow[r] = (float)R;
        finite = finite && std::isfinite(rrow[r]);
        uint16_t* blk = &frags[(r >> 5) * ks * 2 * 512];
        for (size_t c = 0; c < D; ++c) {
            const size_t at = ((c >> 4) * 2 * 64 + ((c >> 3) & 1) * 32 + (r & 31)) * 8 + (c & 7);
            blk[at] = hl[c];
            blk[at + 512] = hl[dpad + c];
        }
    }
    finite = finite && std::isfinite(m.a) && std::isfinite(m.a_hi) && std::isfinite(m.a_lo) && std::isfinite(m.a_res) &&
             std::isfinite(m.r_abs);
    if (!finite) {
        f.frags.release();
        f.rrow.release();
        return;
    }
    try {
        f.frags.ensure(frags.size() * 2);
        f.rrow.ensure(rrow.size() * 4);
        hip_check(hipMemcpyAsync(f.frags.ptr(), frags.data(), frags.size() * 2, hipMemcpyHostToDevice, stream_), "diverg fragments H2D");
        hip_check(hipMemcpyAsync(f.rrow.ptr(), rrow.data(), rrow.size() * 4, hipMemcpyHostToDevice, stream_), "diverg row constants H2D");
        hip_check(hipStreamSynchronize(stream_), "diverg fast copy");
        f.max = m;
        f.have = true;
    } catch (const EngineError& e) {
        if (e.code != Err::OutOfMemory) throw;
        (void)hipGetLastError();
        f.frags.release();
        f.rrow.release();
    }
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
    const size_t rbytes = 2 * nq * k * 4 + nq * 4;
    pinned(std::max(diverg_pack_bytes(nq, D), rbytes));   // (one size for the whole call: a growth keeps nothing)
    const ResultBlock out = result_block(nq, k);
    const bool opted = diverg_fast_enabled();
    const int form = diverg_fast_form(space_), kk = (int)std::min<size_t>(k, INT_MAX);
    // (an index finalized with the path off: the first batch that finds it on and could take it makes the copy)
    if (opted && !dfast_.tried && dvf::plan(form, (int)d_n_, (int)D, (int)nq, kk, true).use) make_diverg_fast_copy();
    // (js_have: a Jensen-Shannon index; its plan takes any D and needs no copy of the rows)
    const bool js = dfast_.js_have;
    const dvf::Plan fp = js ? djs::plan((int)d_n_, (int)D, (int)nq, kk, true) : dvf::plan(form, (int)d_n_, (int)D, (int)nq, kk, dfast_.have);
    // on by default: measured, the path beats the exact scan three times over for KL and Jensen-Shannon and five for
    // Itakura-Saito
    if (!fp.use || !opted) {
        diverg_scan_batch(queries, nq, D, k, out);
        fetch_results(nq, k, "diverg knn", ids, dists, cnt);
        last_path = 0;
        return;
    }
    // large batches of the Bregman "fast" spaces: bf16 MFMA filter, exact re-rank, proof (diverg_mfma_kernels.hip)
    DivergFast& f = dfast_;
    const DivergQueries q = upload_diverg_queries(queries, nq, D);
    const size_t dpad = 16 * (size_t)fp.ksteps, lists = (size_t)fp.qpad * fp.nsplit;
    DivergFastWs ws{};
    // (the queries' operand as the scan reads it: bf16 hi | lo, or for Jensen-Shannon the clamped value plane)
    ws.qsplit = static_cast<uint16_t*>(f.ws_qsplit.ensure(js ? (size_t)diverg_groups((int)D) * fp.qpad * 16 : (size_t)fp.qpad * 2 * dpad * 2));
    ws.qclamp = reinterpret_cast<float*>(ws.qsplit);
    ws.ce = static_cast<double*>(f.ws_ce.ensure((size_t)fp.qpad * 16));
    ws.cand = static_cast<unsigned long long*>(f.ws_cand.ensure(lists * dvf::kKeep * 8));
    ws.cand_cnt = static_cast<int*>(f.ws_cnt.ensure(lists * 4));
    ws.flags = static_cast<int*>(f.ws_flags.ensure((size_t)fp.ngroups * 4));
    const DivergFastRows copy{f.frags.as<uint16_t>(), f.rrow.as<float>(), f.max};
    prof_begin(stream_);
    if (js)
        hip_check(launch_diverg_js_fast(space_, fp, (int)nq, (int)k, diverg_rows(), f.js_r32.as<float>(), f.js_max, q, ws,
                                        d_ids_.as<int32_t>(), out.dists, out.ids, out.cnt, stream_),
                  "diverg js fast scan");
    else
        hip_check(launch_diverg_fast(space_, fp, (int)nq, (int)k, diverg_rows(), copy, q, ws, d_ids_.as<int32_t>(), out.dists,
                                     out.ids, out.cnt, stream_),
                  "diverg fast scan");
    prof_end(stream_);
    std::vector<int> flags((size_t)fp.ngroups);
    hip_check(hipMemcpyAsync(flags.data(), ws.flags, flags.size() * 4, hipMemcpyDeviceToHost, stream_), "diverg flags D2H");
    hip_check(hipStreamSynchronize(stream_), "diverg fast scan");
    last_path = js ? 16 : 14;
    fast_flags_ = ws.flags;
    fast_nqt_ = fp.ngroups;
    fast_has_precise_ = false;
    // groups without a proof: their queries again, as one compacted batch through the exact scan
    std::vector<size_t> redo;
    for (size_t q1 = 0; q1 < nq; ++q1)
        if (flags[q1 / dvf::kGroup]) redo.push_back(q1);
    std::vector<char> sub_host;
    if (!redo.empty()) {
        const size_t m = redo.size();
        std::vector<float> sub_q(m * D);
        for (size_t i = 0; i < m; ++i) std::memcpy(&sub_q[i * D], queries + redo[i] * D, D * 4);
        int32_t* sub_ids = static_cast<int32_t*>(f.ws_sub.ensure(2 * m * k * 4 + m * 4));
        const ResultBlock sub{sub_ids, reinterpret_cast<float*>(sub_ids + m * k), sub_ids + 2 * m * k};
        diverg_scan_batch(sub_q.data(), m, D, k, sub);
        sub_host.resize(2 * m * k * 4 + m * 4);
        hip_check(hipMemcpyAsync(sub_host.data(), sub_ids, sub_host.size(), hipMemcpyDeviceToHost, stream_), "diverg redo D2H");
    }
    fetch_results(nq, k, "diverg knn", ids, dists, cnt);
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

size_t Engine::diverg_pack_bytes(size_t nq, size_t D) const {
    // a tile of the scan reads kDivergTileQ queries from its first one: the pack is that much longer than the batch
    const size_t plane = (size_t)diverg_groups((int)D) * (nq + kDivergTileQ) * 4;
    return (space_ == SP_ITAKURASAITO ? 3 : 2) * plane * 4;
}

// the batch's queries as the kernels read them: packed in the pinned block (sized by the caller), copied to ws_bq_
DivergQueries Engine::upload_diverg_queries(const float* queries, size_t nq, size_t D) {
    const size_t stride = nq + kDivergTileQ, plane = (size_t)diverg_groups((int)D) * stride * 4;
    const bool with_inv = space_ == SP_ITAKURASAITO;
    const size_t qbytes = diverg_pack_bytes(nq, D);
    float* hp = static_cast<float*>(pinned_.ptr());
    pack_queries(space_, queries, nq, D, stride, hp, hp + plane, with_inv ? hp + 2 * plane : nullptr);
    ws_bq_.ensure(qbytes);
    hip_check(hipMemcpyAsync(ws_bq_.ptr(), hp, qbytes, hipMemcpyHostToDevice, stream_), "diverg queries H2D");
    const float* dq = ws_bq_.as<float>();
    return DivergQueries{dq, dq + plane, with_inv ? dq + 2 * plane : nullptr, (int)stride};
}

// the exact scan of a batch into `out` (enqueued; the pinned block holds the batch's pack until the copy has left it)
void Engine::diverg_scan_batch(const float* queries, size_t nq, size_t D, size_t k, const ResultBlock& out) {
    const DivergQueries q = upload_diverg_queries(queries, nq, D);
    const DivergRows rows = diverg_rows();
    scan_slices(nq, k, kDivergTileQ, out, [&](const ScanPlan& p, size_t q0, float* split_d, int32_t* split_pos) {
        hip_check(launch_diverg_knn(space_, p, rows, q, (int)q0, split_d, split_pos, stream_), "diverg scan");
    });
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
