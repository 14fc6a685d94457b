// Dense brute force on the engine (float rows and uint8 SIFT rows): what finalize prepares in HBM beside the rows
// (BruteDense: selection copies, error bounds, the fast paths' tiles) and the k-NN batch over kernels/bf_kernels.hip.
// A batch takes one of: the big-k scan (k > BF_MAX_K), a fast path (large index, large batch), the adaptive path.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "engine.hpp"
#include "l1_quant.hpp"

namespace gfxknn {

void BruteDense::release() {
    have_bf16 = false;
    have_l1 = false;
    l1_u8.release();
    l1_cols.release();
    bf_hi.release();
    bf_lo.release();
    f16_hi.release();
    auxp.release();
    auxp16.release();
}

size_t BruteDense::bytes() const {
    size_t total = 0;
    for (const DevBuf* b : {&rows_i8, &auxh, &rows_sel, &mean, &bf_hi, &bf_lo, &auxp, &f16_hi, &auxp16, &l1_u8, &l1_cols}) total += b->bytes();
    return total;
}

BfF32Tiles BruteDense::tiles(int dp, bool augmented) const {
    BfF32Tiles t{};
    t.hi = bf_hi.ptr();
    t.lo = bf_lo.ptr();
    t.auxp = auxp.as<float>();
    t.h16 = f16_hi.ptr();
    t.auxp16 = auxp16.as<float>();
    t.scale = f16_scale;
    t.bres16 = bres16;
    t.dp = dp;
    t.bmax = augmented ? bmax_c : bmax;
    t.bres = augmented ? bres_c : bres;
    return t;
}

// bm[0] largest row norm, bm[1] largest bf16 residual; chooses the fp16 scale of the one-product scan from the largest
// |element| (a power of two that puts it into [2^13, 2^14): a factor 4 of headroom below fp16's 65504 for the queries) and
// measures the rows' largest fp16 residual at that scale (f16_scale, bres16)
void Engine::measure_rows_f16(const float* rows, size_t n, int ld, int dim, bool relative, float* bm) {
    DevBuf d_bm;
    d_bm.ensure(16);
    hip_check(launch_row_maxnorm(rows, (int)n, ld, dim, relative, d_bm.as<float>(), stream_), "row norms");
    hip_check(hipMemcpyAsync(bm, d_bm.ptr(), 16, hipMemcpyDeviceToHost, stream_), "bmax");
    hip_check(hipStreamSynchronize(stream_), "row norms");
    brute_.f16_scale = 1.f;
    if (bm[2] > 0.f && std::isfinite(bm[2])) {
        // (|exponent| <= 40: scale^2, the unit of the scan's scores, must stay a float; rows smaller than 2^-27 simply lose
        //  fp16 precision, which the measured residual reports)
        const int e = std::max(-40, std::min(40, 13 - (int)std::floor(std::log2(bm[2]))));
        brute_.f16_scale = std::ldexp(1.f, e);
    }
    float bm2[4] = {0.f, 0.f, 0.f, 0.f};
    hip_check(launch_row_maxnorm(rows, (int)n, ld, dim, relative, d_bm.as<float>(), stream_, brute_.f16_scale), "row residuals");
    hip_check(hipMemcpyAsync(bm2, d_bm.ptr(), 16, hipMemcpyDeviceToHost, stream_), "bres16");
    hip_check(hipStreamSynchronize(stream_), "row residuals");
    brute_.bres16 = bm2[3];
    brute_.f16_scale_q = brute_.f16_scale;
}

// The resident side of the f32 fast path for src.n_pad rows of dp columns: bf16 hi / lo tiles (the split-product scan, rows
// of up to 128 dimensions only), fp16 tiles of the rows times f16_scale (the one-product scan) and both start values.
void Engine::make_fast_tiles(const BfSplitSrc& src, int dp, const float* aux, float aux_pad, float aux16_mul) {
    BruteDense& b = brute_;
    const size_t n_pad = (size_t)src.n_pad;
    if (dp == 128) {
        b.bf_hi.ensure(n_pad * dp * 2);
        b.bf_lo.ensure(n_pad * 128 * 2);
    }
    b.f16_hi.ensure(n_pad * dp * 2);
    b.auxp.ensure(n_pad * 4);
    b.auxp16.ensure(n_pad * 4);
    hip_check(launch_split_bf16(src, aux, aux_pad, aux16_mul, b.tiles(dp, false), stream_), "split rows");
    b.have_bf16 = true;
}

// The resident side of the l1 fast path (l1_quant.hpp): column ranges -> common step -> byte copy in the scan's layout and
// the columns' largest residuals.  Declined data (a non-finite element, no usable step) and a failed allocation leave the
// index on the adaptive kernel.
void Engine::make_l1_copy() {
    BruteDense& b = brute_;
    const size_t n = d_n_;  // the rows upload_rows made resident (the live ones of an index with deleted rows)
    const size_t dim = dim_, ld = (size_t)ldb_;
    try {
        DevBuf d_range, d_rmax;
        d_range.ensure((2 * ld + 1) * 4);
        hip_check(launch_l1_col_range(d_rows_.as<float>(), (int)n, ldb_, (int)dim, d_range.as<uint32_t>(), stream_), "l1 column ranges");
        std::vector<uint32_t> range(2 * ld + 1);
        hip_check(hipMemcpyAsync(range.data(), d_range.ptr(), range.size() * 4, hipMemcpyDeviceToHost, stream_), "l1 column ranges");
        hip_check(hipStreamSynchronize(stream_), "l1 column ranges");
        if (range[2 * ld] != 0) return;   // a non-finite element
        auto from_ord = [](uint32_t o) {
            const uint32_t bits = o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu);
            float f;
            memcpy(&f, &bits, 4);
            return f;
        };
        std::vector<float> cols(3 * dim, 0.f);   // lo, hi, rmax
        for (size_t c = 0; c < dim; ++c) {
            cols[c] = from_ord(range[c]);
            cols[dim + c] = from_ord(range[ld + c]);
        }
        bool ok = false;
        const double step = l1q::step_of(l1q::max_range(cols.data(), cols.data() + dim, dim), &ok);
        if (!ok) return;
        const size_t d4 = (dim + 3) / 4;
        b.l1_cols.ensure(cols.size() * 4);
        b.l1_u8.ensure((size_t)bf_l1_rows_padded((int)n) * d4 * 4);
        d_rmax.ensure(dim * 4);
        hip_check(hipMemcpyAsync(b.l1_cols.ptr(), cols.data(), cols.size() * 4, hipMemcpyHostToDevice, stream_), "l1 columns");
        hip_check(launch_l1_quantise_rows(d_rows_.as<float>(), (int)n, ldb_, (int)dim, b.l1_cols.as<float>(), step,
                                          b.l1_u8.as<uint32_t>(), d_rmax.as<uint32_t>(), stream_),
                  "l1 byte copy");
        hip_check(hipMemcpyAsync(b.l1_cols.as<float>() + 2 * dim, d_rmax.ptr(), dim * 4, hipMemcpyDeviceToDevice, stream_), "l1 residuals");
        hip_check(hipStreamSynchronize(stream_), "l1 byte copy");   // (`cols` and d_rmax go out of scope)
        b.l1_step = step;
        b.have_l1 = true;
    } catch (const EngineError& e) {
        if (e.code != Err::OutOfMemory) throw;
        (void)hipGetLastError();
        b.l1_u8.release();
        b.l1_cols.release();
    }
}

// The brute-force branch of finalize(): the rows are in HBM (upload_rows)
void Engine::prepare_brute() {
    BruteDense& b = brute_;
    const size_t n = d_n_;  // the rows upload_rows made resident (the live ones of an index with deleted rows)
    if (is_u8()) {
        const size_t n_pad = (size_t)bf_u8_rows_padded((int)n);
        d_aux_.ensure(n_pad * 4);
        b.rows_i8.ensure(n_pad * 128);
        b.auxh.ensure(n_pad * 4);
        hip_check(launch_prepare_u8(d_rows_.as<uint8_t>(), (int)n, b.rows_i8.as<uint8_t>(), d_aux_.as<int32_t>(),
                                    b.auxh.as<int32_t>(), stream_),
                  "prepare u8 rows");
        hip_check(hipStreamSynchronize(stream_), "finalize");
        return;
    }
    const bool cosine = space_ == SP_COSINE || space_ == SP_ANGULAR;
    d_aux_.ensure(std::max<size_t>(n, 1) * 4);
    const float* sel_rows = d_rows_.as<float>();
    b.centred = false;
    b.rows_sel.release();
    if ((space_ == SP_L2 || cosine) && n > 0) {
        // L2 is translation invariant, the Q.B^T score q.b - |b|^2/2 is not: its f32 rounding error grows with
        // |q||b|, i.e. with a common offset of the data, and can exceed the gaps between neighbours (the
        // reference's direct sum (a-b)^2, distcomp_lp.cc:304-365, has no such term).  When the column mean
        // is not small against the spread, SELECTION runs on rows - mean and queries - mean; the exact
        // re-rank keeps using the original rows.  Cosine / angular: same centred copy, and the score is
        // rebuilt as 1 - cos = (|q'-b'|^2 - (|q|-|b|)^2) / (2|q||b|) (bf_kernels.hip, BF_COSC).
        std::vector<double> st((size_t)ldb_ + 1);
        DevBuf d_stats;
        d_stats.ensure(st.size() * 8);
        hip_check(launch_col_stats(d_rows_.as<float>(), (int)n, ldb_, (int)dim_, d_stats.as<double>(), stream_), "column stats");
        hip_check(hipMemcpyAsync(st.data(), d_stats.ptr(), st.size() * 8, hipMemcpyDeviceToHost, stream_), "stats D2H");
        hip_check(hipStreamSynchronize(stream_), "column stats");
        double mu2 = 0;
        std::vector<float> mean((size_t)ldb_, 0.f);
        for (size_t c = 0; c < dim_; ++c) {
            const double m = st[c] / (double)n;
            mean[c] = (float)m;
            mu2 += m * m;
        }
        const double spread2 = std::max(0.0, st[(size_t)ldb_] / (double)n - mu2);
        b.cosc_spread2 = spread2;
        bool centre = mu2 > 0.0625 * spread2;
        if (const char* env = getenv("NMSLIB_GPU_CENTER")) centre = atoi(env) != 0;
        if (centre) {
            b.mean.ensure((size_t)ldb_ * 4);
            b.rows_sel.ensure(n * (size_t)ldb_ * 4);
            hip_check(hipMemcpyAsync(b.mean.ptr(), mean.data(), (size_t)ldb_ * 4, hipMemcpyHostToDevice, stream_), "mean");
            hip_check(launch_center_rows(d_rows_.as<float>(), b.mean.as<float>(), (int)n, (int)n, ldb_, (int)dim_,
                                         b.rows_sel.as<float>(), stream_),
                      "centre rows");
            hip_check(hipStreamSynchronize(stream_), "centre rows");  // `mean` is read by the copy above
            sel_rows = b.rows_sel.as<float>();
            b.centred = true;
            b.mu_norm = 0;
            for (size_t c = 0; c < dim_; ++c) b.mu_norm += (double)mean[c] * (double)mean[c];
            b.mu_norm = std::sqrt(b.mu_norm);
        }
    }
    if (b.centred && space_ != SP_L2) {
        d_aux_.ensure(std::max<size_t>(n, 1) * 12);
        hip_check(launch_row_aux_cosc(d_rows_.as<float>(), sel_rows, (int)n, ldb_, (int)dim_, b.mu_norm, d_aux_.as<float>(),
                                      stream_),
                  "row aux");
    } else {
        hip_check(launch_row_aux_f32(sel_rows, (int)n, ldb_, (int)dim_, space_, d_aux_.as<float>(), stream_), "row aux");
    }
    // largest norm (and bf16 rounding residual) of the selection rows: the error bounds of the selection scores
    // (proofs in bf_rerank_kernel and bf_rerank_f32_list_kernel)
    {
        float bm[4] = {0.f, 0.f, 0.f, 0.f};
        measure_rows_f16(sel_rows, n, ldb_, (int)dim_, cosine, bm);
        b.bmax = bm[0];
        b.bres = bm[1];
    }
    // fast path (large batches): tiles of the selection rows + padded aux
    b.release();
    const bool fast_space = space_ == SP_L2 || space_ == SP_NEGDOT || (cosine && !b.centred);
    const int n_pad = bf_f32_rows_padded((int)n);
    if (cosine && b.centred && dim_ + 3 <= 1024 && n >= 65536) {
        // centred cosine / angular (round 3): the score -(1 - cos)|q| as an inner product of rows and queries with
        // three more columns (bf_kernels.hip, row_aug_cosc_kernel); tiles of those rows, scanned in the inner-product
        // mode.  A zero-norm row has no score of this form: the index then stays on the adaptive kernel.
        const BfF32Fast f0 = bf_f32_fast_plan((int)n, (int)dim_, 1024, 10, space_, true);
        if (f0.use) {
            const size_t dp = (size_t)f0.dp;
            DevBuf d_aug, d_flag;
            d_aug.ensure(n * dp * 4);
            d_flag.ensure(16);
            hip_check(hipMemsetAsync(d_flag.ptr(), 0, 16, stream_), "clear");
            // (the two constant columns balanced at the typical (|b'|^2 - db^2) / 2 <= spread^2 / 2)
            b.cosc_lambda = (float)std::sqrt(std::max(0.5 * b.cosc_spread2, 1e-30));
            hip_check(launch_row_aug_cosc(d_rows_.as<float>(), sel_rows, (int)n, ldb_, (int)dim_, b.mu_norm, b.cosc_lambda,
                                          d_aug.as<float>(), (int)dp, d_flag.as<int>(), stream_),
                      "augmented rows");
            int fl[1] = {0};
            hip_check(hipMemcpyAsync(fl, d_flag.ptr(), 4, hipMemcpyDeviceToHost, stream_), "flags");
            hip_check(hipStreamSynchronize(stream_), "augmented rows");
            if (fl[0] == 0) {
                float bm[4] = {0.f, 0.f, 0.f, 0.f};
                measure_rows_f16(d_aug.as<float>(), n, (int)dp, (int)dim_ + 3, false, bm);   // (sets f16_scale, bres16)
                // (the augmented rows are divided by their norm ~ |mean|, the augmented queries are not)
                if (b.mu_norm > 0) {
                    const int eq = std::max(-40, std::min(40, (int)std::lround(std::log2((double)b.f16_scale) - std::log2(b.mu_norm))));
                    b.f16_scale_q = std::ldexp(1.f, eq);
                }
                b.bmax_c = bm[0];
                b.bres_c = bm[1];
                make_fast_tiles({d_aug.as<float>(), (int)n, n_pad, (int)dp, (int)dim_ + 3}, (int)dp, nullptr, 0.f, 1.f);
                hip_check(hipStreamSynchronize(stream_), "split rows");   // (d_aug goes out of scope)
            }
        }
    }
    if (fast_space && dim_ <= 1024 && n >= 65536) {
        // (rows up to 128 dimensions: hi and lo tiles; longer rows, round 3: tiles of 128 * kch columns for the K-chunked
        //  one-product scan -- the plan's kch, which depends on the dimension only.  Start values of the fp16 tiles: in
        //  units of scale^2 for l2, the plain 1/|b| for cosine)
        const BfF32Fast f0 = bf_f32_fast_plan((int)n, (int)dim_, 1024, 10, space_, b.centred);
        make_fast_tiles({sel_rows, (int)n, n_pad, ldb_, (int)dim_}, f0.use ? f0.dp : 128,
                        space_ == SP_NEGDOT ? nullptr : d_aux_.as<float>(), space_ == SP_L2 ? -INFINITY : 0.f,
                        space_ == SP_L2 ? b.f16_scale * b.f16_scale : 1.f);
    }
    if (space_ == SP_L1 && n >= 65536 && dim_ <= (size_t)BF_L1_MAX_DIM) make_l1_copy();
    hip_check(hipStreamSynchronize(stream_), "finalize");
}

void Engine::knn_brute(const void* d_queries, size_t nq, size_t k, int32_t* d_ids, float* d_dists, int32_t* d_cnt,
                       hipStream_t stream) {
    BruteDense& b = brute_;
    have_counters_ = false;
    const int dim_eff = d_n_ ? (int)dim_ : 1;
    const BfOut out{d_ids_.as<int32_t>(), d_ids, d_dists, d_cnt};
    if (k > (size_t)BF_MAX_K) {
        // beyond the selection kernels' capacity: per query one pass with the reference formula + one stable radix sort
        const int ld = is_u8() ? 128 : ldb_;
        const int elem = is_u8() ? 1 : 4;
        const size_t n = d_n_;
        ws_qpad_.ensure(std::max<size_t>(nq, 1) * ld * elem);
        hip_check(launch_pad_rows(d_queries, (int)nq, dim_eff, ws_qpad_.ptr(), (int)nq, ld, elem, stream), "pad queries");
        BfBigkWs ws{};
        ws.dist = static_cast<float*>(ws_rdist_.ensure(std::max<size_t>(n, 1) * 4));
        ws.keys = static_cast<uint32_t*>(ws_bigk_.ensure(std::max<size_t>(n, 1) * 16));
        ws.temp_bytes = bf_bigk_temp_bytes((int)n);
        ws.temp = ws_bigk_tmp_.ensure(ws.temp_bytes);
        hip_check(launch_bf_bigk(space_, d_rows_.ptr(), ld, (int)n, dim_eff, ws_qpad_.ptr(), (size_t)ld * elem, (int)nq, (int)k,
                                 ws, out, stream),
                  "bf_bigk");
        last_path = 5;
        return;
    }
    // the blocks of a fast path's workspace, each grown to what the plan asks for
    auto fast_ws = [&](const BfFastWsBytes& need) {
        BfFastWs ws{};
        ws.top8 = b.ws_top8.ensure(need.top8);
        ws.thr = b.ws_thr.ensure(need.thr);
        ws.list = static_cast<uint32_t*>(b.ws_list.ensure(need.list));
        ws.list_cnt = static_cast<int*>(b.ws_listcnt.ensure(need.list_cnt));
        ws.fb.cand = static_cast<unsigned long long*>(ws_cand_.ensure(need.cand));
        ws.fb.cnt = static_cast<int*>(ws_cnt_.ensure(need.cnt));
        if (need.flags_fb) ws.flags_fb = static_cast<int*>(b.ws_flags.ensure(need.flags_fb));
        if (need.queries) ws.queries = b.ws_f32_q.ensure(need.queries);
        return ws;
    };
    if (is_u8()) {
        // large batches: thresholds fixed by a sample pass, then one streaming scan (bf_kernels.hip, bf_scan_u8_kernel)
        const BfU8Fast f = bf_u8_fast_plan((int)d_n_, (int)nq, (int)k);
        if (f.use) {
            // (padding happens inside the fast path's one preparation kernel)
            ws_qpad_.ensure((size_t)f.qpad * 128);
            const BfFastWs ws = fast_ws(bf_fast_ws_bytes(f));
            const BfU8Rows rows{d_rows_.as<uint8_t>(), b.rows_i8.as<uint8_t>(), d_aux_.as<int32_t>(), b.auxh.as<int32_t>(), (int)d_n_};
            hip_check(launch_bf_u8_fast(f, (int)nq, (int)k, rows, static_cast<const uint8_t*>(d_queries), ws_qpad_.as<uint8_t>(),
                                        ws, out, prof_pair(), stream),
                      "bf_u8_fast");
            last_path = 3;
            fast_flags_ = ws.tile_fail(f);
            fast_nqt_ = f.nqt;
            fast_has_precise_ = false;
            return;
        }
    }
    // the float rows and queries as the launchers take them (row stride: an empty index has none of its own)
    const BfF32Rows rows{d_rows_.as<float>(), b.centred ? b.rows_sel.as<float>() : d_rows_.as<float>(), d_aux_.as<float>(),
                         (int)d_n_, dim_eff, d_n_ ? ldb_ : f32_row_stride(dim_eff), b.bmax};
    BfF32Queries q{};
    if (!is_u8() && b.have_bf16) {
        // large batches: bf16 / fp16 MFMA selection with sample-fixed thresholds (bf_scan_f32_kernel, bf_scan_bf16_kernel)
        const BfF32Fast f = bf_f32_fast_plan((int)d_n_, dim_eff, (int)nq, (int)k, space_, b.centred);
        if (f.use) {
            const int ldb = ldb_;
            q.padded = static_cast<float*>(ws_qpad_.ensure((size_t)f.qpad * ldb * 4));
            q.sel = q.padded;
            q.scale_q = b.f16_scale_q;
            if (b.centred) {
                hip_check(launch_pad_rows(d_queries, (int)nq, dim_eff, q.padded, f.qpad, ldb, 4, stream), "pad queries");
                ws_qsel_.ensure((size_t)f.qpad * ldb * 4);
                hip_check(launch_center_rows(q.padded, b.mean.as<float>(), f.qpad, (int)nq, ldb, dim_eff, ws_qsel_.as<float>(),
                                             stream),
                          "centre queries");
                q.sel = ws_qsel_.as<float>();
            } else {
                q.raw = static_cast<const float*>(d_queries);   // (padding happens inside the fast path's one preparation kernel)
            }
            if (f.cosc) {   // centred cosine / angular: the augmented queries (query_aug_cosc_kernel) are what the scans see
                ws_qaux_.ensure((size_t)f.qpad * 16);
                b.ws_qaug.ensure((size_t)f.qpad * f.dp * 4);
                q.centred = ws_qsel_.as<float>();
                q.qaux_cosc = ws_qaux_.as<float>();
                hip_check(launch_query_aux_cosc(q.padded, q.centred, f.qpad, ldb, dim_eff, b.mu_norm, ws_qaux_.as<float>(), stream),
                          "query aux");
                hip_check(launch_query_aug_cosc(q.centred, q.qaux_cosc, (int)nq, f.qpad, ldb, dim_eff, b.cosc_lambda,
                                                b.ws_qaug.as<float>(), f.dp, stream),
                          "augmented queries");
                q.sel = b.ws_qaug.as<float>();
                q.sel_ld = f.dp;
            }
            const BfFastWs ws = fast_ws(bf_fast_ws_bytes(f));
            hip_check(launch_bf_f32_fast(f, space_, (int)nq, (int)k, rows, b.tiles(f.dp, f.cosc), q, ws, out, prof_pair(), stream),
                      "bf_f32_fast");
            last_path = 1;
            fast_flags_ = ws.tile_fail(f);
            fast_nqt_ = f.nqt;
            fast_has_precise_ = true;
            return;
        }
    }
    if (space_ == SP_L1 && b.have_l1) {
        // large batches: v_sad_u8 filter over the byte copy, exact re-rank, proof (bf_l1_kernels.hip)
        const char* env = getenv("NMSLIB_GPU_L1_FAST");
        const BfL1Fast f = bf_l1_fast_plan((int)d_n_, dim_eff, (int)nq, (int)k);
        if (f.use && !(env && atoi(env) == 0)) {
            ws_qpad_.ensure((size_t)f.qpad * ldb_ * 4);
            BfL1Ws ws{};
            ws.qt = static_cast<uint32_t*>(b.ws_l1_qt.ensure((size_t)f.d4 * f.qpad * 4));
            ws.xe = static_cast<double*>(b.ws_l1_xe.ensure((size_t)f.qpad * 16));
            ws.cand.cand = static_cast<unsigned long long*>(b.ws_l1_cand.ensure((size_t)f.qpad * f.nsplit * f.kprime * 8));
            ws.cand.cnt = static_cast<int*>(b.ws_l1_cnt.ensure((size_t)f.qpad * f.nsplit * 4));
            ws.flags = static_cast<int*>(b.ws_flags.ensure((size_t)f.nqt * 4 + 64));
            ws.fb.cand = static_cast<unsigned long long*>(ws_cand_.ensure(bf_cand_elems(f.fallback) * 8));
            ws.fb.cnt = static_cast<int*>(ws_cnt_.ensure(bf_cnt_elems(f.fallback) * 4));
            const float* cols = b.l1_cols.as<float>();
            const BfL1Rows copy{b.l1_u8.as<uint32_t>(), cols, cols + dim_, cols + 2 * dim_, b.l1_step};
            hip_check(launch_bf_l1_fast(f, (int)nq, (int)k, rows, copy, static_cast<const float*>(d_queries), ws_qpad_.as<float>(),
                                        ws, out, prof_pair(), stream),
                      "bf_l1_fast");
            last_path = 6;
            fast_flags_ = ws.flags;
            fast_nqt_ = f.nqt;
            fast_has_precise_ = false;
            return;
        }
    }
    last_path = is_u8() ? 2 : 0;
    BfPlan p = bf_make_plan((int)d_n_, dim_eff, (int)nq, (int)k, is_u8());
    if (d_n_ == 0) p.ldb = is_u8() ? 128 : f32_row_stride(dim_eff);
    const int elem = is_u8() ? 1 : 4;
    ws_qpad_.ensure((size_t)p.qpad * p.ldb * elem);
    const BfCand c{static_cast<unsigned long long*>(ws_cand_.ensure(bf_cand_elems(p) * 8)),
                   static_cast<int*>(ws_cnt_.ensure(bf_cnt_elems(p) * 4))};
    hip_check(launch_pad_rows(d_queries, (int)nq, dim_eff, ws_qpad_.ptr(), p.qpad, p.ldb, elem, stream), "pad queries");
    q.padded = ws_qpad_.as<float>();
    q.sel = q.padded;
    if (b.centred) {
        ws_qsel_.ensure((size_t)p.qpad * p.ldb * 4);
        hip_check(launch_center_rows(q.padded, b.mean.as<float>(), p.qpad, (int)nq, p.ldb, dim_eff, ws_qsel_.as<float>(), stream),
                  "centre queries");
        q.sel = ws_qsel_.as<float>();
        if (space_ != SP_L2) {
            ws_qaux_.ensure((size_t)p.qpad * 16);
            hip_check(launch_query_aux_cosc(q.padded, q.sel, p.qpad, p.ldb, dim_eff, b.mu_norm, ws_qaux_.as<float>(), stream),
                      "query aux");
            q.qaux_cosc = ws_qaux_.as<float>();
        }
    }
    prof_begin(stream);
    if (is_u8()) {
        hip_check(launch_bf_select_u8(p, b.rows_i8.as<uint8_t>(), d_aux_.as<int32_t>(), ws_qpad_.as<uint8_t>(), c, BfGate{}, stream),
                  "bf_select_u8");
    } else if (space_ == SP_L1 || space_ == SP_LINF) {
        hip_check(launch_bf_select_direct_f32(p, space_, rows.orig, q.padded, c, BfGate{}, stream), "bf_select_direct");
    } else {
        // selection + re-rank in one chain (l2: verified, with the exact tail for tiles of near-duplicates)
        b.ws_flags.ensure((size_t)p.nqt * 4 + 64);
        hip_check(launch_bf_adaptive_f32(p, space_, (int)k, rows, q, c, b.ws_flags.as<int>(), BfGate{}, out, stream),
                  "bf_adaptive_f32");
        prof_end(stream);
        return;
    }
    prof_end(stream);
    hip_check(launch_bf_rerank(p, space_, dim_eff, (int)k, d_rows_.ptr(), ws_qpad_.ptr(), c, BfGate{}, BfVerify{}, out, stream),
              "bf_rerank");
}

}  // namespace gfxknn
