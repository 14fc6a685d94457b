// String rows on the engine (data type 3): the host store, its copy in HBM, and the k-NN batch / range / pair
// entries over kernels/string_kernels.hip.  A string index runs on one device: an exact scan (brute_force,
// seq_search) or an HNSW graph built on the host and searched on the GPU.
//   leven      : CSR of the strings' bytes (StringSpace::CreateObjFromStr keeps the bytes as they are).
//   bit_hamming: the text is parsed as the reference's ReadBitMaskVect does (include/space/space_bit_vector.h:
//                156-200) and packed into W uint32 words per row; the bit count is fixed by the first row.
#include <algorithm>
#include <cctype>
#include <cerrno>
#include <chrono>
#include <climits>
#include <cstdlib>
#include <cstring>

#include "engine.hpp"

namespace gfxknn {

namespace {

bool is_space(char c) { return std::isspace(static_cast<unsigned char>(c)) != 0; }

// The reference parses a C string: a NUL ends the text.
std::string c_text(const char* s, size_t len) { return std::string(s, strnlen(s, len)); }

// Object::extractLabel (include/object.h:118-150): a leading "label:<int><whitespace...>" is removed; a prefix that
// is not followed by whitespace, or whose label is not an integer, is an error.
bool strip_label(std::string& line) {
    static const std::string prefix = "label:";
    if (line.size() > prefix.size() + 1 && line.compare(0, prefix.size(), prefix) == 0) {
        size_t p = prefix.size();
        while (p < line.size() && !is_space(line[p])) ++p;
        if (p == line.size()) return false;
        const std::string num = line.substr(prefix.size(), p - prefix.size());
        char* end = nullptr;
        errno = 0;
        const long v = std::strtol(num.c_str(), &end, 10);
        // a stream extraction into an int: leading whitespace is impossible here, the whole token must be consumed
        if (num.empty() || end != num.c_str() + num.size() || errno == ERANGE || v < INT_MIN || v > INT_MAX)
            return false;
        while (p < line.size() && is_space(line[p])) ++p;
        line = line.substr(p);
    }
    return true;
}

}  // namespace

// ReadBitMaskVect: label, then ',' and ':' read as blanks (ReplaceSomePunct), then integers read with strtol until
// one fails to parse (ReadVecDataEfficiently<int>: the rest of the line is ignored, an out-of-range value is an
// error); only 0 and 1 are allowed.  Binarize packs value i into bit i % 32 of word i / 32.
bool Engine::parse_bits(const char* s, size_t len, std::vector<uint32_t>& words, size_t& bits) {
    std::string line = c_text(s, len);
    if (!strip_label(line)) return false;
    for (char& c : line)
        if (c == ',' || c == ':') c = ' ';
    std::vector<uint8_t> v;
    const char* p = line.c_str();
    for (;;) {
        char* end = nullptr;
        errno = 0;
        const long x = std::strtol(p, &end, 10);
        if (end == p) break;
        if (errno == ERANGE || x < INT_MIN || x > INT_MAX) return false;
        if (x != 0 && x != 1) return false;
        v.push_back((uint8_t)x);
        p = end;
    }
    bits = v.size();
    words.assign((bits + 31) / 32, 0u);
    for (size_t i = 0; i < bits; ++i)
        if (v[i]) words[i / 32] |= 1u << (i % 32);
    return true;
}

void Engine::add_strings(const char* const* strs, const size_t* lens, size_t count, const int32_t* ids) {
    if (!str_space_) throw EngineError(Err::SpaceIncompatible, "Not string space");
    if (ids_.size() + count > (size_t)INT32_MAX) throw EngineError(Err::InvalidArgument, "too many rows for one index");
    // the whole batch is checked before any row is stored
    if (space_ == SP_LEVEN) {
        size_t total = 0;
        for (size_t i = 0; i < count; ++i) {
            // the reference CHECKs datalength() > 0 when it computes a distance, and aborts
            if (lens[i] == 0) throw EngineError(Err::InvalidArgument, "leven: empty strings are not accepted");
            if (lens[i] > (size_t)INT32_MAX) throw EngineError(Err::InvalidArgument, "leven: string too long");
            total += lens[i];
        }
        st_bytes_.reserve(st_bytes_.size() + total);
        for (size_t i = 0; i < count; ++i) {
            st_bytes_.insert(st_bytes_.end(), reinterpret_cast<const uint8_t*>(strs[i]),
                             reinterpret_cast<const uint8_t*>(strs[i]) + lens[i]);
            st_ptr_.push_back((int64_t)st_bytes_.size());
            ids_.push_back(ids ? ids[i] : (int32_t)i);
        }
    } else {
        std::vector<uint32_t> packed, w;
        int64_t bits = st_bits_;
        for (size_t i = 0; i < count; ++i) {
            size_t b = 0;
            if (!parse_bits(strs[i], lens[i], w, b))
                throw EngineError(Err::Runtime, "bit_hamming: failed to parse the row (only 0 and 1 values are allowed)");
            if (b == 0) throw EngineError(Err::InvalidArgument, "bit_hamming: a row holds at least one bit");
            if (b > (size_t)INT32_MAX) throw EngineError(Err::InvalidArgument, "bit_hamming: row too long");
            if (bits >= 0 && (int64_t)b != bits)
                throw EngineError(Err::InvalidArgument, "bit_hamming: the row has " + std::to_string(b) +
                                                            " bits, the index " + std::to_string(bits));
            bits = (int64_t)b;
            packed.insert(packed.end(), w.begin(), w.end());
        }
        st_bits_ = bits;
        st_words_.insert(st_words_.end(), packed.begin(), packed.end());
        for (size_t i = 0; i < count; ++i) ids_.push_back(ids ? ids[i] : (int32_t)i);
    }
    dirty_ = true;
    graph_dirty_ = true;
}

size_t Engine::string_object_bytes(size_t pos) const {
    if (space_ == SP_LEVEN) return (size_t)(st_ptr_[pos + 1] - st_ptr_[pos]);
    return (ham_words() + 1) * 4;
}

std::string Engine::string_object(size_t pos) const {
    // Object::data(): leven the bytes; bit_hamming the packed words and the bit count as a trailing word
    if (space_ == SP_LEVEN)
        return std::string(reinterpret_cast<const char*>(st_bytes_.data()) + st_ptr_[pos],
                           (size_t)(st_ptr_[pos + 1] - st_ptr_[pos]));
    const size_t W = ham_words();
    std::string out((W + 1) * 4, '\0');
    std::memcpy(&out[0], st_words_.data() + pos * W, W * 4);
    const uint32_t nb = (uint32_t)st_bits_;
    std::memcpy(&out[W * 4], &nb, 4);
    return out;
}

void Engine::upload_strings() {
    check_device();
    const auto t0 = std::chrono::steady_clock::now();
    const size_t n = ids_.size();
    if (space_ == SP_LEVEN) {
        d_st_ptr_.ensure((n + 1) * sizeof(int64_t));
        d_st_data_.ensure(st_bytes_.size() + 4);  // the scan stages rows as dwords: the last one is read whole
        hip_check(hipMemcpyAsync(d_st_ptr_.ptr(), st_ptr_.data(), (n + 1) * 8, hipMemcpyHostToDevice, stream_),
                  "string row_ptr H2D");
        if (!st_bytes_.empty())
            hip_check(hipMemcpyAsync(d_st_data_.ptr(), st_bytes_.data(), st_bytes_.size(), hipMemcpyHostToDevice, stream_),
                      "string bytes H2D");
    } else {
        // (16-byte aligned rows for the scan's wide loads when W % 4 == 0: DevBuf allocations are)
        d_st_data_.ensure(std::max<size_t>(st_words_.size(), 1) * 4);
        if (!st_words_.empty())
            hip_check(hipMemcpyAsync(d_st_data_.ptr(), st_words_.data(), st_words_.size() * 4, hipMemcpyHostToDevice,
                                     stream_),
                      "bit rows H2D");
    }
    d_ids_.ensure(std::max<size_t>(n, 1) * sizeof(int32_t));
    if (n) hip_check(hipMemcpyAsync(d_ids_.ptr(), ids_.data(), n * 4, hipMemcpyHostToDevice, stream_), "ids H2D");
    if (method_ == Method::Hnsw) {
        ensure_graph();
        const HostGraph& g = graph_;
        d_links0_.ensure(std::max<size_t>(g.links0.size(), 1) * 4);
        d_up_off_.ensure(std::max<size_t>(n, 1) * 8);
        d_up_links_.ensure(std::max<size_t>(g.up_links.size(), 1) * 4);
        if (n) {
            hip_check(hipMemcpyAsync(d_links0_.ptr(), g.links0.data(), g.links0.size() * 4, hipMemcpyHostToDevice, stream_),
                      "links0");
            hip_check(hipMemcpyAsync(d_up_off_.ptr(), g.up_off.data(), n * 8, hipMemcpyHostToDevice, stream_), "up_off");
            if (!g.up_links.empty())
                hip_check(hipMemcpyAsync(d_up_links_.ptr(), g.up_links.data(), g.up_links.size() * 4,
                                         hipMemcpyHostToDevice, stream_),
                          "up_links");
        }
    }
    hip_check(hipStreamSynchronize(stream_), "string upload");
    d_n_ = n;
    rows_uploaded = n;
    rows_appended = 0;
    upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// The graph: the host builder (hnsw_build.cpp) with the string distance, in the reference's insertion order at
// indexThreadQty=1
void Engine::build_string_graph() {
    const auto t0 = std::chrono::steady_clock::now();
    hnsw_build_strings(space_, st_ptr_.data(), st_bytes_.data(), st_words_.data(), ham_words(), ids_.size(), bp_, graph_);
    graph_builder_ = 1;
    build_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// Hnsw::Search with searchMethod_ = 0 (hnsw.cc:724-733): baseSearchAlgorithmOld for algoType=old or hybrid with
// ef >= 1000, else baseSearchAlgorithmV1Merge.  Queries go through in slices that keep the per-query workspaces
// (visited bits, sorted array or heaps, leven block state) within 256 MiB.
void Engine::knn_string_hnsw(const int64_t* d_qoff, const int32_t* d_qlen, const uint64_t* d_peq, const uint32_t* d_qw,
                             int nw_max, size_t nq, size_t k, int32_t* d_ids, float* d_dists, int32_t* d_cnt) {
    const HostGraph& g = graph_;
    const bool old = search_old();
    StringHnswArgs a{};
    a.space = space_;
    a.row_ptr = d_st_ptr_.as<int64_t>();
    a.data = d_st_data_.as<uint8_t>();
    a.words = d_st_data_.as<uint32_t>();
    a.W = (int)ham_words();
    a.q_off = d_qoff;
    a.q_len = d_qlen;
    a.peq = reinterpret_cast<const unsigned long long*>(d_peq);
    a.q_words = d_qw;
    a.nw_max = nw_max;
    a.links0 = d_links0_.as<int32_t>();
    a.up_off = d_up_off_.as<int64_t>();
    a.up_links = d_up_links_.as<int32_t>();
    a.ext_ids = d_ids_.as<int32_t>();
    a.n = g.n;
    a.maxM = g.maxM;
    a.maxM0 = g.maxM0;
    a.maxlevel = g.maxlevel;
    a.enterpoint = g.enterpoint;
    a.ef = ef_;
    a.k = (int)k;
    a.vis_words = ((size_t)g.n + 31) / 32;
    a.ws_per_query = string_hnsw_ws_words(a, old);
    const size_t per_query = a.vis_words * 4 + a.ws_per_query * 8 + (size_t)64 * 2 * nw_max * 8;
    const size_t m = std::max<size_t>(1, std::min<size_t>(nq, ((size_t)256 << 20) / per_query));
    ws_split_.ensure(m * per_query);
    a.visited = ws_split_.as<uint32_t>();
    a.ws = reinterpret_cast<unsigned long long*>(ws_split_.as<char>() + align8(m * a.vis_words * 4));
    a.mw_ws = a.ws + m * a.ws_per_query;
    ws_ndc_.ensure(nq * 4);
    ws_hops_.ensure(nq * 4);
    ws_hops_up_.ensure(nq * 4);
    a.ndc = ws_ndc_.as<int32_t>();
    a.hops = ws_hops_.as<int32_t>();
    a.hops_up = ws_hops_up_.as<int32_t>();
    a.out_ids = d_ids;
    a.out_d = d_dists;
    a.out_cnt = d_cnt;
    for (size_t q0 = 0; q0 < nq; q0 += m) {
        const size_t mm = std::min(m, nq - q0);
        hip_check(hipMemsetAsync(a.visited, 0, mm * a.vis_words * 4, stream_), "visited clear");
        prof_begin(stream_);
        hip_check(launch_string_hnsw(a, old, (int)q0, (int)mm, stream_), "string hnsw search");
        prof_end(stream_);
    }
    have_counters_ = true;
}

namespace {
// Peq table of a pattern: [nw][256] words, bit i % 64 of word [i / 64][p[i]] set
void build_peq(const uint8_t* p, size_t m, uint64_t* out) {
    const size_t nw = (m + 63) / 64;
    std::memset(out, 0, nw * 256 * 8);
    for (size_t i = 0; i < m; ++i) out[(i / 64) * 256 + p[i]] |= 1ull << (i % 64);
}
}  // namespace

// A query of a leven index: its bytes (empty: refused); of a bit_hamming index: its packed words (bit count checked).
void Engine::string_query(const char* s, size_t len, Err parse_err, std::vector<uint32_t>& words) const {
    if (space_ == SP_LEVEN) {
        if (len == 0) throw EngineError(Err::InvalidArgument, "leven: empty query string");
        if (len > (size_t)INT32_MAX) throw EngineError(Err::InvalidArgument, "leven: query string too long");
        return;
    }
    size_t b = 0;
    if (!parse_bits(s, len, words, b))
        throw EngineError(parse_err, "bit_hamming: failed to parse the query (only 0 and 1 values are allowed)");
    if ((int64_t)b != st_bits_)
        throw EngineError(Err::InvalidArgument, "bit_hamming: the query has " + std::to_string(b) + " bits, the index " +
                                                    std::to_string(st_bits_));
}

void Engine::knn_string_host(const char* const* queries, const size_t* lens, size_t nq, size_t k, const int32_t** ids,
                             const float** dists, const int32_t** cnt) {
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (k == 0) throw EngineError(Err::InvalidArgument, "k must be positive");
    if (k > (size_t)INT32_MAX / 2) throw EngineError(Err::QueryTooLarge, "k is too large");
    // every query is checked before any work
    const bool lev = space_ == SP_LEVEN;
    const size_t W = ham_words();
    std::vector<uint32_t> qwords, w;
    size_t peq_words = 0;
    int nw_max = 1;
    for (size_t i = 0; i < nq; ++i) {
        string_query(queries[i], lens[i], Err::QueryExecutionFailed, w);
        if (lev) {
            peq_words += (lens[i] + 63) / 64 * 256;
            nw_max = std::max(nw_max, (int)((lens[i] + 63) / 64));
        } else {
            qwords.insert(qwords.end(), w.begin(), w.end());
        }
    }
    if (!lev && st_bits_ < 0) throw EngineError(Err::QueryExecutionFailed, "bit_hamming: the index holds no rows");
    if (dirty_) finalize();
    check_device();
    order_after_last(stream_);
    // device / pinned layout of the batch: leven q_off int64 [nq+1] | q_len int32 [nq] | Peq u64; bit_hamming words
    const size_t off_b = (nq + 1) * 8, len_b = align8(nq * 4);
    const size_t qbytes = lev ? off_b + len_b + peq_words * 8 : qwords.size() * 4;
    char* hp = static_cast<char*>(pinned(std::max(std::max<size_t>(qbytes, 8), 2 * nq * k * 4 + nq * 4)));
    if (lev) {
        int64_t* hoff = reinterpret_cast<int64_t*>(hp);
        int32_t* hlen = reinterpret_cast<int32_t*>(hp + off_b);
        uint64_t* hpeq = reinterpret_cast<uint64_t*>(hp + off_b + len_b);
        size_t at = 0;
        for (size_t i = 0; i < nq; ++i) {
            hoff[i] = (int64_t)at;
            hlen[i] = (int32_t)lens[i];
            build_peq(reinterpret_cast<const uint8_t*>(queries[i]), lens[i], hpeq + at);
            at += (lens[i] + 63) / 64 * 256;
        }
        hoff[nq] = (int64_t)at;
    } else if (!qwords.empty()) {
        std::memcpy(hp, qwords.data(), qbytes);
    }
    ws_bq_.ensure(std::max<size_t>(qbytes, 8));
    hip_check(hipMemcpyAsync(ws_bq_.ptr(), hp, qbytes, hipMemcpyHostToDevice, stream_), "string queries H2D");
    const int64_t* d_qoff = ws_bq_.as<int64_t>();
    const int32_t* d_qlen = reinterpret_cast<const int32_t*>(ws_bq_.as<char>() + off_b);
    const uint64_t* d_peq = reinterpret_cast<const uint64_t*>(ws_bq_.as<char>() + off_b + len_b);
    const uint32_t* d_qw = ws_bq_.as<uint32_t>();

    const ResultBlock out = result_block(nq, k);
    if (method_ == Method::Hnsw && d_n_ > 0) {
        knn_string_hnsw(d_qoff, d_qlen, d_peq, d_qw, nw_max, nq, k, out.ids, out.dists, out.cnt);
        fetch_results(nq, k, "string hnsw", ids, dists, cnt);
        last_path = 0;
        return;
    }
    have_counters_ = false;
    const int tq = (lev && nw_max > 1) ? 1 : kStrTileQ;
    scan_slices(nq, k, tq, out, [&](const ScanPlan& p, size_t q0, float* split_d, int32_t* split_pos) {
        if (lev) {
            const size_t mw = leven_mw_ws_words(p, nw_max);
            if (mw) ws_st_mw_.ensure(mw * 8);
            hip_check(launch_leven_knn(p, d_st_ptr_.as<int64_t>(), d_st_data_.as<uint8_t>(), d_qoff + q0, d_qlen + q0,
                                       d_peq, nw_max, mw ? ws_st_mw_.as<uint64_t>() : nullptr, split_d, split_pos,
                                       stream_),
                      "leven scan");
        } else {
            hip_check(launch_ham_knn(p, d_st_data_.as<uint32_t>(), (int)W, d_qw + q0 * W, split_d, split_pos, stream_),
                      "bit_hamming scan");
        }
    });
    fetch_results(nq, k, "string knn", ids, dists, cnt);
    last_path = 0;
}

size_t Engine::range_string_host(const char* query, size_t len, double radius, size_t capacity, int32_t* ids,
                                 float* dists) {
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    const bool lev = space_ == SP_LEVEN;
    std::vector<uint32_t> qw;
    string_query(query, len, Err::Runtime, qw);
    if (dirty_) finalize();
    check_device();
    order_after_last(stream_);
    const size_t n = d_n_;
    if (n == 0 || capacity == 0) return 0;
    // RangeQuery<int>(space, obj, static_cast<int>(radius)), nmslib_c.cpp:1092-1093: the radius truncates to int
    const double rc = std::max(-1.0, std::min(radius, 2147483647.0));
    const float r = (float)(int)rc;
    // both distances are symmetric: the filter d(row, query) is also the reported d(query, row)
    return range_select(false, r, capacity, ids, dists, [&](float* d, float*) {
        if (lev) {
            const size_t nw = (len + 63) / 64;
            std::vector<uint64_t> peq(nw * 256);
            build_peq(reinterpret_cast<const uint8_t*>(query), len, peq.data());
            ws_q_.ensure(peq.size() * 8);
            hip_check(hipMemcpyAsync(ws_q_.ptr(), peq.data(), peq.size() * 8, hipMemcpyHostToDevice, stream_), "query H2D");
            const size_t mw = nw > 1 ? (size_t)2 * nw * 256 * leven_dist_grid((int)n) : 0;
            if (mw) ws_st_mw_.ensure(mw * 8);
            hip_check(launch_leven_dist(d_st_ptr_.as<int64_t>(), d_st_data_.as<uint8_t>(), (int)n, ws_q_.as<uint64_t>(),
                                        (int)len, (int)nw, mw ? ws_st_mw_.as<uint64_t>() : nullptr, d, stream_),
                      "leven range distances");
        } else {
            ws_q_.ensure(std::max<size_t>(qw.size(), 1) * 4);
            hip_check(hipMemcpyAsync(ws_q_.ptr(), qw.data(), qw.size() * 4, hipMemcpyHostToDevice, stream_), "query H2D");
            hip_check(launch_ham_dist(d_st_data_.as<uint32_t>(), (int)ham_words(), (int)n, ws_q_.as<uint32_t>(), d, stream_),
                      "bit_hamming range distances");
        }
    });
}

float Engine::pair_distance_string(size_t p1, size_t p2) {
    // IndexTimeDistance(data[p1], data[p2]) (nmslib_c.cpp:1166) on the device store
    if (dirty_) finalize();
    check_device();
    order_after_last(stream_);
    ws_pair_.ensure(16);
    float* out = ws_pair_.as<float>();
    if (space_ == SP_LEVEN) {
        const size_t m = (size_t)(st_ptr_[p1 + 1] - st_ptr_[p1]), nw = (m + 63) / 64;
        std::vector<uint64_t> peq(nw * 256);
        build_peq(st_bytes_.data() + st_ptr_[p1], m, peq.data());
        ws_q_.ensure(peq.size() * 8 + 2 * nw * 8);
        uint64_t* d_peq = ws_q_.as<uint64_t>();
        hip_check(hipMemcpyAsync(d_peq, peq.data(), peq.size() * 8, hipMemcpyHostToDevice, stream_), "pair H2D");
        hip_check(launch_leven_pair(d_st_ptr_.as<int64_t>(), d_st_data_.as<uint8_t>(), (int)p2, d_peq, (int)m, (int)nw,
                                    d_peq + peq.size(), out, stream_),
                  "leven pair distance");
    } else {
        hip_check(launch_ham_pair(d_st_data_.as<uint32_t>(), (int)ham_words(), (int)p1, (int)p2, out, stream_),
                  "bit_hamming pair distance");
    }
    return read_float(out, "string pair distance");
}

}  // namespace gfxknn
