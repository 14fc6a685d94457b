// Engine: host logic around the gfx950 kernels (see engine.hpp).
#include "engine.hpp"
#include "f16_pack.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <set>
#include <sstream>
#include <thread>
#include <unordered_set>

namespace gfxknn {

using clk = std::chrono::steady_clock;

void hip_check(hipError_t e, const char* what) {
    if (e == hipSuccess) return;
    std::string msg = std::string(what) + ": " + hipGetErrorString(e);
    (void)hipGetLastError();
    throw EngineError(e == hipErrorOutOfMemory ? Err::OutOfMemory : Err::Runtime, msg);
}

// ---------------------------------------------------------------------------------------------
// ParamSet
// ---------------------------------------------------------------------------------------------
ParamSet::ParamSet(const std::vector<std::string>& desc) {
    std::set<std::string> seen;
    for (const std::string& d : desc) {
        // AnyParams(const vector<string>&), params.h:50-74: exactly one '=' separating two parts
        size_t eq = d.find('=');
        if (eq == std::string::npos || d.find('=', eq + 1) != std::string::npos || eq == 0 || eq + 1 == d.size())
            throw std::runtime_error("Wrong format of an argument: '" + d + "' should be in the format: <Name>=<Value>");
        std::string name = d.substr(0, eq), val = d.substr(eq + 1);
        if (seen.count(name)) throw std::runtime_error("Duplicate parameter: " + name);
        seen.insert(name);
        kv_.emplace_back(name, val);
    }
    seen_.assign(kv_.size(), false);
}
bool ParamSet::has(const std::string& name) const {
    for (auto& p : kv_)
        if (p.first == name) return true;
    return false;
}
const std::string* ParamSet::find(const std::string& name) {
    for (size_t i = 0; i < kv_.size(); ++i)
        if (kv_[i].first == name) {
            seen_[i] = true;
            return &kv_[i].second;
        }
    return nullptr;
}
template <typename T>
static void convert(const std::string& s, T& v) {
    std::stringstream str(s);
    if (!(str >> v) || !str.eof()) throw std::runtime_error("Failed to convert value '" + s + "'");
}
void ParamSet::get(const std::string& name, long long& v) {
    if (auto s = find(name)) convert(*s, v);
}
void ParamSet::get(const std::string& name, int& v) {
    if (auto s = find(name)) convert(*s, v);
}
void ParamSet::get(const std::string& name, size_t& v) {
    if (auto s = find(name)) convert(*s, v);
}
void ParamSet::get(const std::string& name, double& v) {
    if (auto s = find(name)) convert(*s, v);
}
void ParamSet::get(const std::string& name, bool& v) {
    if (auto s = find(name)) convert(*s, v);
}
void ParamSet::get(const std::string& name, std::string& v) {
    if (auto s = find(name)) v = *s;
}
void ParamSet::check_unused() const {
    for (size_t i = 0; i < kv_.size(); ++i)
        if (!seen_[i]) throw std::runtime_error("Unknown parameters found!");
}

// ---------------------------------------------------------------------------------------------
// DevBuf, Event, PinnedBuf
// ---------------------------------------------------------------------------------------------
void* DevBuf::ensure(size_t bytes) {
    if (bytes <= n_ && p_) return p_;
    release();
    if (bytes == 0) bytes = 16;
    hip_check(hipMalloc(&p_, bytes), "hipMalloc");
    n_ = bytes;
    // NMSLIB_GPU_POISON=<byte>: fill every new workspace with that byte, so that a kernel reading memory nobody wrote
    // shows up in the tests instead of depending on what the allocator hands back
    static const char* poison = getenv("NMSLIB_GPU_POISON");
    if (poison) {
        // (waited for: the fill runs on the null stream, the buffer's first user may be a stream that does not wait for it)
        hip_check(hipMemset(p_, atoi(poison) & 0xFF, bytes), "poison");
        hip_check(hipStreamSynchronize(nullptr), "poison");
    }
    return p_;
}
void* DevBuf::grow_keep(size_t bytes, size_t keep, hipStream_t s) {
    if (bytes <= n_ && p_) return p_;
    DevBuf grown;
    grown.ensure(bytes);
    if (keep > n_) keep = n_;
    if (p_ && keep) {
        hip_check(hipMemcpyAsync(grown.p_, p_, keep, hipMemcpyDeviceToDevice, s), "grow: copy");
        hip_check(hipStreamSynchronize(s), "grow: copy");  // the old block is freed below
    }
    swap(grown);
    return p_;
}
void DevBuf::swap(DevBuf& o) {
    std::swap(p_, o.p_);
    std::swap(n_, o.n_);
}

void DevBuf::release() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
    n_ = 0;
}

void Event::record(hipStream_t s) {
    if (!e_) hip_check(hipEventCreateWithFlags(&e_, hipEventDisableTiming), "hipEventCreate");
    hip_check(hipEventRecord(e_, s), "hipEventRecord");
}
void* PinnedBuf::ensure(size_t bytes, size_t slack) {
    if (bytes <= n_ && p_) return p_;
    if (p_) (void)hipHostFree(p_);
    p_ = nullptr;
    hip_check(hipHostMalloc(&p_, n_ = bytes + slack, hipHostMallocDefault), "hipHostMalloc");
    return p_;
}

// ---------------------------------------------------------------------------------------------
// Engine: construction / data
// ---------------------------------------------------------------------------------------------
static int space_from_name(const std::string& s) {
    // registered dense names: include/factory/init_spaces.h:77-86,120
    if (s == "l2") return SP_L2;
    if (s == "l1") return SP_L1;
    if (s == "linf") return SP_LINF;
    if (s == "cosinesimil") return SP_COSINE;
    if (s == "angulardist") return SP_ANGULAR;
    if (s == "negdotprod") return SP_NEGDOT;
    if (s == "l2sqr_sift") return SP_L2SQR_SIFT;
    return -1;
}

// The divergences over dense float rows (include/factory/init_spaces.h:57-71): the Bregman family and Jensen-Shannon.
static int diverg_space_from_name(const std::string& s) {
    if (s == "kldivfast") return SP_KLDIV;
    if (s == "kldivfastrq") return SP_KLDIV_RQ;
    if (s == "kldivgenfast") return SP_KLDIVGEN;
    if (s == "kldivgenfastrq") return SP_KLDIVGEN_RQ;
    if (s == "kldivgenslow") return SP_KLDIVGEN_SLOW;
    if (s == "itakurasaitofast") return SP_ITAKURASAITO;
    if (s == "jsdivfast") return SP_JSDIV;
    if (s == "jsdivslow") return SP_JSDIV_SLOW;
    if (s == "jsmetrfast") return SP_JSMETR;
    if (s == "jsmetrslow") return SP_JSMETR_SLOW;
    return -1;
}

// Sparse spaces whose objects the reference's C ABI can build (SpaceSparseVectorSimpleStorage, nmslib_c.cpp:245-265):
// include/space/space_sparse_scalar.h:32-35, include/space/space_sparse_lp.h.  lp_sparse needs its parameter p.
static int sparse_space_from_name(const std::string& s, const std::vector<std::string>& space_params) {
    if (s == "cosinesimil_sparse") return SP_COSINE;
    if (s == "angulardist_sparse") return SP_ANGULAR;
    if (s == "negdotprod_sparse") return SP_NEGDOT;
    if (s == "querynorm_negdotprod_sparse") return SP_QNORM_NEGDOT;
    if (s == "l1_sparse") return SP_L1;
    if (s == "l2_sparse") return SP_L2;
    if (s == "linf_sparse") return SP_LINF;
    if (s == "lp_sparse") {
        ParamSet ps(space_params);
        if (!ps.has("p")) throw EngineError(Err::SpaceIncompatible, "lp_sparse: parameter p is required");
        double p = 0;
        ps.get("p", p);
        // SpaceLpDist (include/space/space_lp.h:43-66): p in {-1, 1, 2} selects LInf / L1 / L2NormSIMD
        const float pf = (float)p;
        if (pf == -1.f) return SP_LINF;
        if (pf == 1.f) return SP_L1;
        if (pf == 2.f) return SP_L2;
        throw EngineError(Err::SpaceIncompatible, "lp_sparse: only p = 1, 2 and -1 are served by the GPU engine (p = " +
                                                      std::to_string(p) + " uses the generic Lp formula)");
    }
    return -1;
}

Engine::Engine(const std::string& space, const std::string& method, int data_type, int dist_type,
               const std::vector<std::string>& space_params)
    : space_name_(space), method_name_(method) {
    if (space == "jsdivfastapprox" || space == "jsmetrfastapprox")
        throw EngineError(Err::SpaceIncompatible,
                          "space '" + space + "' is not served by the GPU engine: its table-lookup logarithm is not "
                          "restated (Jensen-Shannon spaces: jsdivslow, jsdivfast, jsmetrslow, jsmetrfast)");
    if (const int dsp = diverg_space_from_name(space); dsp >= 0) {
        if (data_type != 0)
            throw EngineError(Err::SpaceIncompatible, "divergence space '" + space + "' is served over dense float "
                                                      "vectors only (data type 0)");
        if (dist_type != 0)
            throw EngineError(Err::SpaceIncompatible, "divergence space '" + space + "' is served with the float "
                                                      "distance type");
        if (method != "brute_force" && method != "seq_search")
            throw EngineError(Err::SpaceIncompatible,
                              "method '" + method + "' over divergence space '" + space + "' is not served: a graph over "
                              "a non-symmetric divergence is not built (divergences: brute_force, seq_search)");
        space_ = dsp;
        diverg_ = true;
        thread_pool_size = std::thread::hardware_concurrency();
        return;
    }
    if (data_type == 1) {
        const int ssp = sparse_space_from_name(space, space_params);
        if (ssp < 0)
            throw EngineError(Err::SpaceIncompatible,
                              "sparse space '" + space + "' is not served by the GPU engine (sparse spaces: "
                              "cosinesimil_sparse, angulardist_sparse, negdotprod_sparse, querynorm_negdotprod_sparse, "
                              "l1_sparse, l2_sparse, linf_sparse, lp_sparse with p = 1, 2, -1)");
        if (method != "brute_force" && method != "seq_search")
            throw EngineError(Err::SpaceIncompatible,
                              "method '" + method + "' over sparse data is not served (sparse: brute_force, seq_search)");
        space_ = ssp;
        sparse_ = true;
        thread_pool_size = std::thread::hardware_concurrency();
        return;
    }
    if (data_type == 3) {
        // the int-registry string spaces (include/factory/init_spaces.h:47-53) with the int distance; normleven and
        // bit_jaccard are float spaces that the reference's data type 3 dispatch would treat as int indexes
        // (nmslib_c.cpp:205-208)
        if (space != "leven" && space != "bit_hamming")
            throw EngineError(Err::SpaceIncompatible,
                              "string space '" + space + "' is not served by the GPU engine (string spaces: leven, "
                              "bit_hamming)");
        if (dist_type != 1)
            throw EngineError(Err::SpaceIncompatible, "string space '" + space + "' is served with the int distance type");
        if (method != "brute_force" && method != "seq_search" && method != "hnsw")
            throw EngineError(Err::SpaceIncompatible, "method '" + method +
                                                          "' over string data is not served (strings: hnsw, brute_force, "
                                                          "seq_search)");
        space_ = space == "leven" ? SP_LEVEN : SP_BIT_HAMMING;
        str_space_ = true;
        thread_pool_size = std::thread::hardware_concurrency();
        return;
    }
    const int sp = space_from_name(space);
    if (sp < 0)
        throw EngineError(Err::SpaceIncompatible,
                          "space '" + space + "' is not served by the GPU engine (dense spaces: l2, l1, linf, "
                          "cosinesimil, angulardist, negdotprod, l2sqr_sift; divergences: kldivfast, kldivfastrq, "
                          "kldivgenfast, kldivgenfastrq, kldivgenslow, itakurasaitofast, jsdivslow, jsdivfast, "
                          "jsmetrslow, jsmetrfast)");
    space_ = sp;
    // data_type: 0 dense float, 2 dense uint8 (nmslib_c.h:12-17)
    if (data_type != 0 && data_type != 2)
        throw EngineError(Err::SpaceIncompatible, "only dense float and dense uint8 data are served by the GPU engine");
    if ((sp == SP_L2SQR_SIFT) != (data_type == 2))
        throw EngineError(Err::SpaceIncompatible, "data type does not match space '" + space + "'");
    // The method name is resolved at nmslib_create_index, like the reference
    // (MethodFactoryRegistry::CreateMethod, nmslib_c.cpp:493-496).
    thread_pool_size = std::thread::hardware_concurrency();
}

Engine::~Engine() {
    for (auto& pr : prof_events_) {
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    // the members go after stream_: destroying an event or freeing pinned or device memory behind its stream is legal
    if (stream_) (void)hipStreamDestroy(stream_);
}

void Engine::order_after_last(hipStream_t next) {
    if (have_last_ && last_stream_ != next) {
        order_event_.record(last_stream_);
        order_event_.stream_wait(next);
    }
    last_stream_ = next;
    have_last_ = true;
}

std::pair<hipEvent_t, hipEvent_t> Engine::prof_pair() {
    if (!prof_ || prof_events_.size() >= 65536) return {nullptr, nullptr};
    hipEvent_t a, b;
    hip_check(hipEventCreate(&a), "hipEventCreate");
    hip_check(hipEventCreate(&b), "hipEventCreate");
    prof_events_.emplace_back(a, b);
    return prof_events_.back();
}
void Engine::prof_begin(hipStream_t s) {
    if (hipEvent_t a = prof_pair().first) hip_check(hipEventRecord(a, s), "hipEventRecord");
}
void Engine::prof_end(hipStream_t s) {
    if (!prof_ || prof_events_.empty()) return;
    hip_check(hipEventRecord(prof_events_.back().second, s), "hipEventRecord");
}
void Engine::collect_profile(double* total_ms, uint64_t* launches) {
    double tot = 0;
    uint64_t n = 0;
    for (auto& pr : prof_events_) {
        float ms = 0;
        if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
            tot += ms;
            ++n;
        }
        (void)hipEventDestroy(pr.first);
        (void)hipEventDestroy(pr.second);
    }
    prof_events_.clear();
    if (total_ms) *total_ms = tot;
    if (launches) *launches = n;
}

void Engine::add_row(const void* data, size_t elem_count, int32_t id) {
    if (sparse_ || str_space_) throw EngineError(Err::SpaceIncompatible, "Not dense space");
    if (is_u8()) {
        // CreateObjFromUint8Vect CHECKs size == SIFT_DIM (space_l2sqr_sift.cc:136-140)
        if (elem_count != 128) throw EngineError(Err::Runtime, "SIFT vectors must have 128 bytes");
        if (dim_ == 0) dim_ = 128;
        const uint8_t* p = static_cast<const uint8_t*>(data);
        rows_u8_.insert(rows_u8_.end(), p, p + 128);
    } else {
        if (dim_ == 0) dim_ = elem_count;
        if (elem_count != dim_)
            throw EngineError(Err::InvalidArgument, "all rows of a dense index must have the same dimension");
        const float* p = static_cast<const float*>(data);
        rows_f32_.insert(rows_f32_.end(), p, p + elem_count);
    }
    ids_.push_back(id);
    dirty_ = true;
    graph_dirty_ = true;
}

const void* Engine::host_row(size_t pos) const {
    return is_u8() ? static_cast<const void*>(&rows_u8_[pos * 128]) : static_cast<const void*>(&rows_f32_[pos * dim_]);
}

void Engine::stored_row(size_t pos, void* dst) const {
    if (is_u8()) {
        // payload = 128 bytes + int32 sum of squares (space_l2sqr_sift.cc:146-149)
        std::memcpy(dst, &rows_u8_[pos * 128], 128);
        int32_t s = 0;
        for (int i = 0; i < 128; ++i) s += (int32_t)rows_u8_[pos * 128 + i] * (int32_t)rows_u8_[pos * 128 + i];
        std::memcpy(static_cast<char*>(dst) + 128, &s, 4);
    } else {
        std::memcpy(dst, &rows_f32_[pos * dim_], dim_ * 4);
        // the "fast" divergence objects: the values, then their logarithms (CreateObjFromVect, space_bregman.cc:144-152)
        if (diverg_stores_logs()) diverg_logs(&rows_f32_[pos * dim_], dim_, static_cast<float*>(dst) + dim_);
    }
}

static const char* const kDeleteServed =
    "deleting rows is served for hnsw, brute_force and seq_search over the dense spaces (float rows and l2sqr_sift) on one "
    "device";

size_t Engine::delete_ids(const int32_t* ids, size_t count) {
    if (sparse_ || str_space_ || diverg_)
        throw EngineError(Err::SpaceIncompatible, std::string(sparse_ ? "a sparse" : str_space_ ? "a string" : "a divergence") +
                                                      " index does not delete rows: " + kDeleteServed);
    if (gpu_shards_ > 1)
        throw EngineError(Err::SpaceIncompatible, "an index with gpu_shards=" + std::to_string(gpu_shards_) +
                                                      " does not delete rows: " + kDeleteServed);
    if (count == 0) return 0;
    const std::unordered_set<int32_t> listed(ids, ids + count);
    const size_t n = ids_.size();
    size_t marked = 0;
    for (size_t i = 0; i < n; ++i) {
        if (!listed.count(ids_[i]) || is_dead(i)) continue;
        if (tomb_.size() <= (i >> 5)) tomb_.resize((n + 31) / 32, 0);
        tomb_[i >> 5] |= 1u << (i & 31);
        ++marked;
    }
    if (!marked) return 0;
    n_dead_ += marked;
    if (!shards_.empty()) dirty_ = graph_dirty_ = true;  // shards made without being asked for: back to one device
    if (!created_) return marked;
    if (method_ == Method::Brute) dirty_ = true;  // the scan's index is prepared again, over the live rows
    else if (!dirty_) upload_tombstones();        // a resident graph: the filter's bitset follows now
    return marked;
}

// The whole bitset goes to the device again (125 KB at 1M rows), from a pinned block of its own: the copy is enqueued behind
// the index's other work and the call does not wait for it.  A batch enqueued before sees the old bits, a later one the new.
void Engine::upload_tombstones() {
    check_device();
    const size_t words = (size() + 31) / 32;
    tomb_.resize(words, 0);
    if (words == 0) return;
    void* hp = tomb_staged_.begin(words * 4, "tombstones");  // (its slack: room to grow with appends)
    std::memcpy(hp, tomb_.data(), words * 4);
    order_after_last(stream_);  // batches in flight read the old bits (and a buffer that grows is freed)
    d_tomb_.ensure(words * 4);
    hip_check(hipMemcpyAsync(d_tomb_.ptr(), hp, words * 4, hipMemcpyHostToDevice, stream_), "tombstones H2D");
    tomb_staged_.sent(stream_);
}

void Engine::reset() {
    ids_.clear();
    rows_f32_.clear();
    rows_u8_.clear();
    tomb_.clear();
    n_dead_ = 0;
    d_tomb_.release();
    d_livepos_.release();
    ++pos_epoch_;  // (filters of the old rows are stale)
    sp_ptr_.assign(1, 0);
    sp_ids_.clear();
    sp_vals_.clear();
    st_ptr_.assign(1, 0);
    st_bytes_.clear();
    st_words_.clear();
    st_bits_ = -1;
    graph_ = HostGraph();
    graph_rows_.clear();
    loaded_graph_ = false;
    graph_builder_ = 0;
    built_n_ = 0;
    host_links_stale_ = false;
    save_resident_rows_ = false;
    rows_appended = rows_uploaded = 0;
    created_ = false;
    dirty_ = true;
    graph_dirty_ = true;
    d_n_ = 0;
    shards_.clear();
    dim_ = 0;  // a reset index accepts rows of another dimension
    brute_ = BruteDense();
    last_path = 0;
    fast_flags_ = nullptr;
    fast_nqt_ = 0;
    hnsw_fix_valid_ = false;
    have_counters_ = false;
    d_rows16_.release();
    rows16_failed_ = false;
    rows_f16_index_ = rows_f16_ = false;
    rerank_ = 0;
    inwalk_ = false;
}

size_t Engine::memory_usage() const {
    // nmslib_index_memory_usage (nmslib_c.cpp:1546-1565): object buffers + n*dim*4
    if (!created_) return 0;
    if (sparse_)  // objects (16-byte header + elements) and the CSR copy in HBM
        return ids_.size() * 16 + sp_ids_.size() * sizeof(SparseElem) + hbm_bytes();
    if (str_space_)  // objects (16-byte header + datalength) and the store's copy in HBM
        return ids_.size() * 16 + (space_ == SP_LEVEN ? st_bytes_.size() : ids_.size() * (ham_words() + 1) * 4) +
               hbm_bytes();
    size_t total = ids_.size() * (16 + stored_row_bytes());
    total += ids_.size() * dim_ * sizeof(float);
    return total + rows16_bytes() + d_tomb_.bytes();
}

size_t Engine::rows16_bytes() const {
    size_t b = d_rows16_.bytes();
    for (const auto& c : shards_) b += c->rows16_bytes();
    return b;
}

size_t Engine::hbm_bytes() const {
    size_t sh = 0;
    for (const auto& c : shards_) sh += c->hbm_bytes();
    return sh + d_rows_.bytes() + d_aux_.bytes() + d_ids_.bytes() + d_links0_.bytes() + d_up_off_.bytes() + d_up_links_.bytes() +
           d_rownorm_.bytes() + d_rows16_.bytes() + d_tomb_.bytes() + d_livepos_.bytes() + brute_.bytes() + d_sp_ptr_.bytes() + d_sp_ids_.bytes() + d_sp_vals_.bytes() + d_st_ptr_.bytes() + d_st_data_.bytes();
}

// ---------------------------------------------------------------------------------------------
// Index / query parameters
// ---------------------------------------------------------------------------------------------
void Engine::create_index(const std::vector<std::string>& params) {
    ParamSet ps(params);
    int defer = 0;
    if (method_name_ == "hnsw") {
        method_ = Method::Hnsw;
        HnswBuildParams bp;
        // Hnsw::CreateIndex, hnsw.cc:187-208
        ps.get("M", bp.M);
        int search_method = 0;
        ps.get("searchMethod", search_method);
        ps.get("indexThreadQty", bp.threads);
        ps.get("efConstruction", bp.efConstruction);
        bp.maxM = bp.M;
        ps.get("maxM", bp.maxM);
        bp.maxM0 = bp.M * 2;
        ps.get("maxM0", bp.maxM0);
        ps.get("mult", bp.mult);
        ps.get("delaunay_type", bp.delaunay);
        ps.get("post", bp.post);
        int skip = 0;
        ps.get("skip_optimized_index", skip);
        bp.skip_optimized = skip != 0;
        ps.get("gpu_defer", defer);  // engine extension: build now, upload to HBM at first use
        ps.get("gpu_build", bp.gpu_build);  // engine extension: batched construction on the GPU (1), host (0)
        ps.get("gpu_build_batch", bp.gpu_build_batch);
        ps.get("gpu_build_div", bp.gpu_build_div);
        if (!str_space_) {  // the dense spaces' GPU builder (a string graph is built on the host: unknown parameters there)
            ps.get("gpu_build_cut", bp.gpu_build_cut);  // engine extension: a batch boundary at this position
            ps.get("gpu_append", bp.gpu_append);        // engine extension: later rows go into the GPU-built graph (1)
        }
        ps.get("gpu_shards", gpu_shards_);  // engine extension: row shards over the visible GPUs (0 = all)
        std::string gpu_rows = "f32";       // engine extension: f16 = the search walks an fp16 copy of the rows
        ps.get("gpu_rows", gpu_rows);
        ps.check_unused();
        const bool f16 = parse_gpu_rows(gpu_rows);
        if (f16) check_rows16_served();
        if (bp.gpu_append != 0 && bp.gpu_append != 1)
            throw EngineError(Err::IndexBuildFailed, "gpu_append must be 0 or 1, got " + std::to_string(bp.gpu_append));
        if (bp.gpu_build_cut < 0)
            throw EngineError(Err::IndexBuildFailed, "gpu_build_cut must be a row position (0 = off), got " +
                                                         std::to_string(bp.gpu_build_cut));
        rows_f16_index_ = rows_f16_ = f16;
        rerank_ = 0;
        inwalk_ = false;
        if (defer && bp.gpu_build < 0) bp.gpu_build = 0;  // deferred upload = no device work now
        bp_ = bp;
        ef_ = 200;  // the shim forces efSearch=200 per query (nmslib_c.cpp:330,986)
        algo_ = "hybrid";
    } else if (method_name_ == "brute_force" || method_name_ == "seq_search") {
        method_ = Method::Brute;
        bool copy_mem = false, multi = false;
        size_t thread_qty = 0;
        ps.get("copyMem", copy_mem);  // SeqSearch::CreateIndex, seqsearch.cc:63-66
        ps.get("multiThread", multi);
        ps.get("threadQty", thread_qty);
        ps.get("gpu_defer", defer);
        ps.get("gpu_shards", gpu_shards_);
        ps.check_unused();
        if ((sparse_ || str_space_ || diverg_) && gpu_shards_ != -1 && gpu_shards_ != 1)
            throw EngineError(Err::IndexBuildFailed, std::string(sparse_ ? "a sparse" : str_space_ ? "a string" : "a divergence") +
                                                         " index runs on one GPU: gpu_shards=" +
                                                         std::to_string(gpu_shards_) + " is not supported");
    } else {
        throw EngineError(Err::IndexBuildFailed,
                          "method '" + method_name_ + "' is not served by the GPU engine (hnsw, brute_force, seq_search)");
    }
    if (n_dead_ && gpu_shards_ > 1)
        throw EngineError(Err::SpaceIncompatible, "gpu_shards=" + std::to_string(gpu_shards_) + " on an index with deleted rows: " +
                                                      kDeleteServed);
    created_ = true;
    dirty_ = true;
    graph_dirty_ = true;
    loaded_graph_ = false;
    graph_builder_ = 0;
    built_n_ = 0;
    host_links_stale_ = false;
    save_resident_rows_ = false;
    if (!ids_.empty()) {
        if (defer) ensure_graph();
        else finalize();
    }
}

void Engine::set_query_params(const std::vector<std::string>& params) {
    ParamSet ps(params);
    if (method_ == Method::Hnsw) {
        // Hnsw::SetQueryTimeParams, hnsw.cc:472-507
        if (ps.has("ef") && ps.has("efSearch"))
            throw std::runtime_error("The user shouldn't specify parameters ef and efSearch at the same time");
        size_t ef = 20;
        ps.get("ef", ef);
        ps.get("efSearch", ef);
        int tmp = 0;
        ps.get("searchMethod", tmp);
        std::string algo = "hybrid";
        ps.get("algoType", algo);
        std::transform(algo.begin(), algo.end(), algo.begin(), ::tolower);
        if (algo != "v1merge" && algo != "old" && algo != "hybrid")
            throw std::runtime_error("algoType should be one of the following: old, v1merge");
        // engine extensions (absent: unchanged)
        const bool has_rows = ps.has("gpu_rows"), has_rerank = ps.has("gpu_rerank");
        std::string gpu_rows = "f32";
        long long rerank = 0;
        ps.get("gpu_rows", gpu_rows);
        ps.get("gpu_rerank", rerank);
        // (the dense spaces' in-walk kernel: an unknown parameter on a string or a sparse graph)
        const bool has_inwalk = !str_space_ && !sparse_ && ps.has("gpu_inwalk");
        std::string inwalk = "0";
        if (has_inwalk) ps.get("gpu_inwalk", inwalk);
        ps.check_unused();
        if (has_inwalk && inwalk != "0" && inwalk != "1")
            throw EngineError(Err::InvalidArgument, "gpu_inwalk must be 0 or 1, got '" + inwalk + "'");
        if (ef < 1) throw std::runtime_error("ef must be positive");
        const bool f16 = has_rows && parse_gpu_rows(gpu_rows);
        if (f16) check_rows16_served();
        if (has_rerank && rerank < 1)
            throw EngineError(Err::InvalidArgument, "gpu_rerank must be at least 1 (it is clamped to [k, max(ef, k)]), got " +
                                                        std::to_string(rerank));
        ef_ = (int)ef;
        algo_ = algo;
        if (has_rows) rows_f16_ = f16;
        if (has_rerank) rerank_ = (int)std::min<long long>(rerank, INT32_MAX);
        if (has_inwalk) inwalk_ = inwalk == "1";
    } else {
        ps.check_unused();  // SeqSearch has no query-time parameters
    }
}

bool Engine::parse_gpu_rows(const std::string& v) {
    if (v == "f32") return false;
    if (v == "f16") return true;
    throw EngineError(Err::InvalidArgument, "gpu_rows must be f32 or f16, got '" + v + "'");
}

void Engine::check_rows16_served() const {
    if (is_u8())
        throw EngineError(Err::InvalidArgument, "gpu_rows=f16: l2sqr_sift rows are uint8 (128 bytes each, less than an fp16 "
                                                "copy would take); the fp16 copy serves the float dense spaces");
    if (str_space_ || sparse_ || diverg_)
        throw EngineError(Err::InvalidArgument, std::string("gpu_rows=f16: ") +
                                                    (str_space_ ? "a string" : sparse_ ? "a sparse" : "a divergence") +
                                                    " index has no dense float rows to copy; the fp16 copy serves hnsw "
                                                    "over l2, l1, linf, cosinesimil, angulardist and negdotprod");
}

// ---------------------------------------------------------------------------------------------
// Device residency
// ---------------------------------------------------------------------------------------------
void Engine::check_device() {
    if (device_ >= 0) {
        hip_check(hipSetDevice(device_), "hipSetDevice");
        return;
    }
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        (void)hipGetLastError();
        throw EngineError(Err::Runtime,
                          "no HIP device available: the k-NN path of this library runs only on the GPU "
                          "(there is no CPU fallback)");
    }
    int dev = 0;
    if (forced_device_ >= 0) dev = forced_device_ % count;
    else if (const char* env = getenv("NMSLIB_GPU_DEVICE")) dev = atoi(env);
    else if (const char* lr = getenv("LOCAL_RANK")) dev = atoi(lr) % count;
    hip_check(hipSetDevice(dev), "hipSetDevice");
    device_ = dev;
    hip_check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
}

// Rows [first, n) go to HBM.  first = 0: all of them, into buffers sized for n.  first > 0 (gpu_append): the buffers grow keeping
// rows [0, first), and only the new rows cross PCIe.
//
// Exact scan with tombstones: the live rows and their ids are staged contiguously, in position order, and go up in the place of
// all rows -- from here on the index is the one a caller gets by adding the live rows only (d_n_ = their number).
void Engine::upload_rows(size_t first) {
    std::vector<float> live_f32;
    std::vector<uint8_t> live_u8;
    std::vector<int32_t> live_ids, live_pos;
    const bool compact = method_ == Method::Brute && n_dead_ > 0 && !parent_;
    ++prepared_;
    if (compact) {
        const size_t all = size(), rb = row_bytes();
        live_ids.reserve(all - n_dead_);
        live_pos.reserve(all - n_dead_);
        if (is_u8()) live_u8.resize((all - n_dead_) * rb);
        else live_f32.resize((all - n_dead_) * dim_);
        char* dst = is_u8() ? reinterpret_cast<char*>(live_u8.data()) : reinterpret_cast<char*>(live_f32.data());
        for (size_t i = 0; i < all; ++i) {
            if (is_dead(i)) continue;
            std::memcpy(dst + live_ids.size() * rb, host_row(i), rb);
            live_ids.push_back(ids_[i]);
            live_pos.push_back((int32_t)i);
        }
    }
    const size_t n = compact ? live_ids.size() : size(), added = n - first;
    const int32_t* src_ids = compact ? live_ids.data() : ids_.data();
    auto t0 = clk::now();
    dg_.rows16 = nullptr;  // the fp16 copy follows the rows
    rows16_failed_ = false;
    auto room = [&](DevBuf& b, size_t row_bytes) {
        if (first) b.grow_keep(n * row_bytes, first * row_bytes, stream_);
        else b.ensure(std::max<size_t>(n, 1) * row_bytes);
    };
    if (is_u8()) {
        ldb_ = 128;
        room(d_rows_, 128);
        if (added)
            hip_check(hipMemcpy(d_rows_.as<uint8_t>() + first * 128, (compact ? live_u8.data() : rows_u8()) + first * 128,
                                added * 128, hipMemcpyHostToDevice),
                      "upload rows");
    } else {
        ldb_ = f32_row_stride((int)dim_);
        room(d_rows_, (size_t)ldb_ * 4);
        const float* src = compact ? live_f32.data() : rows_f32();
        if (loaded_graph_ && !graph_rows_.empty()) src = graph_rows_.data();
        if (added) {
            float* dst = d_rows_.as<float>() + first * (size_t)ldb_;
            hip_check(hipMemset(dst, 0, added * ldb_ * 4), "clear rows");
            hip_check(hipMemcpy2D(dst, (size_t)ldb_ * 4, src + first * dim_, dim_ * 4, dim_ * 4, added, hipMemcpyHostToDevice),
                      "upload rows");
        }
    }
    room(d_ids_, 4);
    if (parent_) {
        // shard child: results carry GLOBAL positions; the parent maps them to external ids after the merge, so
        // that ties are ordered exactly as in the unsharded index (distance, position)
        std::vector<int32_t> pos(added);
        for (size_t i = 0; i < added; ++i) pos[i] = (int32_t)(view_lo_ + first + i);
        if (added)
            hip_check(hipMemcpy(d_ids_.as<int32_t>() + first, pos.data(), added * 4, hipMemcpyHostToDevice), "upload positions");
    } else if (added) {
        hip_check(hipMemcpy(d_ids_.as<int32_t>() + first, src_ids + first, added * 4, hipMemcpyHostToDevice), "upload ids");
    }
    // the resident rows' positions (one int32 each), for a filter's compaction: a filter names positions
    if (compact && n) {
        d_livepos_.ensure(n * 4);
        hip_check(hipMemcpy(d_livepos_.ptr(), live_pos.data(), n * 4, hipMemcpyHostToDevice), "upload positions");
    } else {
        d_livepos_.release();
    }
    d_n_ = n;
    rows_uploaded = added;
    rows_appended = 0;
    upload_seconds = std::chrono::duration<double>(clk::now() - t0).count();
}

void Engine::build_graph() {
    auto t0 = clk::now();
    if (!loaded_graph_) {
        const void* rows = is_u8() ? static_cast<const void*>(rows_u8()) : static_cast<const void*>(rows_f32());
        hnsw_build_host(space_, rows, size(), dim_, bp_, graph_);
        graph_builder_ = 1;
        built_n_ = 0;
        host_links_stale_ = false;
        save_resident_rows_ = false;
    }
    build_seconds = std::chrono::duration<double>(clk::now() - t0).count();
}

// first > 0 (gpu_append): rows [0, first) are prepared already and dg_ describes their graph; only rows [first, n) are touched
void Engine::prepare_graph_rows(size_t first) {
    // search-time distance of the flat ("optimized") index, hnsw.cc:369-412
    const size_t n = size(), added = n - first;
    int sspace = space_;
    bool normalize = false;
    const bool optimized = !bp_.skip_optimized;
    if (optimized) {
        if (space_ == SP_L2) sspace = SP_L2SQR;
        else if (space_ == SP_COSINE) {
            sspace = SP_NORMCOS;
            normalize = true;
        }
    }
    if (normalize && !(loaded_graph_ && !graph_rows_.empty()))
        hip_check(launch_normalize_rows(d_rows_.as<float>() + first * (size_t)ldb_, (int)added, ldb_, (int)dim_, stream_),
                  "normalize rows");
    if (is_u8()) {
        if (first) d_rownorm_.grow_keep(n * 4, first * 4, stream_);
        else d_rownorm_.ensure(std::max<size_t>(n, 1) * 4);
        std::vector<int32_t> norms(added);
        for (size_t i = 0; i < added; ++i) {
            int32_t s = 0;
            const uint8_t* r8 = rows_u8() + (first + i) * 128;
            for (int t = 0; t < 128; ++t) s += (int32_t)r8[t] * (int32_t)r8[t];
            norms[i] = s;
        }
        if (added)
            hip_check(hipMemcpy(d_rownorm_.as<int32_t>() + first, norms.data(), added * 4, hipMemcpyHostToDevice), "row norms");
    }
    if (!first) dg_ = HnswDeviceGraph{};
    dg_.rows = d_rows_.ptr();
    dg_.row_norm = d_rownorm_.as<int32_t>();
    dg_.ext_ids = d_ids_.as<int32_t>();
    dg_.n = (int)n;
    dg_.dim = (int)dim_;
    dg_.ldv = is_u8() ? 128 : ldb_;
    dg_.space = sspace;
    dg_.normalize_query = normalize ? 1 : 0;
}

void Engine::upload_graph() {
    const HostGraph& g = graph_;
    const size_t n = (size_t)g.n;
    d_links0_.ensure(std::max<size_t>(g.links0.size(), 1) * 4);
    d_up_off_.ensure(std::max<size_t>(n, 1) * 8);
    d_up_links_.ensure(std::max<size_t>(g.up_links.size(), 1) * 4);
    if (n) {
        hip_check(hipMemcpy(d_links0_.ptr(), g.links0.data(), g.links0.size() * 4, hipMemcpyHostToDevice), "links0");
        hip_check(hipMemcpy(d_up_off_.ptr(), g.up_off.data(), n * 8, hipMemcpyHostToDevice), "up_off");
        if (!g.up_links.empty())
            hip_check(hipMemcpy(d_up_links_.ptr(), g.up_links.data(), g.up_links.size() * 4, hipMemcpyHostToDevice),
                      "up_links");
    }
    prepare_graph_rows();
    bind_graph_buffers();
    dg_.maxM = g.maxM;
    dg_.maxM0 = g.maxM0;
    dg_.maxlevel = g.maxlevel;
    dg_.enterpoint = g.enterpoint;
    hip_check(hipStreamSynchronize(stream_), "graph upload");
}

// dg_ names the graph's three buffers (after they were allocated, or grew and moved)
void Engine::bind_graph_buffers() {
    dg_.links0 = d_links0_.as<int32_t>();
    dg_.up_off = d_up_off_.as<int64_t>();
    dg_.up_links = d_up_links_.as<int32_t>();
}

// largest |element| of the resident rows [first, n)
float Engine::rows_max_abs(size_t first, size_t n) {
    DevBuf d_bm;
    d_bm.ensure(16);
    float bm[4] = {0.f, 0.f, 0.f, 0.f};  // [2]: largest |element|
    hip_check(launch_row_maxnorm(d_rows_.as<float>() + first * (size_t)ldb_, (int)(n - first), ldb_, (int)dim_, false,
                                 d_bm.as<float>(), stream_),
              "fp16 rows: range");
    hip_check(hipMemcpyAsync(bm, d_bm.ptr(), 16, hipMemcpyDeviceToHost, stream_), "fp16 rows: range");
    hip_check(hipStreamSynchronize(stream_), "fp16 rows: range");
    return bm[2];
}

// The fp16 traversal copy of the rows the search kernels read (cosine on the optimized index: the normalised rows), scaled by
// one power of two per index (f16_pack.hpp).  An index that cannot spare the HBM keeps working on its f32 rows.
bool Engine::ensure_rows16() {
    if (dg_.rows16) return true;
    if (rows16_failed_ || is_u8() || d_n_ == 0 || !dg_.rows) return false;
    const size_t n = d_n_;
    const int ld16 = (int)f16pack::row_stride(dim_);
    int e = 0;
    try {
        rows16_max_ = rows_max_abs(0, n);
        e = f16pack::scale_exp(rows16_max_);
        d_rows16_.ensure(n * (size_t)ld16 * 2);
        pack_rows16(0, n, e);
    } catch (const EngineError& x) {
        if (x.code != Err::OutOfMemory) throw;
        d_rows16_.release();  // (nothing partial stays behind)
        rows16_failed_ = true;
        return false;
    }
    dg_.rows16 = d_rows16_.ptr();
    dg_.ld16 = ld16;
    dg_.inv_scale16 = f16pack::scale_of(-e);
    rows16_exp_ = e;
    return true;
}

void Engine::pack_rows16(size_t first, size_t n, int e) {
    const size_t ld16 = f16pack::row_stride(dim_);
    hip_check(launch_hnsw_pack_rows16(d_rows_.as<float>() + first * (size_t)ldb_, (int)(n - first), ldb_, (int)dim_,
                                      f16pack::scale_of(e), d_rows16_.as<uint16_t>() + first * ld16, (int)ld16, stream_),
              "fp16 rows");
    hip_check(hipStreamSynchronize(stream_), "fp16 rows");
}

void Engine::ensure_graph() {
    if (method_ != Method::Hnsw || !graph_dirty_) return;
    if (str_space_) {
        build_string_graph();
        graph_dirty_ = false;
        return;
    }
    if (use_gpu_build() || (!parent_ && (shards_.size() > 1 || (dirty_ && resolve_shards() > 1)))) {
        finalize();
        return;
    }
    build_graph();
    graph_dirty_ = false;
}

void Engine::finalize() {
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (!dirty_) return;
    finalize_index();
    // the graph holds the deleted rows as before (a rebuild too: positions do not move), so they stay marked; rows that came
    // since are live
    if (method_ == Method::Hnsw && n_dead_ > 0) upload_tombstones();
}

void Engine::finalize_index() {
    if (have_last_) {   // batches in flight read the rows that are replaced here
        check_device();
        order_after_last(stream_);
    }
    if (sparse_) {
        upload_sparse();
        dirty_ = false;
        return;
    }
    if (str_space_) {
        upload_strings();
        dirty_ = false;
        return;
    }
    if (diverg_) {
        upload_diverg();
        dirty_ = false;
        return;
    }
    if (!parent_) {
        const int nsh = resolve_shards();
        if (nsh > 1) {
            finalize_sharded(nsh);
            dirty_ = false;
            graph_dirty_ = false;
            return;
        }
        shards_.clear();
    }
    if (method_ == Method::Hnsw && graph_dirty_ && use_gpu_build()) {
        check_device();
        if (can_append() && append_rows_gpu()) {
            graph_dirty_ = false;
            dirty_ = false;
            return;
        }
        upload_rows();
        build_graph_gpu();
        graph_dirty_ = false;
        dirty_ = false;
        if (rows_f16_index_) (void)ensure_rows16();
        return;
    }
    ensure_graph();  // host-side construction first: it needs no device
    check_device();
    upload_rows();
    if (method_ == Method::Brute) prepare_brute();
    else upload_graph();
    dirty_ = false;
    if (method_ == Method::Hnsw && rows_f16_index_) (void)ensure_rows16();
}

// ---------------------------------------------------------------------------------------------
// Row shards behind one handle: shard s owns rows [s*n/S, (s+1)*n/S) on device (base + s) % count,
// with its own workspaces, stream and (HNSW) graph.  A query batch goes to every shard; per-shard top-k lists are
// copied peer-to-peer to the primary device and merged there by (distance, global position) -- for the exact scan
// that is bit for bit the unsharded result.  Nothing here needs torch or RCCL: the caller of nmslib_knn_query_batch
// gets all GPUs of the node.  Shards hold windows of this engine's host rows, not copies.
// ---------------------------------------------------------------------------------------------
int Engine::resolve_shards() const {
    if (loaded_graph_ || parent_ || ids_.empty()) return 1;
    if (n_dead_) return 1;  // deleted rows are served on one device (delete_ids refuses an index that asked for shards)
    int want = gpu_shards_;
    if (want < 0) {
        if (const char* env = getenv("NMSLIB_GPU_SHARDS")) want = atoi(env);
        // a process that was given its device (one rank per GPU, bench.py) keeps to it
        else if (getenv("NMSLIB_GPU_DEVICE") || getenv("LOCAL_RANK")) return 1;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return 1;  // finalize() reports the missing device
    }
    const size_t n = ids_.size();
    if (want < 0) {
        // automatic: the exact scan only -- sharded it returns the unsharded result bit for bit.  One HNSW graph per
        // GPU changes ids and recall with the number of visible devices and cannot be saved in the reference's
        // single-graph file, so HNSW is sharded only when gpu_shards / NMSLIB_GPU_SHARDS ask for it.
        if (method_ != Method::Brute) return 1;
        want = (int)std::min<size_t>((size_t)count, std::max<size_t>(1, n / 1000000));  // 1M rows per shard
    } else if (want == 0) want = count;
    if ((size_t)want > n) want = (int)n;
    return std::max(1, want);
}

void Engine::finalize_sharded(int nshards) {
    check_device();  // primary device: queries arrive there, results are merged there
    int count = 1;
    hip_check(hipGetDeviceCount(&count), "hipGetDeviceCount");
    const size_t n = ids_.size();
    shards_.clear();
    for (int s = 0; s < nshards; ++s) {
        std::unique_ptr<Engine> c(new Engine(space_name_, method_name_, is_u8() ? 2 : 0, 0));
        c->parent_ = this;
        c->view_lo_ = n * (size_t)s / (size_t)nshards;
        c->view_n_ = n * (size_t)(s + 1) / (size_t)nshards - c->view_lo_;
        c->dim_ = dim_;
        c->method_ = method_;
        c->bp_ = bp_;
        c->rows_f16_index_ = c->rows_f16_ = rows_f16_index_;
        c->created_ = true;
        c->forced_device_ = (device_ + s) % count;
        shards_.push_back(std::move(c));
    }
    // build all shards at once: every shard has its own device (or at least its own stream)
    std::vector<std::string> errors((size_t)nshards);
    std::vector<std::thread> th;
    auto t0 = clk::now();
    for (int s = 0; s < nshards; ++s)
        th.emplace_back([&, s] {
            try {
                shards_[(size_t)s]->finalize();
            } catch (const std::exception& e) {
                errors[(size_t)s] = e.what();
                if (errors[(size_t)s].empty()) errors[(size_t)s] = "failed";
            }
        });
    for (auto& t : th) t.join();
    for (int s = 0; s < nshards; ++s)
        if (!errors[(size_t)s].empty()) {
            shards_.clear();
            throw EngineError(Err::IndexBuildFailed, "shard " + std::to_string(s) + ": " + errors[(size_t)s]);
        }
    build_seconds = std::chrono::duration<double>(clk::now() - t0).count();
    rows_uploaded = n;
    rows_appended = 0;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    d_ids_.ensure(std::max<size_t>(n, 1) * 4);  // position -> external id, applied after the merge
    hip_check(hipMemcpy(d_ids_.ptr(), ids_.data(), n * 4, hipMemcpyHostToDevice), "upload ids");
    d_n_ = n;
    shard_events_.clear();  // (made again at their first record, each on its shard's device)
    shard_events_.resize((size_t)nshards);
}

void Engine::knn_sharded(const void* d_queries, size_t nq, size_t elem_count, size_t k, int32_t* d_ids, float* d_dists,
                         int32_t* d_cnt, hipStream_t stream) {
    const size_t S = shards_.size();
    const size_t qbytes = nq * elem_count * elem_bytes();
    have_counters_ = false;
    DeviceGuard guard(device_);  // an exception thrown by a shard must not leave this thread on the shard's device
    ws_sh_ids_.ensure(S * nq * k * 4);
    ws_sh_d_.ensure(S * nq * k * 4);
    shard_ready_.record(stream);  // the queries are ready on the caller's stream
    for (size_t s = 0; s < S; ++s) {
        Engine& c = *shards_[s];
        hip_check(hipSetDevice(c.device_), "hipSetDevice");
        c.ef_ = ef_;
        c.algo_ = algo_;
        c.rows_f16_ = rows_f16_;
        c.rerank_ = rerank_;
        c.inwalk_ = inwalk_;
        shard_ready_.stream_wait(c.stream_);
        const void* q = d_queries;
        if (c.device_ != device_) {
            c.ws_q_.ensure(qbytes);
            hip_check(hipMemcpyPeerAsync(c.ws_q_.ptr(), c.device_, d_queries, device_, qbytes, c.stream_), "queries P2P");
            q = c.ws_q_.ptr();
        }
        c.ws_ids_.ensure(nq * k * 4);
        c.ws_dists_.ensure(nq * k * 4);
        c.knn_device(q, nq, elem_count, k, c.ws_ids_.as<int32_t>(), c.ws_dists_.as<float>(), nullptr, c.stream_);
        hip_check(hipMemcpyPeerAsync(ws_sh_ids_.as<int32_t>() + s * nq * k, device_, c.ws_ids_.ptr(), c.device_, nq * k * 4,
                                     c.stream_),
                  "ids P2P");
        hip_check(hipMemcpyPeerAsync(ws_sh_d_.as<float>() + s * nq * k, device_, c.ws_dists_.ptr(), c.device_, nq * k * 4,
                                     c.stream_),
                  "dists P2P");
        shard_events_[s].record(c.stream_);
        // NMSLIB_GPU_SHARD_SERIAL=1 (diagnostics): one shard at a time instead of all shards' kernels side by side
        static const bool serial = getenv("NMSLIB_GPU_SHARD_SERIAL") && atoi(getenv("NMSLIB_GPU_SHARD_SERIAL"));
        if (serial) hip_check(hipStreamSynchronize(c.stream_), "shard (serial)");
    }
    hip_check(hipSetDevice(device_), "hipSetDevice");
    last_path = shards_[0]->last_path;  // every shard takes the same path for the same batch shape
    for (size_t s = 0; s < S; ++s) shard_events_[s].stream_wait(stream);
    hip_check(launch_merge_topk_ex(ws_sh_d_.as<float>(), ws_sh_ids_.as<int32_t>(), nq * k, (int)S, (int)nq, (int)k, d_dists,
                                   d_ids, d_cnt, d_ids_.as<int32_t>(), stream),
              "merge_topk");
}

// ---------------------------------------------------------------------------------------------
// Queries
// ---------------------------------------------------------------------------------------------
void Engine::knn_device(const void* d_queries, size_t nq, size_t elem_count, size_t k, int32_t* d_ids,
                        float* d_dists, int32_t* d_cnt, hipStream_t stream, Filter* f) {
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (f) check_filter(f);
    if (diverg_)
        throw EngineError(Err::SpaceIncompatible, "the device-resident batch is not served over a divergence space: a "
                                                  "query's logarithms are taken on the host, so divergence queries "
                                                  "go through nmslib_knn_query_batch");
    if (dirty_) finalize();
    check_device();
    if (nq == 0) return;
    if (k == 0) throw EngineError(Err::InvalidArgument, "k must be positive");
    if (sparse_ || str_space_)
        throw EngineError(Err::SpaceIncompatible, "the device-resident batch takes dense queries; sparse and string "
                                                  "queries go through nmslib_knn_query_batch");
    if (f) filter_begin_batch(*f);
    order_after_last(stream);   // (row shards: the parent's stream; every child keeps to its own)
    if (!shards_.empty()) {
        if (size() > 0 && elem_count != dim_)
            throw EngineError(Err::QueryExecutionFailed, "query dimension does not match the index");
        knn_sharded(d_queries, nq, elem_count, k, d_ids, d_dists, d_cnt, stream);
        return;
    }
    if (d_n_ > 0 && elem_count != dim_)
        // SpaceLp::HiddenDistance CHECKs equal lengths (space_lp.cc:27-35) -> the query fails
        throw EngineError(Err::QueryExecutionFailed, "query dimension does not match the index");
    // very large batches go through in slices: the per-query workspaces (candidate buffers, visited bitsets)
    // stay bounded and every slice still fills the chip (the work counters then describe the last slice)
    const size_t slice = method_ == Method::Brute ? 32768 : 65536;
    const size_t qbytes = elem_count * elem_bytes();
    HnswOut out{};
    if (method_ == Method::Hnsw) {  // results and work counters of the WHOLE batch (a slice gets out.at(q0, k))
        for (DevBuf* b : {&ws_ndc_, &ws_hops_, &ws_hops_up_, &sw_.status}) b->ensure(nq * 4);
        if (!d_cnt) sw_.outcnt.ensure(nq * 4);  // the counts go to a workspace when the caller asks for none
        out = {d_ids, d_dists, d_cnt ? d_cnt : sw_.outcnt.as<int32_t>(), ws_ndc_.as<int32_t>(), ws_hops_.as<int32_t>(),
               ws_hops_up_.as<int32_t>(), sw_.status.as<int32_t>()};
    }
    for (size_t q0 = 0; q0 < nq; q0 += slice) {
        const size_t m = std::min(slice, nq - q0);
        const void* qs = static_cast<const char*>(d_queries) + q0 * qbytes;
        int32_t* cnt = d_cnt ? d_cnt + q0 : nullptr;
        if (method_ == Method::Hnsw) {
            if (f) knn_hnsw_filtered(*f, qs, m, k, out.at(q0, k), stream);
            else knn_hnsw(qs, m, k, out.at(q0, k), stream);
        } else if (f) knn_filtered_slice(*f, qs, m, k, d_ids + q0 * k, d_dists + q0 * k, cnt, stream);
        else knn_brute(qs, m, k, d_ids + q0 * k, d_dists + q0 * k, cnt, stream);
    }
}

void Engine::fast_tile_counts(size_t* tiles, size_t* precise, size_t* fallback) {
    *tiles = *precise = *fallback = 0;
    if (!shards_.empty()) {   // row shards: every shard sees the same batch; the first one's counters stand for the handle
        shards_[0]->fast_tile_counts(tiles, precise, fallback);
        return;
    }
    const int path = stats_path();
    if ((path != 1 && path != 3 && path != 6) || !fast_flags_ || fast_nqt_ <= 0) return;
    std::vector<int> h((size_t)fast_nqt_ * 2, 0);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipStreamSynchronize(last_stream_ ? last_stream_ : stream_), "stats");
    hip_check(hipMemcpy(h.data(), fast_flags_, (size_t)fast_nqt_ * (fast_has_precise_ ? 2 : 1) * sizeof(int), hipMemcpyDeviceToHost),
              "stats flags");
    *tiles = (size_t)fast_nqt_;
    for (int i = 0; i < fast_nqt_; ++i) {
        *fallback += h[i] != 0;
        if (fast_has_precise_) *precise += h[(size_t)fast_nqt_ + i] != 0;
    }
}

// The result block of a host batch: ids | dists | counts in ONE device block (ws_ids_), so that one D2H brings it
// into the pinned block.
Engine::ResultBlock Engine::result_block(size_t nq, size_t k) {
    ws_ids_.ensure(2 * nq * k * 4 + nq * 4);
    int32_t* d_ids = ws_ids_.as<int32_t>();
    return {d_ids, reinterpret_cast<float*>(d_ids + nq * k), d_ids + 2 * nq * k};
}

// ... copied into the pinned block (the caller sized it for the batch: its queries were staged there), after the
// stream's work; the pointers stay valid until the next call
void Engine::fetch_results(size_t nq, size_t k, const char* what, const int32_t** ids, const float** dists,
                           const int32_t** cnt) {
    const size_t rbytes = nq * k * 4;
    char* hp = static_cast<char*>(pinned_.ptr());
    hip_check(hipMemcpyAsync(hp, ws_ids_.ptr(), 2 * rbytes + nq * 4, hipMemcpyDeviceToHost, stream_), "results D2H");
    hip_check(hipStreamSynchronize(stream_), what);
    *ids = reinterpret_cast<const int32_t*>(hp);
    *dists = reinterpret_cast<const float*>(hp + rbytes);
    *cnt = reinterpret_cast<const int32_t*>(hp + 2 * rbytes);
}

// Exact scan of a batch over sparse or string rows.  Batches go through in slices of queries: the per-split lists
// ([nsplit][queries][k] keys) stay bounded.  launch(plan, q0, split_d, split_pos) enqueues the scan of the slice that
// starts at query q0; its lists are merged into `out`, positions mapped to external ids.
void Engine::scan_slices(size_t nq, size_t k, int tq, const ResultBlock& out, const ScanLaunch& launch) {
    const int n = (int)d_n_;
    const size_t max_split_keys = (size_t)1 << 25;  // 256 MiB of per-split lists at most (one query always fits)
    for (size_t q0 = 0; q0 < nq;) {
        int m = (int)std::min<size_t>(32768, nq - q0);
        ScanPlan p = scan_make_plan(n, m, (int)k, tq);
        while (m > 1 && (size_t)p.nsplit * m * k > max_split_keys) {
            m = std::max(1, m / 2);
            p = scan_make_plan(n, m, (int)k, tq);
        }
        const size_t keys = (size_t)p.nsplit * m * k;
        ws_split_.ensure(keys * 8);
        float* split_d = ws_split_.as<float>();
        int32_t* split_pos = reinterpret_cast<int32_t*>(split_d + keys);
        prof_begin(stream_);
        launch(p, q0, split_d, split_pos);
        hip_check(launch_merge_topk_ex(split_d, split_pos, (size_t)m * k, p.nsplit, m, (int)k, out.dists + q0 * k,
                                       out.ids + q0 * k, out.cnt + q0, d_ids_.as<int32_t>(), stream_),
                  "scan merge");
        prof_end(stream_);
        q0 += (size_t)m;
    }
}

// the one place a divergence query's length is checked: the objects of a pair must be equally long
void Engine::check_diverg_query_length(size_t elem_count, size_t dim) {
    if (elem_count != dim)
        throw EngineError(Err::InvalidArgument, "query length " + std::to_string(elem_count) +
                                                    " does not match the rows' length " + std::to_string(dim));
}

void Engine::knn_host(const void* queries, size_t nq, size_t elem_count, size_t k, const int32_t** ids, const float** dists,
                      const int32_t** cnt, Filter* f) {
    if (!created_) throw EngineError(Err::IndexBuildFailed, "Index not built");
    if (f) check_filter(f);  // (refused before the index is finalized for it)
    if (diverg_ && !ids_.empty()) check_diverg_query_length(elem_count, dim_);  // refused before any device work
    if (dirty_) finalize();
    check_device();
    if (diverg_) {
        order_after_last(stream_);
        return knn_diverg_host(static_cast<const float*>(queries), nq, elem_count, k, ids, dists, cnt);
    }
    const size_t qbytes = nq * elem_count * elem_bytes();
    // device: queries | ids | dists | counts in ONE block each way; host: one pinned block
    ws_q_.ensure(qbytes);
    const ResultBlock out = result_block(nq, k);
    char* hp = static_cast<char*>(pinned(std::max(qbytes, 2 * nq * k * 4 + nq * 4)));
    std::memcpy(hp, queries, qbytes);
    order_after_last(stream_);
    hip_check(hipMemcpyAsync(ws_q_.ptr(), hp, qbytes, hipMemcpyHostToDevice, stream_), "queries H2D");
    knn_device(ws_q_.ptr(), nq, elem_count, k, out.ids, out.dists, out.cnt, stream_, f);
    fetch_results(nq, k, "knn", ids, dists, cnt);
}

// *d_out, after the stream's work
float Engine::read_float(const float* d_out, const char* what) {
    float v = 0;
    hip_check(hipMemcpyAsync(&v, d_out, 4, hipMemcpyDeviceToHost, stream_), "pair D2H");
    hip_check(hipStreamSynchronize(stream_), what);
    return v;
}

float Engine::pair_distance(size_t p1, size_t p2) {
    // Space::IndexTimeDistance on the ORIGINAL rows (nmslib_c.cpp:1166), one wave on the GPU
    if (sparse_) return pair_distance_sparse(p1, p2);
    if (str_space_) return pair_distance_string(p1, p2);
    if (diverg_) return pair_distance_diverg(p1, p2);
    check_device();
    const size_t rb = is_u8() ? 128 : (size_t)f32_row_stride((int)dim_) * 4;
    ws_pair_.ensure(2 * rb + 16);
    order_after_last(stream_);
    hip_check(hipMemsetAsync(ws_pair_.ptr(), 0, 2 * rb + 16, stream_), "pair clear");
    char* base = ws_pair_.as<char>();
    hip_check(hipMemcpyAsync(base, host_row(p1), row_bytes(), hipMemcpyHostToDevice, stream_), "pair H2D");
    hip_check(hipMemcpyAsync(base + rb, host_row(p2), row_bytes(), hipMemcpyHostToDevice, stream_), "pair H2D");
    float* out = reinterpret_cast<float*>(base + 2 * rb);
    hip_check(launch_pair_distance(space_, base, base + rb, (int)dim_, out, stream_), "pair_distance");
    return read_float(out, "pair_distance");
}

// ---------------------------------------------------------------------------------------------
// Persistence: the reference's own formats
//   <path>      optimized HNSW index, hnsw.cc:774-806 / 1025-1074
//   <path>.dat  object vector, space.cc:88-105
// ---------------------------------------------------------------------------------------------
template <typename T>
static void wr(std::ostream& o, const T& v) {
    o.write(reinterpret_cast<const char*>(&v), sizeof(T));
}
template <typename T>
static void rd(std::istream& i, T& v) {
    i.read(reinterpret_cast<char*>(&v), sizeof(T));
    if (!i) throw EngineError(Err::DataIO, "unexpected end of index file");
}

void Engine::save(const std::string& path, bool save_data) {
    if (!created_) throw EngineError(Err::InvalidArgument, "Index not built");
    if (str_space_)  // SeqSearch has no SaveIndex (include/index.h:56-58); the object file is not written either
        throw EngineError(Err::DataIO, "SaveIndex is not implemented for method: Sequential search (string index; "
                                       "the data file is not written)");
    if (diverg_)  // SeqSearch has no SaveIndex (include/index.h:56-58); the object file is not written either
        throw EngineError(Err::DataIO, "SaveIndex is not implemented for method: Sequential search (divergence index; "
                                       "the data file is not written)");
    if (sparse_)  // SeqSearch has no SaveIndex (include/index.h:56-58); the object file is not written either
        throw EngineError(Err::DataIO, "SaveIndex is not implemented for method: Sequential search (sparse index; "
                                       "the data file is not written)");
    if (n_dead_)  // (before anything is written: a file without the marks would bring the rows back at load)
        throw EngineError(Err::DataIO, "the index has " + std::to_string(n_dead_) + " deleted rows and neither file format "
                                       "(the index file, the .dat object file) has a place for deleted rows; nothing is "
                                       "written");
    if (method_ == Method::Hnsw && !loaded_graph_ && (shards_.size() > 1 || (dirty_ && resolve_shards() > 1)))
        throw EngineError(Err::DataIO, "a sharded HNSW index holds one graph per GPU and has no single-file form; "
                                       "build with gpu_shards=1 to save it in the reference's format");
    ensure_graph();  // persistence is host-side: no device needed
    sync_host_graph();  // (but for the lists of a graph that grew on the device)
    const size_t n = ids_.size();
    if (save_data) {
        std::ofstream out(path + ".dat", std::ios::binary);
        if (!out) throw EngineError(Err::DataIO, "Cannot open file '" + path + ".dat' for writing");
        wr(out, (uint64_t)n);
        std::vector<char> buf(16 + stored_row_bytes());
        for (size_t i = 0; i < n; ++i) {
            const uint64_t len = 16 + stored_row_bytes();
            wr(out, len);
            const int32_t id = ids_[i], label = -1;
            const uint64_t dl = stored_row_bytes();
            std::memcpy(&buf[0], &id, 4);
            std::memcpy(&buf[4], &label, 4);
            std::memcpy(&buf[8], &dl, 8);
            stored_row(i, &buf[16]);
            out.write(buf.data(), (std::streamsize)buf.size());
        }
        if (!out) throw EngineError(Err::DataIO, "write failed: " + path + ".dat");
    }
    if (method_ != Method::Hnsw)
        // Index::SaveIndex default throws for SeqSearch (include/index.h:56-58)
        throw EngineError(Err::DataIO, "SaveIndex is not implemented for method: Sequential search");
    int dist_func = -1;
    if (!bp_.skip_optimized) {
        if (space_ == SP_L2) dist_func = (dim_ % 16 == 0) ? 1 : 2;
        else if (space_ == SP_COSINE) dist_func = 3;
        else if (space_ == SP_NEGDOT) dist_func = 4;
        else if (space_ == SP_L1) dist_func = 5;
        else if (space_ == SP_LINF) dist_func = 6;
    }
    std::ofstream out(path, std::ios::binary);
    if (!out) throw EngineError(Err::DataIO, "Cannot open file '" + path + "' for writing");
    const HostGraph& g = graph_;
    if (dist_func < 0) {
        // regular (non-optimized) index, SaveRegularIndexBin hnsw.cc:808-840
        wr(out, (uint32_t)0);
        wr(out, (uint32_t)n);
        wr(out, (int32_t)g.maxlevel);
        wr(out, (uint32_t)g.enterpoint);
        wr(out, (uint64_t)g.M);
        wr(out, (uint64_t)g.maxM);
        wr(out, (uint64_t)g.maxM0);
        for (size_t i = 0; i < n; ++i) {
            wr(out, (uint32_t)g.levels[i]);
            for (int l = 0; l <= g.levels[i]; ++l) {
                const int32_t* L = l == 0 ? &g.links0[i * (g.maxM0 + 1)]
                                          : &g.up_links[g.up_off[i] + (size_t)(l - 1) * (g.maxM + 1)];
                wr(out, (uint32_t)L[0]);
                out.write(reinterpret_cast<const char*>(L + 1), (std::streamsize)L[0] * 4);
            }
        }
    } else {
        const uint64_t data_section = 16 + dim_ * 4;
        const uint64_t mem_per_obj = data_section + (uint64_t)(g.maxM0 + 1) * 4;
        wr(out, (uint32_t)1);
        wr(out, (uint32_t)n);
        wr(out, mem_per_obj);
        wr(out, data_section);   // offsetLevel0_
        wr(out, (uint64_t)0);    // offsetData_
        wr(out, (int32_t)g.maxlevel);
        wr(out, (uint32_t)g.enterpoint);
        wr(out, (uint64_t)g.maxM);
        wr(out, (uint64_t)g.maxM0);
        wr(out, (int32_t)dist_func);
        wr(out, (uint64_t)3);    // searchMethod_
        std::vector<char> rec(mem_per_obj);
        std::vector<float> row(dim_), resident;
        const bool from_device = fetch_resident_rows(resident);  // (a consolidated cosine graph: normalised already)
        for (size_t i = 0; i < n; ++i) {
            const int32_t id = ids_[i], label = -1;
            const uint64_t dl = dim_ * 4;
            std::memcpy(&rec[0], &id, 4);
            std::memcpy(&rec[4], &label, 4);
            std::memcpy(&rec[8], &dl, 8);
            const float* src = from_device ? &resident[i * dim_]
                               : (loaded_graph_ && !graph_rows_.empty()) ? &graph_rows_[i * dim_] : &rows_f32_[i * dim_];
            std::memcpy(row.data(), src, dim_ * 4);
            if (space_ == SP_COSINE && !from_device && !(loaded_graph_ && !graph_rows_.empty())) {
                float s = 0;  // NormalizeVect, hnsw.h:486-497
                for (size_t d = 0; d < dim_; ++d) s += row[d] * row[d];
                if (s != 0.0f) {
                    s = 1 / std::sqrt(s);
                    for (size_t d = 0; d < dim_; ++d) row[d] *= s;
                }
            }
            std::memcpy(&rec[16], row.data(), dim_ * 4);
            std::memcpy(&rec[data_section], &g.links0[i * (g.maxM0 + 1)], (size_t)(g.maxM0 + 1) * 4);
            out.write(rec.data(), (std::streamsize)rec.size());
        }
        for (size_t i = 0; i < n; ++i) {
            const uint32_t bytes = (uint32_t)((size_t)g.levels[i] * (g.maxM + 1) * 4);
            wr(out, bytes);
            if (bytes) out.write(reinterpret_cast<const char*>(&g.up_links[g.up_off[i]]), bytes);
        }
    }
    // Trailer (ignored by the reference's readers, which stop after the last node): lets this
    // library restore the space of an index it saved itself; the reference hard-codes "l2"
    // on load (nmslib_c.cpp:1421-1429).
    char trailer[32] = {0};
    std::memcpy(trailer, "GFXKNNv1", 8);
    std::strncpy(trailer + 8, space_name_.c_str(), 23);
    out.write(trailer, 32);
    if (!out) throw EngineError(Err::DataIO, "write failed: " + path);
}

std::unique_ptr<Engine> Engine::load(const std::string& path, int data_type, int dist_type, bool load_data) {
    std::ifstream in(path, std::ios::binary);
    if (!in) throw EngineError(Err::DataIO, "Cannot open file '" + path + "' for reading");
    std::string saved_space;
    {
        in.seekg(0, std::ios::end);
        const std::streamoff sz = in.tellg();
        if (sz >= 36) {
            char trailer[32];
            in.seekg(sz - 32);
            in.read(trailer, 32);
            if (std::memcmp(trailer, "GFXKNNv1", 8) == 0) {
                trailer[31] = 0;
                saved_space = trailer + 8;
            }
        }
        in.clear();
        in.seekg(0);
    }
    uint32_t flag = 0;
    rd(in, flag);
    std::unique_ptr<Engine> e;
    // objects first (.dat), as nmslib_load_index does when load_data is set (nmslib_c.cpp:1430-1434)
    std::vector<int32_t> dat_ids;
    std::vector<char> dat_payload;
    size_t dat_len = 0;
    if (load_data) {
        std::ifstream d(path + ".dat", std::ios::binary);
        if (!d) throw EngineError(Err::DataIO, "Cannot open file '" + path + ".dat' for reading");
        uint64_t qty = 0;
        rd(d, qty);
        for (uint64_t i = 0; i < qty; ++i) {
            uint64_t osz = 0;
            rd(d, osz);
            std::vector<char> buf(osz);
            d.read(buf.data(), (std::streamsize)osz);
            if (!d || osz < 16) throw EngineError(Err::DataIO, "corrupt .dat file");
            int32_t id;
            uint64_t dl;
            std::memcpy(&id, &buf[0], 4);
            std::memcpy(&dl, &buf[8], 8);
            if (i == 0) dat_len = dl;
            if (dl != dat_len || dl + 16 != osz) throw EngineError(Err::DataIO, "ragged .dat file");
            dat_ids.push_back(id);
            dat_payload.insert(dat_payload.end(), buf.begin() + 16, buf.end());
        }
    }
    if (flag == 1) {
        uint32_t n;
        uint64_t mem_per_obj, off_l0, off_data, maxM, maxM0, search_method;
        int32_t maxlevel, dist_func;
        uint32_t enterpoint;
        rd(in, n); rd(in, mem_per_obj); rd(in, off_l0); rd(in, off_data); rd(in, maxlevel); rd(in, enterpoint);
        rd(in, maxM); rd(in, maxM0); rd(in, dist_func); rd(in, search_method);
        const char* space = nullptr;
        switch (dist_func) {  // DistFuncType, hnsw.h:50-58
            case 1: case 2: space = "l2"; break;
            case 3: space = "cosinesimil"; break;
            case 4: space = "negdotprod"; break;
            case 5: space = "l1"; break;
            case 6: space = "linf"; break;
            default: throw EngineError(Err::DataIO, "Unknown distance function code in index file");
        }
        if (data_type != 0) throw EngineError(Err::DataIO, "an optimized HNSW index holds dense float vectors");
        if (off_l0 < off_data + 16 || mem_per_obj < off_l0 + (maxM0 + 1) * 4 || maxM0 > 8192 || maxM > 4096)
            throw EngineError(Err::DataIO, "unsupported optimized index geometry");
        e.reset(new Engine(space, "hnsw", data_type, dist_type));
        const size_t dim = (off_l0 - off_data - 16) / 4;
        e->dim_ = dim;
        HostGraph& g = e->graph_;
        g.n = (int)n;
        g.maxM = (int)maxM;
        g.M = (int)maxM;
        g.maxM0 = (int)maxM0;
        g.maxlevel = maxlevel;
        g.enterpoint = (int)enterpoint;
        g.levels.assign(n, 0);
        g.links0.assign((size_t)n * (maxM0 + 1), 0);
        g.up_off.assign(n, -1);
        e->graph_rows_.resize((size_t)n * dim);
        e->ids_.resize(n);
        std::vector<char> rec(mem_per_obj);
        for (uint32_t i = 0; i < n; ++i) {
            in.read(rec.data(), (std::streamsize)mem_per_obj);
            if (!in) throw EngineError(Err::DataIO, "truncated index file");
            std::memcpy(&e->ids_[i], &rec[off_data], 4);  // Object header id (object.h:61-77)
            std::memcpy(&e->graph_rows_[(size_t)i * dim], &rec[off_data + 16], dim * 4);
            int32_t cnt;
            std::memcpy(&cnt, &rec[off_l0], 4);
            if (cnt < 0 || (uint64_t)cnt > maxM0) throw EngineError(Err::DataIO, "corrupt level-0 list");
            std::memcpy(&g.links0[(size_t)i * (maxM0 + 1)], &rec[off_l0], (size_t)(cnt + 1) * 4);
        }
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t bytes;
            rd(in, bytes);
            if (!bytes) continue;
            const size_t ints = bytes / 4;
            g.levels[i] = (int)(ints / (maxM + 1));  // the level is not stored: SURVEY.md 8f N1
            g.up_off[i] = (int64_t)g.up_links.size();
            const size_t at = g.up_links.size();
            g.up_links.resize(at + ints);
            in.read(reinterpret_cast<char*>(&g.up_links[at]), bytes);
            if (!in) throw EngineError(Err::DataIO, "truncated index file");
            for (size_t l = 0; l < ints / (maxM + 1); ++l) {  // zero the uninitialised tail slots
                int32_t* L = &g.up_links[at + l * (maxM + 1)];
                for (uint64_t j = (uint64_t)L[0] + 1; j <= maxM; ++j) L[j] = 0;
            }
        }
        e->bp_.M = e->bp_.maxM = (int)maxM;
        e->bp_.maxM0 = (int)maxM0;
        e->method_ = Method::Hnsw;
        if (load_data && !dat_ids.empty()) {
            if (dat_ids.size() != n || dat_len != dim * 4) throw EngineError(Err::DataIO, ".dat does not match the index");
            e->rows_f32_.resize((size_t)n * dim);
            std::memcpy(e->rows_f32_.data(), dat_payload.data(), dat_payload.size());
        } else {
            e->rows_f32_ = e->graph_rows_;  // rows as stored in the index (cosine: normalised)
        }
    } else {
        // regular index: graph only, rows must come from .dat (LoadRegularIndexBin, hnsw.cc:941-991)
        if (!load_data || dat_ids.empty()) throw EngineError(Err::DataIO, "a regular HNSW index needs its .dat file");
        uint32_t n, enterpoint;
        int32_t maxlevel;
        uint64_t M, maxM, maxM0;
        rd(in, n); rd(in, maxlevel); rd(in, enterpoint); rd(in, M); rd(in, maxM); rd(in, maxM0);
        if (n != dat_ids.size()) throw EngineError(Err::DataIO, "The number of stored elements doesn't match the data");
        const bool u8 = data_type == 2;
        // like the reference, a float index without further information is taken to be "l2"
        e.reset(new Engine(u8 ? "l2sqr_sift" : (saved_space.empty() ? "l2" : saved_space.c_str()), "hnsw", data_type,
                           dist_type));
        if (u8) {
            if (dat_len != 132) throw EngineError(Err::DataIO, "unexpected SIFT payload size");
            e->dim_ = 128;
            e->rows_u8_.resize((size_t)n * 128);
            for (uint32_t i = 0; i < n; ++i) std::memcpy(&e->rows_u8_[(size_t)i * 128], &dat_payload[(size_t)i * 132], 128);
        } else {
            e->dim_ = dat_len / 4;
            e->rows_f32_.resize((size_t)n * e->dim_);
            std::memcpy(e->rows_f32_.data(), dat_payload.data(), dat_payload.size());
        }
        e->ids_ = dat_ids;
        HostGraph& g = e->graph_;
        g.n = (int)n;
        g.M = (int)M;
        g.maxM = (int)maxM;
        g.maxM0 = (int)maxM0;
        g.maxlevel = maxlevel;
        g.enterpoint = (int)enterpoint;
        g.levels.assign(n, 0);
        g.links0.assign((size_t)n * (maxM0 + 1), 0);
        g.up_off.assign(n, -1);
        for (uint32_t i = 0; i < n; ++i) {
            uint32_t lvl;
            rd(in, lvl);
            g.levels[i] = (int)lvl;
            if (lvl) {
                g.up_off[i] = (int64_t)g.up_links.size();
                g.up_links.resize(g.up_links.size() + (size_t)lvl * (maxM + 1), 0);
            }
            for (uint32_t l = 0; l <= lvl; ++l) {
                uint32_t qty;
                rd(in, qty);
                int32_t* L = l == 0 ? &g.links0[(size_t)i * (maxM0 + 1)]
                                    : &g.up_links[g.up_off[i] + (size_t)(l - 1) * (maxM + 1)];
                if (qty > (l == 0 ? maxM0 : maxM)) throw EngineError(Err::DataIO, "corrupt adjacency list");
                L[0] = (int32_t)qty;
                in.read(reinterpret_cast<char*>(L + 1), (std::streamsize)qty * 4);
                if (!in) throw EngineError(Err::DataIO, "truncated index file");
            }
        }
        e->bp_.M = (int)M;
        e->bp_.maxM = (int)maxM;
        e->bp_.maxM0 = (int)maxM0;
        e->bp_.skip_optimized = true;
        e->method_ = Method::Hnsw;
        e->graph_rows_.clear();
    }
    e->loaded_graph_ = true;
    e->created_ = true;
    e->dirty_ = true;
    e->graph_dirty_ = false;
    e->ef_ = 200;
    return e;
}

}  // namespace gfxknn
