// Host side of the MI355X k-NN engine: index objects whose rows and graphs live in HBM.
//
// Data model (deliberately not NMSLIB's Object* soup, include/object.h:41-104): rows are one
// row-major array in HBM (stride padded to 32 bytes), external ids a parallel int32 array, the
// HNSW graph two fixed-stride int32 arrays.  The host keeps a copy of the rows only to serve
// nmslib_get_data_point / borrow / save and to construct the graph.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "kernels/kernels.hpp"

namespace gfxknn {

// ---- errors: thrown inside the engine, mapped to nmslib_error_t at the ABI ----------------
enum class Err : int {
    InvalidArgument = 2,
    OutOfMemory = 3,
    SpaceIncompatible = 5,
    QueryTooLarge = 6,
    IndexBuildFailed = 8,
    QueryExecutionFailed = 9,
    DataIO = 10,
    Runtime = 13,
};
struct EngineError : std::runtime_error {
    Err code;
    EngineError(Err c, const std::string& m) : std::runtime_error(m), code(c) {}
};

void hip_check(hipError_t e, const char* what);  // throws EngineError(Runtime / OutOfMemory)
inline size_t align8(size_t b) { return (b + 7) & ~(size_t)7; }

// ---- "name=value" parameters (include/params.h:44-74,181-251) -------------------------------
class ParamSet {
   public:
    ParamSet() = default;
    explicit ParamSet(const std::vector<std::string>& desc);  // throws on bad format / duplicates
    bool has(const std::string& name) const;
    // Typed optional getters; conversion failures throw like ConvertStrToValue (params.h:289-299).
    void get(const std::string& name, long long& v);
    void get(const std::string& name, int& v);
    void get(const std::string& name, size_t& v);
    void get(const std::string& name, double& v);
    void get(const std::string& name, bool& v);
    void get(const std::string& name, std::string& v);
    void check_unused() const;  // AnyParamManager::CheckUnused (params.h:241-251)

   private:
    const std::string* find(const std::string& name);
    std::vector<std::pair<std::string, std::string>> kv_;
    std::vector<bool> seen_;
};

// ---- device buffer ---------------------------------------------------------------------------
class DevBuf {
   public:
    DevBuf() = default;
    ~DevBuf() { release(); }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept { swap(o); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        release();
        swap(o);
        return *this;
    }
    void* ensure(size_t bytes);  // grow-only; a growth does NOT keep the contents
    // grow to `bytes` keeping the first `keep` bytes: new allocation, device-to-device copy on `s`, then the old block is
    // freed (both exist for the copy).  Throws like ensure; after a failed allocation the old block is untouched.
    void* grow_keep(size_t bytes, size_t keep, hipStream_t s);
    void release();
    void swap(DevBuf& o);
    void* ptr() const { return p_; }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p_);
    }
    size_t bytes() const { return n_; }

   private:
    void* p_ = nullptr;
    size_t n_ = 0;
};

// ---- an event that orders work (no timing): made at its first record, destroyed with its owner ----
class Event {
   public:
    Event() = default;
    ~Event() { if (e_) (void)hipEventDestroy(e_); }
    Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }  // move-only
    void record(hipStream_t s);  // (stream_wait: after a record)
    // the host waits for the last record (none yet: returns at once); a failure names `what`
    void wait(const char* what) { if (e_) hip_check(hipEventSynchronize(e_), what); }
    void stream_wait(hipStream_t s) { hip_check(hipStreamWaitEvent(s, e_, 0), "hipStreamWaitEvent"); }

   private:
    hipEvent_t e_ = nullptr;
};

// ---- pinned host block (grow-only; a growth does NOT keep the contents) ----
class PinnedBuf {
   public:
    PinnedBuf() = default;
    ~PinnedBuf() { if (p_) (void)hipHostFree(p_); }
    PinnedBuf(PinnedBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }  // move-only
    void* ensure(size_t bytes, size_t slack = 0);  // a growth allocates bytes + slack
    void* ptr() const { return p_; }

   private:
    void* p_ = nullptr;
    size_t n_ = 0;
};

// ---- staged upload: a pinned block and the event behind the last copy out of it ----
struct StagedUpload : PinnedBuf {
    // waits until the last copy has left the block (a failure names `what`), then the block with room for `bytes` (a growth
    // adds a quarter: slowly growing uploads do not allocate each time)
    void* begin(size_t bytes, const char* what) {
        sent_.wait(what);
        return ensure(bytes, bytes / 4);
    }
    void sent(hipStream_t s) { sent_.record(s); }  // the copy out of the block was enqueued on s
   private:
    Event sent_;
};

// restores the calling thread's current device on every way out of a scope that visits other devices
struct DeviceGuard {
    int dev;
    explicit DeviceGuard(int d) : dev(d) {}
    ~DeviceGuard() { (void)hipSetDevice(dev); }
};

// ---- HNSW graph on the host (flat arrays; same layout goes to HBM) ---------------------------
struct HostGraph {
    int n = 0, M = 16, maxM = 16, maxM0 = 32, efConstruction = 200, delaunay = 2;
    int maxlevel = 0, enterpoint = 0;
    std::vector<int32_t> levels;    // [n]
    std::vector<int32_t> links0;    // [n][maxM0+1] = count, ids...
    std::vector<int64_t> up_off;    // [n] offset (ints) into up_links, -1 if level 0 only
    std::vector<int32_t> up_links;  // per node: level blocks of (maxM+1) ints
    bool empty() const { return n == 0; }
};

struct HnswBuildParams {
    int M = 16, maxM = 16, maxM0 = 32, efConstruction = 200, delaunay = 2, post = 0;
    int threads = 0;  // 0 = hardware concurrency
    double mult = 0;  // 0 = 1/ln(M)
    bool skip_optimized = false;
    int gpu_build = -1;       // engine extension: 1 = batched construction on the GPU, 0 = host, -1 = auto
    int gpu_build_batch = 0;  // max nodes inserted per batch (0 = default)
    int gpu_build_div = 0;    // a batch is at most 1/div of the graph built so far (0 = default)
    int gpu_build_cut = 0;    // GPU builder: no batch spans position N (0 = off); see DESIGN.md 4.6a
    int gpu_append = 0;       // 1 = rows added after a GPU build are inserted into the resident graph
};


void hnsw_check_params(const HnswBuildParams& bp);
std::vector<int32_t> hnsw_random_levels(size_t n, const HnswBuildParams& bp);

// Construct the graph (restates Hnsw::add / kSearchElementsWithAttemptsLevel /
// getNeighborsByHeuristic2 / addFriendlevel, src/method/hnsw.cc:534-708, include/method/hnsw.h:
// 129-169,258-314) with `threads` workers.  space = index-time SpaceCode.  rows: f32 [n][dim]
// or u8 [n][128].
void hnsw_build_host(int space, const void* rows, size_t n, size_t dim, const HnswBuildParams& bp,
                     HostGraph& out);
// ... over strings: leven rows as CSR bytes (row_ptr, bytes), bit_hamming rows as W words each
void hnsw_build_strings(int space, const int64_t* row_ptr, const uint8_t* bytes, const uint32_t* words, size_t W,
                        size_t n, const HnswBuildParams& bp, HostGraph& out);

// ---- dense brute force (brute.cpp): what prepare_brute leaves for knn_brute, next to the engine's rows, ids and aux ----
struct BruteDense {
    // uint8: the re-centred rows (x ^ 0x80) and aux >> 1 of the fast-path scan
    DevBuf rows_i8, auxh;
    // float rows on un-centred data (l2, cosine, angular): selection copy (rows - column mean) and the mean
    DevBuf rows_sel, mean;
    bool centred = false;
    double mu_norm = 0;       // |column mean| (centred cosine scoring)
    double cosc_spread2 = 0;  // E|b - mean|^2 measured at finalize
    float bmax = 0;           // largest norm of the selection rows
    float bres = 0;           // their largest bf16 rounding residual (relative to the norm for the cosine spaces)
    // f32 fast path: bf16 hi / lo tiles of the selection rows and their start values (split-product scan); fp16 tiles of
    // the rows times f16_scale and their start values (one-product scan)
    DevBuf bf_hi, bf_lo, auxp, f16_hi, auxp16;
    bool have_bf16 = false;
    float f16_scale = 1.f, bres16 = 0;   // power-of-two scale of the fp16 tiles, the rows' largest fp16 residual
    float f16_scale_q = 1.f;             // scale of a batch's fp16 queries (the rows' scale, except centred cosine)
    float cosc_lambda = 1.f;             // centred cosine on the fast path: scale of the two constant columns (row_aug_cosc_kernel)
    float bmax_c = 0, bres_c = 0;        // largest norm / bf16 rounding residual of the augmented rows
    // l1 fast path: the 8-bit copy of the rows in the scan's layout, per column lo / hi / rmax ([3][dim]
    // floats) and the common step; have_l1 = false: declined (l1_quant.hpp) or no room in HBM, the index stays adaptive
    DevBuf l1_u8, l1_cols;
    double l1_step = 0;
    bool have_l1 = false;
    // per-batch workspaces (grow-only, not resident data): the blocks of BfFastWs and of BfL1Ws; the augmented queries of centred
    // cosine on the fast path; verified l2 path: query tiles whose proof failed (exact tail)
    DevBuf ws_top8, ws_thr, ws_list, ws_listcnt, ws_f32_q, ws_qaug, ws_flags;
    DevBuf ws_l1_qt, ws_l1_xe, ws_l1_cand, ws_l1_cnt;

    void release();        // drops the fast paths' resident data
    size_t bytes() const;  // every resident buffer (no workspace)
    // the tiles as a launch part; dp: the plan's row length; augmented: they were cut from the augmented rows
    BfF32Tiles tiles(int dp, bool augmented) const;
};

// ---- GPU HNSW builder (hnsw_gpu_build.cpp): construction workspaces, released after the build ----
struct BatchPairs;  // hnsw_batch_plan.hpp
struct HnswBuildWs {
    // per (node, level) pair of a batch: the node, its pair one level up, its start node, its efConstruction candidates
    DevBuf pts, src, starts, cand_ids, cand_d, cand_n, status;
    // per level slice: batch-mates (64 per new node); reverse-link requests (M per new node), sorted, and their distinct targets
    DevBuf extra_ids, extra_d, extra_n, req_key, req_dist, req_key2, req_dist2, sort_tmp, active, nactive;
    size_t sort_tmp_bytes = 0;  // what the request sort asked for (reserve_batches)

    void release() { *this = HnswBuildWs{}; }
    void reserve_batches(int max_batch, int M, size_t n);  // what holds for every batch of a pass over n rows
    void reserve_pairs(size_t npairs, int efC);            // one batch's pairs
};

// ---- dense HNSW search (hnsw_search.cpp): per-batch workspaces (grow-only, not resident data) ----
struct HnswSearchWs {
    // per query of the whole batch: the counts when the caller asks for none, SearchOld's status
    DevBuf outcnt, status;
    // visited bitsets of the HBM-visited plans; the visited-overflow list of the LDS-table plans (count + query ids)
    DevBuf bitset, fix;
    // fp16 walk: its sorted arrays (positions, fp16-row distances) and their lengths
    DevBuf rr_ids, rr_d, rr_cnt;
    // two stages (tombstones, filters): the walk's max(ef, k) results per query of a slice, their counts
    DevBuf live_ids, live_d, live_cnt;
    // SearchOld's per-query queues; the HBM-array kernel's sorted array (old_a keys, old_r positions)
    DevBuf old_a, old_r, old_heap;
};

// ---- the index ---------------------------------------------------------------------------------
enum class Method { Brute, Hnsw };

// nmslib_sparse_elem_float_t (nmslib_c.h): the reference's SparseVectElem<float> layout
struct SparseElem {
    uint32_t id;
    float value;
};

struct Filter;  // filtered search, below the engine

class Engine {
   public:
    // space_params: the space factory's parameters ("p" of lp_sparse); the dense factories ignore theirs
    Engine(const std::string& space, const std::string& method, int data_type, int dist_type,
           const std::vector<std::string>& space_params = {});
    ~Engine();

    const std::string& space_name() const { return space_name_; }
    const std::string& method_name() const { return method_name_; }
    bool is_u8() const { return space_ == SP_L2SQR_SIFT; }
    size_t size() const { return parent_ ? view_n_ : ids_.size(); }
    size_t dim() const { return dim_; }
    size_t elem_bytes() const { return is_u8() ? 1 : 4; }
    size_t row_bytes() const { return dim_ * elem_bytes(); }
    // Object::datalength(): u8 rows carry their norm, the "fast" divergence objects their logarithms
    size_t stored_row_bytes() const { return is_u8() ? dim_ + 4 : diverg_stores_logs() ? dim_ * 8 : dim_ * 4; }

    void add_row(const void* data, size_t elem_count, int32_t id);
    const void* host_row(size_t pos) const;
    void stored_row(size_t pos, void* dst) const;  // payload as the reference stores it
    int32_t ext_id(size_t pos) const { return ids_[pos]; }
    void reset();

    // ---- deleted rows (nmslib_gpu_delete_ids) ----
    // Marks every row that carries one of ids[0 .. count) now; returns how many rows were newly marked.  A tombstone
    // belongs to a position: positions do not move and a row added later under the same id is live.  HNSW: the resident
    // bitset follows at once and the results are filtered; exact scan: the index is prepared again without the rows.
    size_t delete_ids(const int32_t* ids, size_t count);
    size_t deleted_rows() const { return n_dead_; }
    // nmslib_gpu_consolidate (hnsw_consolidate.cpp): the marked rows leave the index and positions move
    // (a live row's new position is its rank among the live rows).  A resident HNSW graph is repaired around the deleted
    // nodes and compacted on the device; anything else compacts its host side and is built / prepared again at its next
    // use.  removed / repaired (optional): rows dropped, (node, level) lists rewritten.  Returns when the device is done.
    void consolidate(size_t* removed, size_t* repaired);

    // ---- filtered search (nmslib_gpu_filter_*; filter.cpp) ----
    // bits: one bit per position, `words` words of host memory.  Finalizes a dirty index, may block.  The filter belongs to
    // this engine and goes with it.
    Filter* filter_create(const uint32_t* bits, size_t words, size_t scan_rows);
    void filter_destroy(Filter* f);
    void filter_info(const Filter* f, size_t* allowed_live_rows, size_t* hbm_bytes) const;
    // a filtered batch is knn_device / knn_host with the filter as their last argument

    // ---- sparse vectors (data type 1; sparse.cpp) ----
    bool is_sparse() const { return sparse_; }
    // one row of strictly increasing ids (validated by the caller)
    void add_sparse_row(const SparseElem* elems, size_t count, int32_t id);
    size_t sparse_row_len(size_t pos) const { return (size_t)(sp_ptr_[pos + 1] - sp_ptr_[pos]); }
    void sparse_row(size_t pos, SparseElem* dst) const;
    // k-NN of nq sparse queries (query i: counts[i] elements at queries[i]); results in the pinned staging block
    void knn_sparse_host(const SparseElem* const* queries, const size_t* counts, size_t nq, size_t k,
                         const int32_t** ids, const float** dists, const int32_t** cnt);
    size_t range_sparse_host(const SparseElem* query, size_t count, double radius, size_t capacity, int32_t* ids,
                             float* dists);

    // ---- divergences over dense float rows (diverg.cpp): the KL family, Itakura-Saito, Jensen-Shannon ----
    // rows enter through add_row; queries, range queries and pairs are routed here by knn_host / range_host /
    // pair_distance
    bool diverg_stores_logs() const;  // the reference's object is values + logarithms (2 * dim floats)
    void diverg_logs(const float* x, size_t count, float* out) const;

    // ---- strings (data type 3; strings.cpp): leven and bit_hamming ----
    bool is_string() const { return str_space_; }
    // the HNSW graph of a string index (built by finalize / a deferred create_index), for inspection
    const HostGraph& string_graph() {
        ensure_graph();
        return graph_;
    }
    // one row per string (strs[i]: lens[i] bytes); the whole batch is checked before any row is stored
    void add_strings(const char* const* strs, const size_t* lens, size_t count, const int32_t* ids);
    size_t string_object_bytes(size_t pos) const;  // Object::datalength()
    std::string string_object(size_t pos) const;   // Object::data(), as the reference builds it
    // k-NN of nq string queries (query i: lens[i] bytes); results in the pinned staging block
    void knn_string_host(const char* const* queries, const size_t* lens, size_t nq, size_t k, const int32_t** ids,
                         const float** dists, const int32_t** cnt);
    size_t range_string_host(const char* query, size_t len, double radius, size_t capacity, int32_t* ids, float* dists);

    void create_index(const std::vector<std::string>& params);  // nmslib_create_index
    void set_query_params(const std::vector<std::string>& params);
    bool index_created() const { return created_; }
    void finalize();  // upload + build if dirty (nmslib_initialize_pool / lazy)

    // k-NN: device-resident batch (the hot entry) and host convenience wrapper.  f (optional): a filter of this index, the
    // batch then runs over the rows it allows (filter.cpp)
    void knn_device(const void* d_queries, size_t nq, size_t elem_count, size_t k, int32_t* d_ids,
                    float* d_dists, int32_t* d_cnt, hipStream_t stream, Filter* f = nullptr);
    // host buffers in, results in this engine's pinned staging block (valid until the next call; the caller holds `mu`)
    void knn_host(const void* queries, size_t nq, size_t elem_count, size_t k, const int32_t** ids, const float** dists,
                  const int32_t** cnt, Filter* f = nullptr);
    // ... with one filter per query (filter.cpp): filter_of_query [nq] (host) names an entry of filters
    // [n_filters] (host), or -1 = unfiltered; both are read before the call returns.  routes [nq] (host, optional): per query
    // the last_path of the single-filter batch its filter's queries would form.  last_path is 9 afterwards.  HNSW: one launch
    // chain per route segment of the batch (filter_batch_plan.hpp); exact scan: one knn_brute per filter that has queries.
    void knn_device_each(Filter* const* filters, size_t n_filters, const int32_t* filter_of_query, const void* d_queries,
                         size_t nq, size_t elem_count, size_t k, int32_t* d_ids, float* d_dists, int32_t* d_cnt,
                         hipStream_t stream, int32_t* routes);
    void knn_host_each(Filter* const* filters, size_t n_filters, const int32_t* filter_of_query, const void* queries, size_t nq,
                       size_t elem_count, size_t k, const int32_t** ids, const float** dists, const int32_t** cnt,
                       int32_t* routes);
    float pair_distance(size_t p1, size_t p2);
    // RangeQuery on the brute-force index (range.cpp): matches in insertion order, the first `capacity`; returns how many were written
    size_t range_host(const void* query, size_t elem_count, double radius, size_t capacity, int32_t* ids, float* dists);
    bool is_brute() const { return method_ == Method::Brute; }
    // ---- batched range queries on the exact scan (nmslib_gpu_range_query_batch*; range.cpp) ----
    // Row q of the outputs ([nq][capacity]; -1 / +inf behind counts[q] = min(totals[q], capacity) entries) is what range_host
    // writes for query q with radii[q]; totals[q] counts every match.  radii is host memory in both entries and is read
    // before the call returns.  capacity == 0: count only (ids / dists unused).  counts and totals may be null.
    // The refusals that need no device (the index kinds that are not served, the query length) come first, in both.
    // The device entry only enqueues (range_batch_plan.hpp: last_path 10 the batched kernels, 11 the single-query
    // launches per query); the host entry is the device entry plus copies, and asks the shards of a sharded index in order.
    void range_batch_device(const void* d_queries, size_t nq, size_t elem_count, const double* radii, size_t capacity,
                            int32_t* d_ids, float* d_dists, int32_t* d_counts, int32_t* d_totals, hipStream_t stream,
                            bool pad = true);  // (pad = false: the host entry pads in host memory)
    void range_batch_host(const void* queries, size_t nq, size_t elem_count, const double* radii, size_t capacity,
                          int32_t* ids, float* dists, int32_t* counts, int32_t* totals);

    void save(const std::string& path, bool save_data);
    static std::unique_ptr<Engine> load(const std::string& path, int data_type, int dist_type, bool load_data);

    size_t thread_pool_size = 0;
    size_t memory_usage() const;

    // counters of the last HNSW batch (device pointers)
    const int32_t* last_ndc() const { return have_counters_ ? ws_ndc_.as<int32_t>() : nullptr; }
    const int32_t* last_hops() const { return have_counters_ ? ws_hops_.as<int32_t>() : nullptr; }
    const int32_t* last_hops_up() const { return have_counters_ ? ws_hops_up_.as<int32_t>() : nullptr; }

    // HIP-event timing of the dominant kernel (nmslib_gpu_kernel_timing)
    void set_profiling(bool on) { prof_ = on; }
    void collect_profile(double* total_ms, uint64_t* launches);

    double upload_seconds = 0, build_seconds = 0;
    // the last finalize: rows it inserted into an existing graph (0: a full build), rows it copied to HBM
    size_t rows_appended = 0, rows_uploaded = 0;
    int last_path = 0;  // see nmslib_gpu_stats_t
    int each_path_ = 0;  // last_path 9: the path of the last part of that batch (what the fast-path statistics describe)
    int stats_path() const { return last_path == 9 ? each_path_ : last_path; }
    size_t rows16_bytes() const;  // the fp16 traversal copy (gpu_rows=f16), shards included
    // flags of the last fast-path slice (device): [fast_nqt_] fallback flags, then (float rows) [fast_nqt_] precise flags
    const int* fast_flags_ = nullptr;
    int fast_nqt_ = 0;
    bool fast_has_precise_ = false;
    void fast_tile_counts(size_t* tiles, size_t* precise, size_t* fallback);
    // HNSW (LDS visited table): queries of the last batch that were re-run by the bitset kernel (waits for the batch);
    // SearchOld: queries of the last batch whose table filled up, on which the batch ran again with bitsets
    size_t hnsw_redone();
    hipStream_t last_stream_ = nullptr;  // stream of the most recent batch (the statistics wait for THAT one)
    // Batches of one index run in the order of the calls, whatever streams they are given: they share the workspaces.
    // Called under `mu` before anything is enqueued on `next`: when the last work went to another stream, `next` waits
    // for an event recorded there.  The same stream again is a pointer compare.
    void order_after_last(hipStream_t next);
    // sw_.fix holds the last batch's count: set by hnsw_search_lds with an LDS-table plan; cleared by every other search path,
    // reset, the consolidate and the builder (false / 0).  kRedoneOnHost: SearchOld's last batch held queries whose table
    // filled up (status 1) and ran again with bitsets; their number is hnsw_old_redone_
    static constexpr int kRedoneOnHost = 2;
    int hnsw_fix_valid_ = 0;
    size_t hnsw_old_redone_ = 0;
    size_t hbm_bytes() const;

    std::mutex mu;  // serialises finalize + queries on one index

    // ---- row shards behind one handle (index parameter gpu_shards) ----
    size_t shard_count() const { return shards_.size(); }
    // nmslib_gpu_graph_builder: 0 no graph or a loaded one, 1 host, 2 GPU (shards: all children take the same route)
    int graph_builder() const { return shards_.empty() ? graph_builder_ : shards_[0]->graph_builder_; }

   private:
    // host rows / ids of this engine: its own, or (shard child) a window of the parent's
    const float* rows_f32() const { return parent_ ? parent_->rows_f32_.data() + view_lo_ * dim_ : rows_f32_.data(); }
    const uint8_t* rows_u8() const { return parent_ ? parent_->rows_u8_.data() + view_lo_ * 128 : rows_u8_.data(); }
    int resolve_shards() const;
    void finalize_sharded(int nshards);
    void knn_sharded(const void* d_queries, size_t nq, size_t elem_count, size_t k, int32_t* d_ids, float* d_dists,
                     int32_t* d_cnt, hipStream_t stream);
    std::vector<std::unique_ptr<Engine>> shards_;
    std::vector<Event> shard_events_;
    Event shard_ready_;
    Event order_event_;                 // order_after_last: made at the first change of stream
    bool have_last_ = false;            // last_stream_ names a stream that work of this index went to (nullptr: the null stream)
    const Engine* parent_ = nullptr;  // shard child: rows [view_lo_, view_lo_ + view_n_) of the parent, no copy
    size_t view_lo_ = 0, view_n_ = 0;
    int forced_device_ = -1;
    int gpu_shards_ = -1;  // index parameter: -1 unset, 0 = all visible devices, N = that many
    DevBuf ws_sh_ids_, ws_sh_d_, ws_bigk_, ws_bigk_tmp_;
    // Pinned host staging buffer (grow-only): PCIe copies from/to pageable memory are staged by the runtime in small
    // chunks and block the calling thread; one pinned block makes the batch's H2D and D2H a single DMA each.
    void* pinned(size_t bytes) { return pinned_.ensure(bytes); }
    PinnedBuf pinned_;
    void check_device();
    static void check_diverg_query_length(size_t elem_count, size_t dim);
    // ---- plumbing shared by the host entries of every data type (engine.cpp) ----
    struct ResultBlock {  // device pointers into ws_ids_
        int32_t* ids;
        float* dists;
        int32_t* cnt;
    };
    ResultBlock result_block(size_t nq, size_t k);
    void fetch_results(size_t nq, size_t k, const char* what, const int32_t** ids, const float** dists,
                       const int32_t** cnt);
    using ScanLaunch = std::function<void(const ScanPlan& p, size_t q0, float* split_d, int32_t* split_pos)>;
    void scan_slices(size_t nq, size_t k, int tq, const ResultBlock& out, const ScanLaunch& launch);
    // ---- dense range search (range.cpp) ----
    using RangeLaunch = std::function<void(float* filter, float* report)>;
    size_t range_select(bool two_dists, float r, size_t capacity, int32_t* ids, float* dists, const RangeLaunch& launch);
    // RangeQuery<dist_t>(space, obj, static_cast<dist_t>(radius)), nmslib_c.cpp:1092-1093
    float range_radius(double radius) const { return is_u8() ? (float)(int)radius : (float)radius; }
    void check_range_batch(size_t elem_count, bool device_entry) const;  // the refusals that need no device
    const float* stage_radii(const double* radii, size_t nq, int turn, hipStream_t stream);  // -> the staging block's copy
    // range_batch_host's two ways; both leave got[q] = the entries of row q and write no padding
    void range_batch_merge_shards(const void* queries, size_t nq, size_t elem_count, const double* radii, size_t capacity,
                                  int32_t* ids, float* dists, int32_t* counts, int32_t* totals, std::vector<size_t>& got);
    void range_batch_fetch(const void* queries, size_t nq, size_t elem_count, const double* radii, size_t capacity,
                           int32_t* ids, float* dists, int32_t* counts, int32_t* totals, std::vector<size_t>& got);
    // workspaces (grow-only): range_select's block counts; a batch's radii as floats, in two staged uploads and two device
    // buffers that calls take in turn; the match bits and block counts of a slice; the host entry's result block
    struct RangeWs {
        DevBuf cnt, radii[2], masks, counts, res;
        StagedUpload staged[2];
        int turn = 0;
    } rw_;
    float read_float(const float* d_out, const char* what);
    void upload_sparse();
    float pair_distance_sparse(size_t p1, size_t p2);
    void upload_diverg();
    DivergRows diverg_rows() const;
    void knn_diverg_host(const float* queries, size_t nq, size_t elem_count, size_t k, const int32_t** ids,
                         const float** dists, const int32_t** cnt);
    size_t range_diverg_host(const float* query, size_t elem_count, double radius, size_t capacity, int32_t* ids,
                             float* dists);
    float pair_distance_diverg(size_t p1, size_t p2);
    void upload_strings();
    void build_string_graph();
    void knn_string_hnsw(const int64_t* d_qoff, const int32_t* d_qlen, const uint64_t* d_peq, const uint32_t* d_qw,
                         int nw_max, size_t nq, size_t k, int32_t* d_ids, float* d_dists, int32_t* d_cnt);
    float pair_distance_string(size_t p1, size_t p2);
    static bool parse_bits(const char* s, size_t len, std::vector<uint32_t>& words, size_t& bits);
    void string_query(const char* s, size_t len, Err parse_err, std::vector<uint32_t>& words) const;
    size_t ham_words() const { return st_bits_ > 0 ? (size_t)(st_bits_ + 31) / 32 : 0; }
    void ensure_graph();
    void finalize_index();                        // finalize() without the tombstones' upload
    bool is_dead(size_t pos) const { return (pos >> 5) < tomb_.size() && ((tomb_[pos >> 5] >> (pos & 31)) & 1u); }
    // filtered search (filter.cpp)
    void check_filter_served() const;             // SpaceIncompatible for what filters do not serve (needs no device)
    void check_filter(const Filter* f) const;     // InvalidArgument: another index's filter, a stale one
    void filter_compact(Filter& f, const uint32_t* tomb, const int32_t* row_pos, size_t n_rows, DevBuf& list, size_t list_max,
                        size_t& count);
    void filter_gather(Filter& f);                // exact scan: f.sub = the index of the allowed live rows
    // a filtered batch, from knn_device: what has to happen before anything is enqueued (refusals; the exact scan's gather
    // when the index was prepared again: may block), and one slice of the batch (exact scan; HNSW)
    void filter_begin_batch(Filter& f);
    void knn_filtered_slice(Filter& f, const void* d_queries, size_t nq, size_t k, int32_t* d_ids, float* d_dists, int32_t* d_cnt,
                            hipStream_t stream);
    void filter_forget_flags(const Filter& f);    // the statistics' pointer into f's child, before its workspaces go
    void knn_hnsw_filtered(Filter& f, const void* d_queries, size_t nq, size_t k, const HnswOut& out, hipStream_t stream);
    // one filter per query: every check that needs no device (served index kinds, the entries' range, each filter)
    void check_filters_each(Filter* const* filters, size_t n_filters, const int32_t* filter_of_query, size_t nq) const;
    // dst row i = src row list[i] (rows of a multiple of 4 bytes): the 16-byte gather where its rule holds, else word by word
    void gather_rows(const void* src, const int32_t* list, size_t m, size_t row_bytes, void* dst, hipStream_t stream);
    // what a batch with one filter per query uploads and works in (grow-only): the filter table, slots and permutations (one
    // block, staged in `staged`), the batch in plan order and its results
    struct FilterEachWs {
        DevBuf tab, q, res;
        StagedUpload staged;
    } each_;
    std::vector<std::unique_ptr<Filter>> filters_;
    uint64_t pos_epoch_ = 0;     // counts what moves positions: a consolidate that removed a row, a reset
    uint64_t prepared_ = 0;      // counts upload_rows: an exact-scan filter gathered at another count gathers again
    DevBuf d_livepos_;           // exact scan with deleted rows: the position of every resident row (upload_rows)
    void upload_tombstones();                     // the bitset of all size() rows -> d_tomb_, ordered behind the index's work
    // consolidate: host rows and ids at newpos (-1: dropped), marks cleared; the all-rows-marked case; the resident graph
    void compact_host_rows(const std::vector<int32_t>& newpos, size_t live);
    void drop_all_rows();
    void consolidate_resident(const std::vector<int32_t>& newpos, size_t live, size_t& repaired);
    void upload_rows(size_t first = 0);           // rows [first, n); first > 0 keeps what is resident
    void build_graph();
    bool use_gpu_build() const;
    void build_graph_gpu();
    void build_graph_gpu_pass(const std::vector<int32_t>& levels, bool reverse);
    void build_graph_gpu_insert(size_t first, bool reverse);  // positions [first, n) into the graph of dg_ / graph_
    void search_batch(const HnswDeviceGraph& bgraph, const BatchPairs& pairs);
    void link_batch(const HnswDeviceGraph& bgraph, const BatchPairs& pairs, size_t linked);
    void download_graph_links();
    bool can_append() const;
    bool append_rows_gpu();   // gpu_append=1; false: a buffer could not grow, take the full path
    void sync_host_graph();   // the lists of graph_ follow the device's after an append or a consolidate (read by save)
    // cosine on the optimized index after a consolidate: the normalised rows as the device holds them, [n][dim]; false: the
    // file writer normalises the host rows itself, as it always did
    bool fetch_resident_rows(std::vector<float>& rows);
    void pack_rows16(size_t first, size_t n, int e);  // rows [first, n) of the fp16 copy at scale 2^e
    void prepare_graph_rows(size_t first = 0);
    void upload_graph();
    void bind_graph_buffers();                  // dg_.links0 / up_off / up_links = the three buffers
    float rows_max_abs(size_t first, size_t n);  // largest |element| of the resident rows [first, n)
    // dense brute force (brute.cpp)
    void prepare_brute();
    void measure_rows_f16(const float* rows, size_t n, int ld, int dim, bool relative, float* bm);
    void make_fast_tiles(const BfSplitSrc& src, int dp, const float* aux, float aux_pad, float aux16_mul);
    void make_l1_copy();   // the l1 fast path's resident side; leaves have_l1 = false when declined or out of memory
    void knn_brute(const void* d_queries, size_t nq, size_t k, int32_t* d_ids, float* d_dists,
                   int32_t* d_cnt, hipStream_t stream);
    // dense HNSW search (hnsw_search.cpp).  out: the results and work counters of the slice (knn_device: out.at(q0, k))
    void knn_hnsw(const void* d_queries, size_t nq, size_t k, const HnswOut& out, hipStream_t stream);
    // the search of one slice on whichever path it takes; positions: on dg_ without ext_ids, so that positions come out
    void hnsw_walk(bool positions, const void* d_queries, size_t nq, size_t k, const HnswOut& out, hipStream_t stream);
    // the walk for max(ef, k) positions into a workspace, then the first k of them that are live (an index with tombstones) and
    // allowed (allow: a filter's bits over n_allow positions, or nullptr)
    // each (optional, in place of allow): every query's own filter (slot[0] is the first query's)
    void knn_hnsw_two_stage(const void* d_queries, size_t nq, size_t k, const uint32_t* allow, size_t n_allow,
                            const HnswOut& out, hipStream_t stream, const FilterEach* each = nullptr);
    // gpu_inwalk=1: the same two tests inside the walk, in place of the two stages, where the kernel serves
    // the batch (hnsw_inwalk_plan.hpp); last_path 8
    bool inwalk_serves(size_t k) const;
    void knn_hnsw_inwalk(const void* d_queries, size_t nq, size_t k, const uint32_t* allow, size_t n_allow, const HnswOut& out,
                         hipStream_t stream, const FilterEach* each = nullptr);
    void knn_hnsw_old(const HnswDeviceGraph& g, const void* d_queries, size_t nq, size_t k, const HnswOut& out,
                      hipStream_t stream);
    // Hnsw::Search, hnsw.cc:724: algoType=old, or hybrid with ef >= 1000, runs SearchOld
    bool search_old() const { return algo_ == "old" || (algo_ == "hybrid" && ef_ >= 1000); }
    // SearchV1Merge on the LDS kernels: the launch, and behind it the bitset launch for queries whose visited table
    // filled up; timed: the first launch is the timed interval (else the caller closes it with prof_end)
    void hnsw_search_lds(const HnswDeviceGraph& g, bool rows_f16, const void* d_queries, size_t nq, size_t k, int ef,
                         const HnswOut& out, bool timed, hipStream_t stream);
    // gpu_rows=f16: the walk over the fp16 copy, then the f32 re-rank of its sorted array
    void knn_hnsw_f16(const HnswDeviceGraph& g, const void* d_queries, size_t nq, size_t k, const HnswOut& fin,
                      hipStream_t stream);
    bool ensure_rows16();  // makes the copy if there is none; false: no copy (allocation failed, no rows): stay on f32
    static bool parse_gpu_rows(const std::string& v);  // "f32" -> false, "f16" -> true, else InvalidArgument
    void check_rows16_served() const;                  // InvalidArgument for indexes without float rows
    uint32_t* cleared_bitset(size_t m, size_t words, hipStream_t stream);

    std::string space_name_, method_name_;
    int space_ = SP_L2;
    Method method_ = Method::Brute;
    size_t dim_ = 0;
    std::vector<int32_t> ids_;
    std::vector<float> rows_f32_;
    std::vector<uint8_t> rows_u8_;
    // deleted rows: bit = position (rows beyond the last word are live), how many bits are set; HNSW: the copy the filter
    // kernel reads and the block it is staged in
    std::vector<uint32_t> tomb_;
    size_t n_dead_ = 0;
    DevBuf d_tomb_;
    StagedUpload tomb_staged_;
    bool diverg_ = false;  // a divergence space: rows_f32_ on the host, values + logarithms in d_rows_
    // sparse rows: host CSR (get_data_point / borrow) and its copy in HBM after finalize
    bool sparse_ = false;
    std::vector<int64_t> sp_ptr_{0};
    std::vector<uint32_t> sp_ids_;
    std::vector<float> sp_vals_;
    DevBuf d_sp_ptr_, d_sp_ids_, d_sp_vals_;
    // string rows: leven CSR bytes, or bit_hamming words (W = ham_words() per row, st_bits_ bits; -1: no row yet);
    // the HBM copy after finalize
    bool str_space_ = false;
    std::vector<int64_t> st_ptr_{0};
    std::vector<uint8_t> st_bytes_;
    std::vector<uint32_t> st_words_;
    int64_t st_bits_ = -1;
    DevBuf d_st_ptr_, d_st_data_;
    DevBuf ws_st_mw_;  // multi-block leven state

    // index-time state
    bool created_ = false;       // nmslib_create_index was called
    bool dirty_ = true;          // rows added since the last finalize (device copy stale)
    bool graph_dirty_ = true;    // rows added since the graph was last built
    bool loaded_graph_ = false;  // graph came from a file: never rebuild it
    int graph_builder_ = 0;      // who built graph_: 0 nobody (no graph yet, or loaded), 1 the host builder, 2 the GPU builder
    size_t graph_up_ints_ = 0;   // ints of the upper-level lists of the graph on the device (GPU builder, consolidate)
    size_t built_n_ = 0;         // rows the GPU builder's resident graph covers (0: none, or it was not completed); after a
                                 // consolidate: the rows of the compacted graph, whoever built it
    bool save_resident_rows_ = false;  // a consolidate compacted the resident graph: the index file gets the device's normalised rows
    bool host_links_stale_ = false;  // an append or a consolidate changed the lists on the device; graph_.links0 / up_links are behind
    HnswBuildParams bp_;
    HostGraph graph_;
    std::vector<float> graph_rows_;  // rows as stored inside a loaded index (cosine: normalised)
    int ef_ = 200;                   // the shim's default (nmslib_c.cpp:330)
    std::string algo_ = "hybrid";
    // engine extensions, index-time gpu_rows and query-time gpu_rows / gpu_rerank / gpu_inwalk: they stay as set until set again
    bool rows_f16_index_ = false;    // make the fp16 copy at finalize
    bool rows_f16_ = false;          // walk the fp16 copy (made at the next batch if there is none)
    int rerank_ = 0;                 // entries of the walk's sorted array that are re-ranked in f32; 0 = all
    bool inwalk_ = false;            // deleted rows and filters are tested inside the walk (hnsw_inwalk_kernels.hip)
    bool rows16_failed_ = false;     // the copy did not fit into HBM: f32 until the rows change
    int rows16_exp_ = 0;             // the copy's scale is 2^rows16_exp_, chosen for rows16_max_ = the largest |element|
    float rows16_max_ = 0;

    // device state
    int device_ = -1;
    hipStream_t stream_ = nullptr;
    DevBuf d_rows_, d_aux_, d_ids_, d_links0_, d_up_off_, d_up_links_, d_rownorm_;
    DevBuf d_rows16_;  // fp16(scale * rows) [n][dg_.ld16], see dg_.rows16
    BruteDense brute_;
    size_t d_n_ = 0;
    int ldb_ = 0;
    HnswDeviceGraph dg_{};

    // workspaces
    DevBuf ws_q_, ws_qpad_, ws_qsel_, ws_qaux_, ws_cand_, ws_cnt_, ws_ids_, ws_dists_;
    DevBuf ws_ndc_, ws_hops_, ws_hops_up_, ws_pair_, ws_rdist_;  // (the counters: dense and string HNSW, the builder)
    HnswSearchWs sw_;
    HnswBuildWs bw_;
    DevBuf ws_bq_, ws_split_;  // sparse / string batches: the packed queries; per-split lists (string HNSW: per-query state)
    // the last batch left work counters: set by the dense HNSW search (hnsw_search.cpp, filter.cpp's subset route) and the string
    // HNSW; cleared by the exact scans, knn_sharded, reset and the consolidate
    bool have_counters_ = false;
    bool prof_ = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events_;
    std::pair<hipEvent_t, hipEvent_t> prof_pair();  // a new pair of prof_events_ (nulls: not profiling)
    void prof_begin(hipStream_t s);
    void prof_end(hipStream_t s);
};

// ---- filtered search (filter.cpp): a subset of an index's positions, prepared on the device ----
struct Filter {
    Engine* owner = nullptr;
    uint64_t epoch = 0;     // the owner's position epoch when the filter was made: a consolidate, a reset make it stale
    size_t n = 0;           // rows of the index when it was made: positions at or beyond n are not allowed
    size_t scan_rows = 0;   // HNSW: the caller's bound of the subset route (0 = none)
    std::vector<uint32_t> bits;  // the allow bitset, ceil(n / 32) words, bits at or beyond n clear
    DevBuf d_allow;         // ... in HBM
    // HNSW: m = allowed live rows when the filter was made, their ascending positions when m <= HNSW_SUBSET_MAX
    size_t m = 0;
    DevBuf d_list;
    // exact scan: the index of the allowed live rows alone, and the owner's prepare count it was gathered at
    std::unique_ptr<Engine> sub;
    uint64_t gathered_at = 0;
};

}  // namespace gfxknn
