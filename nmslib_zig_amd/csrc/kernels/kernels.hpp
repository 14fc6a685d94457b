// Host-callable launchers of the gfx950 kernels.  Plain pointers + hipStream_t; every
// function only enqueues work on `stream` and returns the launch status.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <utility>

namespace gfxknn {

// Space codes (host and device).  Names: include/factory/init_spaces.h:77-86,120.
enum SpaceCode : int {
    SP_L2 = 0,
    SP_L1 = 1,
    SP_LINF = 2,
    SP_COSINE = 3,
    SP_ANGULAR = 4,
    SP_NEGDOT = 5,
    SP_L2SQR_SIFT = 6,
    // search-time variants of the optimized HNSW index (hnsw.cc:70-102): squared L2 and
    // cosine over pre-normalised rows
    SP_L2SQR = 7,
    SP_NORMCOS = 8,
    // sparse only: -QueryNormScalarProduct over the union arrays (querynorm_negdotprod_sparse)
    SP_QNORM_NEGDOT = 9,
    // strings (data type 3)
    SP_LEVEN = 10,
    SP_BIT_HAMMING = 11,
    // divergences over dense float rows (include/factory/init_spaces.h:57-71); SP_JSDIV / SP_JSMETR are the "fast"
    // spaces, whose objects carry their logarithms
    SP_KLDIV = 12,
    SP_KLDIV_RQ = 13,
    SP_KLDIVGEN = 14,
    SP_KLDIVGEN_RQ = 15,
    SP_KLDIVGEN_SLOW = 16,
    SP_ITAKURASAITO = 17,
    SP_JSDIV = 18,
    SP_JSDIV_SLOW = 19,
    SP_JSMETR = 20,
    SP_JSMETR_SLOW = 21,
};

// ---- geometry shared by host and device ------------------------------------------------
constexpr int BF_TQ = 128;     // queries per workgroup (4 waves x 32)
constexpr int BF_BN = 64;      // base rows staged per step
constexpr int BF_KC = 128;     // K-chunk (floats) staged per step
constexpr int BF_MAX_K = 512;  // largest k the selection kernels support

struct BfPlan {
    int nq, qpad, nqt;         // queries, padded to BF_TQ, number of query tiles
    int n;                     // base rows
    int ldb;                   // row stride (floats for f32, bytes for u8)
    int nsplit, rows_per_split;
    int kprime, cap;           // per-(query,split) survivors / candidate buffer capacity
    int p2max;                 // power of two >= nsplit*kprime (rerank sort size)
    int xj, xm;                // counted-bound exchange between splits (bf_kernels.hip); xj = 0: off
    size_t lds_select, lds_rerank;
};
// Fills every field of the plan from (n, dim, nq, k).  is_u8 selects the integer path.
BfPlan bf_make_plan(int n, int dim, int nq, int k, bool is_u8, int qpad_multiple = BF_TQ);
inline size_t bf_cand_elems(const BfPlan& p) { return (size_t)p.qpad * p.nsplit * p.cap; }
// per-(query,split) survivor counts, then the per-query shared thresholds (gthr), then the
// per-(query,split) counted bounds (gq)
// (a second gthr/gq region behind the first: the exact-tail selection of the verified l2 path gets its own, so that one
//  clear at the start of a batch serves both selections -- see bf_f32_prep_kernel)
inline size_t bf_cnt_elems(const BfPlan& p) { return 3 * (size_t)p.qpad * p.nsplit + 2 * (size_t)p.qpad; }

// Row padding for the f32 device copy: multiple of 8 floats (two 16-byte half-wave loads).
inline int f32_row_stride(int dim) { return (dim + 7) & ~7; }

// ---- preparation -------------------------------------------------------------------------
// rowaux per space: L2 -> -0.5*||b||^2 ; COSINE/ANGULAR -> 1/||b|| (0 when ||b||^2 < 2*FLT_MIN);
// NEGDOT -> unused (0).
hipError_t launch_row_aux_f32(const float* base, int n, int ldb, int dim, int space, float* aux,
                              hipStream_t s);
// u8 brute force: rows_i8 [n_pad][128] = re-centred copy (x ^ 0x80), aux [n_pad] = 256*sum(a) - sum(a^2);
// n_pad = bf_u8_rows_padded(n), pad rows are zero with an aux that can never be selected (see bf_select_u8)
inline int bf_u8_rows_padded(int n) { return (n + BF_BN - 1) / BF_BN * BF_BN + BF_BN; }
hipError_t launch_prepare_u8(const uint8_t* base, int n, uint8_t* rows_i8, int32_t* aux, int32_t* auxh, hipStream_t s);
// Copy [rows][dim] -> [rows_pad][ld] with zero fill (elem = 4 or 1 bytes).
hipError_t launch_pad_rows(const void* src, int rows, int dim, void* dst, int rows_pad, int ld,
                           int elem_bytes, hipStream_t s);
// In-place L2 normalisation of rows (hnsw.cc:441-446, hnsw.h:486-497).
hipError_t launch_normalize_rows(float* rows, int n, int ld, int dim, hipStream_t s);

// Column sums in f64: stats[0..ldb) = per-column sums, stats[ldb] = sum of squares of all elements.
hipError_t launch_col_stats(const float* base, int n, int ldb, int dim, double* stats, hipStream_t s);
// dst = src - mean (columns < dim of the first rows_valid rows); used for the centred L2 selection copy and its queries.
hipError_t launch_center_rows(const float* src, const float* mean, int rows, int rows_valid, int ld, int dim, float* dst,
                              hipStream_t s);

// ---- brute force: selection (MFMA) + exact re-rank ---------------------------------------
hipError_t launch_row_aux_cosc(const float* orig, const float* centred, int n, int ldb, int dim, double mu_norm, float* aux,
                               hipStream_t s);
hipError_t launch_query_aux_cosc(const float* orig, const float* centred, int nq, int ldb, int dim, double mu_norm,
                                 float* qaux, hipStream_t s);

// ---- the named parts of a dense brute-force launch (host side) ----
// Where a launch writes: k results per query (ids[i] = ext_ids[position], or the position without ext_ids) and the
// number of valid results per query (cnt, optional).
struct BfOut {
    const int32_t* ext_ids;
    int32_t* ids;
    float* dists;
    int32_t* cnt;
};
// Run only the query groups that an earlier stage flagged: one flag per `tiles` query tiles of BF_TQ queries.
// flags = null: everything runs.
struct BfGate {
    const int* flags = nullptr;
    int tiles = 1;
};
// Survivors of a selection: cand [bf_cand_elems(p)] keys, cnt [bf_cnt_elems(p)] ints (the counts, then the shared
// thresholds and counted bounds of the selection kernels)
struct BfCand {
    unsigned long long* cand;
    int* cnt;
};
// The l2 proof of a re-rank (bf_rerank_kernel): tiles of BF_TQ queries whose proof fails are flagged in flags [p.nqt].
// flags = null: no verification.
struct BfVerify {
    int* flags = nullptr;
    const float* queries_sel = nullptr;
    float bmax = 0.f;
};
// The float rows as finalize leaves them: the originals (re-rank), the selection rows (the centred copy, or the
// originals again), the selection rows' aux (launch_row_aux_f32, or the three planes of launch_row_aux_cosc) and largest
// norm.  The adaptive launchers take n and ldb from their BfPlan, which is made for these rows.
struct BfF32Rows {
    const float *orig, *sel, *aux;
    int n, dim, ldb;
    float bmax;
};
// The float queries of a batch.  The adaptive path reads padded, sel and qaux_cosc; the fast path all of it.
struct BfF32Queries {
    const float* raw;        // [nq][dim] as the caller gave them: the fast path pads them into `padded` (null: already done)
    float* padded;           // [qpad][ldb]: the re-rank's queries
    const float* sel;        // what the selection sees: padded, its centred copy, or (fast path, centred cosine / angular)
                             // the augmented queries [qpad][sel_ld] (launch_query_aug_cosc)
    const float* centred;    // centred cosine / angular on the fast path: the centred copy, for the adaptive fallback
    const float* qaux_cosc;  // centred cosine / angular: per-query constants (launch_query_aux_cosc), else null
    int sel_ld;              // row stride of the augmented queries
    float scale_q;           // fast path: scale of the batch's fp16 queries (l2: the rows' scale -- the start values carry the
                             // product; centred cosine: rows are divided by their norm, queries are not)
};
// The uint8 rows as finalize leaves them (launch_prepare_u8)
struct BfU8Rows {
    const uint8_t *orig, *i8;
    const int32_t *aux, *auxh;
    int n;
};
// HIP events recorded around the scan of a fast path (null: none)
using BfScanEvents = std::pair<hipEvent_t, hipEvent_t>;

// Selections.  `cleared`: the caller's preparation kernel zeroed the shared thresholds at the start of the batch.
hipError_t launch_bf_select_u8(const BfPlan& p, const uint8_t* base_i8, const int32_t* aux, const uint8_t* queries_padded,
                               const BfCand& c, const BfGate& gate, hipStream_t s, bool cleared = false);
// Direct (VALU) selection for spaces with no inner-product form (l1, linf); SP_L2 = squared differences summed on the
// ORIGINAL rows (the exact tail of the verified l2 path; cleared_second_region: it uses the second threshold region)
hipError_t launch_bf_select_direct_f32(const BfPlan& p, int space, const float* base, const float* queries_padded,
                                       const BfCand& c, const BfGate& gate, hipStream_t s,
                                       bool cleared_second_region = false);
// Exact distances of the survivors in the reference's formula, (dist, position) order, top k.
hipError_t launch_bf_rerank(const BfPlan& p, int space, int dim, int k, const void* base, const void* queries_padded,
                            const BfCand& c, const BfGate& gate, const BfVerify& verify, const BfOut& out, hipStream_t s);
// The adaptive f32 path end to end (MFMA selection, re-rank; l2: verification + exact tail).  flags: [p.nqt] ints.
hipError_t launch_bf_adaptive_f32(const BfPlan& p, int space, int k, const BfF32Rows& rows, const BfF32Queries& q,
                                  const BfCand& c, int* flags, const BfGate& gate, const BfOut& out, hipStream_t s,
                                  bool cleared = false);

// uint8 fast path for large batches (bf_kernels.hip: sample pass -> fixed-threshold scan -> list re-rank with
// verification -> adaptive fallback for flagged tile groups).  Exact like the adaptive path.
struct BfU8Fast {
    bool use;
    int qg;                    // query groups of 32 per wave: a workgroup serves 128 * qg queries
    int qpad, nqt;             // queries padded to 128 * qg; scan query tiles
    int stride, r;             // sample = every stride-th tile; threshold = r-th best score of the sample
    int nsplit, tps, caph;     // scan: row splits, 64-row tiles per split, list capacity per (query, split, half)
    int p2max;
    size_t lds_scan, lds_thr, lds_rerank;
    int s_nsplit, s_tps;       // sample pass: splits and sample tiles per split
    BfPlan fallback;           // plan of the adaptive kernel for the fallback
};
BfU8Fast bf_u8_fast_plan(int n, int nq, int k);

// f32 fast path for large batches (bf_kernels.hip: bf16 / fp16 MFMA selection with sample-fixed thresholds, exact f32
// re-rank with verification, adaptive fallback).  Exact like the adaptive path.
struct BfF32Fast {
    bool use;
    int mode;                  // 0 l2, 1 negdotprod (and centred cosine / angular, see cosc), 2 cosine / angular (uncentred)
    int qg;                    // a scan workgroup serves 256 * qg queries (= one query tile)
    bool cosc;                 // centred cosine / angular: mode 1 over augmented rows of sel_dim = dim + 3 columns
    int sel_dim;               // columns of the selection rows / queries (dim, or dim + 3)
    int kch;                   // rows longer than 128: chunks of 128 dimensions per row (1 = the classic shape)
    int dp;                    // 128 * kch: row length of the bf16 tiles
    int tq;                    // queries per scan workgroup / query tile: 256 * qg, or 128 when kch > 1
    int qpad, nqt;             // queries padded to tq; scan query tiles
    int stride, r;
    int rcap;                  // one-product scan: its threshold may sit as low as the rcap-th best sample score
    bool force_precise;        // NMSLIB_GPU_F32_TERMS=3: every tile through the split-product scan
    int nsplit, tps, caph, p2max;
    int s_nsplit, s_tps;
    size_t lds_scan, lds_scan1, lds_thr, lds_rerank;
    BfPlan fallback;
};
BfF32Fast bf_f32_fast_plan(int n, int dim, int nq, int k, int space, bool cosine_centred);

// Per-batch workspace of a fast path: one block per member, each of at least its bf_fast_ws_bytes().  What lies inside
// a block is known here and nowhere else.
struct BfFastWsBytes {
    size_t top8, thr, list, list_cnt, cand, cnt, flags_fb, queries;
};
inline BfFastWsBytes bf_fast_ws_bytes(const BfU8Fast& f) {
    const size_t lists = (size_t)f.qpad * f.nsplit * 2;
    return {(size_t)f.qpad * f.s_nsplit * 2 * 8 * 4, (size_t)f.qpad * 4 + (size_t)f.nqt * 4 + 64, lists * f.caph * 4, lists * 4,
            bf_cand_elems(f.fallback) * 8, bf_cnt_elems(f.fallback) * 4, 0, 0};
}
inline BfFastWsBytes bf_fast_ws_bytes(const BfF32Fast& f) {
    const size_t lists = (size_t)f.qpad * f.nsplit * 2;
    // (list: two planes -- the entries, and behind them the second words of the one-product scan's entries)
    return {(size_t)f.qpad * f.s_nsplit * 2 * 8 * 4, (size_t)f.qpad * 8 + (size_t)f.nqt * 8 + 64, 2 * lists * f.caph * 4, lists * 4,
            bf_cand_elems(f.fallback) * 8, bf_cnt_elems(f.fallback) * 4, (size_t)f.fallback.nqt * 4 + 64,
            (size_t)f.qpad * f.dp * 2 * 3};
}
struct BfFastWs {
    void* top8;        // sample pass: the per-lane top-8 scores (u8: int, f32: float)
    void* thr;         // u8: [qpad] int thresholds, [nqt] fallback flags; f32: [qpad] split-product thresholds, [qpad]
                       // one-product thresholds, [nqt] fallback flags, [nqt] precise flags
    uint32_t* list;    // scan: the rows that reached the threshold, per (query, split, half): hit entries [qpad][caph][lists];
                       // f32: a second plane of the same shape behind it (one-product scan: the entries' largest scores)
    int* list_cnt;
    BfCand fb;         // the adaptive fallback's survivors (f.fallback)
    int* flags_fb;     // f32: the fallback's own proof flags [f.fallback.nqt]
    void* queries;     // f32: the converted queries, [qpad][dp] bf16 hi, bf16 lo, fp16

    size_t list_m_off(const BfF32Fast& f) const { return (size_t)f.qpad * f.caph * f.nsplit * 2; }   // in words
    int* tile_fail(const BfU8Fast& f) const { return static_cast<int*>(thr) + f.qpad; }
    float* thr1(const BfF32Fast& f) const { return static_cast<float*>(thr) + f.qpad; }
    int* tile_fail(const BfF32Fast& f) const { return reinterpret_cast<int*>(thr1(f) + f.qpad); }
    int* precise(const BfF32Fast& f) const { return tile_fail(f) + f.nqt; }
    enum QueryTile { Q_HI = 0, Q_LO = 1, Q_H16 = 2 };
    void* q_tile(const BfF32Fast& f, QueryTile t) const { return static_cast<char*>(queries) + (size_t)t * f.qpad * f.dp * 2; }
};

hipError_t launch_bf_u8_fast(const BfU8Fast& f, int nq, int k, const BfU8Rows& rows, const uint8_t* queries_raw,
                             uint8_t* queries_padded, const BfFastWs& ws, const BfOut& out, const BfScanEvents& ev,
                             hipStream_t s);

inline int bf_f32_rows_padded(int n) { return (n + BF_BN - 1) / BF_BN * BF_BN + BF_BN; }
// out (16 bytes): [0] largest norm, [1] largest bf16 residual, [2] largest |element|, [3] largest fp16 residual of scale16 * row
hipError_t launch_row_maxnorm(const float* rows, int n, int ld, int dim, bool relative_residual, float* out, hipStream_t s,
                              float scale16 = 0.f);
// The resident side of the f32 fast path, cut from the selection rows at finalize (launch_split_bf16): bf16 hi / lo tiles
// [n_pad][128] and start values auxp [n_pad] of the split-product scan (hi / lo: null when dp > 128); fp16(scale * row)
// tiles [n_pad][dp] and start values auxp16 of the one-product scan, with the rows' largest fp16 residual (scaled units);
// largest norm and bf16 residual of the rows the tiles were cut from (centred cosine / angular: the augmented rows).
struct BfF32Tiles {
    void *hi, *lo;
    float* auxp;
    void* h16;
    float* auxp16;
    float scale, bres16;
    int dp;
    float bmax, bres;
};
// src rows [n][ld] of `cols` columns -> the tiles of dst, n_pad rows of dst.dp columns each; auxp = aux (null: 0),
// auxp16 = aux * aux16_mul, both aux_pad behind the n rows
struct BfSplitSrc {
    const float* rows;
    int n, n_pad, ld, cols;
};
hipError_t launch_split_bf16(const BfSplitSrc& src, const float* aux, float aux_pad, float aux16_mul, const BfF32Tiles& dst,
                             hipStream_t s);
hipError_t launch_bf_f32_fast(const BfF32Fast& f, int space, int nq, int k, const BfF32Rows& rows, const BfF32Tiles& tiles,
                              const BfF32Queries& q, const BfFastWs& ws, const BfOut& out, const BfScanEvents& ev,
                              hipStream_t s);
// centred cosine / angular on the fast path: augmented rows / queries (see row_aug_cosc_kernel)
hipError_t launch_row_aug_cosc(const float* orig, const float* centred, int n, int ldb, int dim, double mu_norm, float lambda,
                               float* out, int ldo, int* zero_rows, hipStream_t s);
hipError_t launch_query_aug_cosc(const float* centred, const float* qaux, int nq, int qpad, int ldb, int dim, float lambda,
                                 float* out, int ldo, hipStream_t s);

// l1 fast path for large batches (bf_l1_kernels.hip: v_sad_u8 filter scan over an 8-bit copy of the rows, exact f32
// re-rank of the per-split lists, per-query proof, adaptive fallback for flagged tiles).  Exact like the adaptive path.
constexpr int BF_L1_MAX_DIM = 256;    // a SAD over 256 bytes still fits the 16-bit score field of the scan's keys
constexpr int BF_L1_ROW_TILE = 128;   // rows per scan step: the copy is padded to a multiple of it
inline int bf_l1_rows_padded(int n) { return (n + BF_L1_ROW_TILE - 1) / BF_L1_ROW_TILE * BF_L1_ROW_TILE; }
struct BfL1Fast {
    bool use;
    int d4;                            // dwords per row of the copy: ceil(dim / 4)
    int qpad, nqt;                     // queries padded to BF_TQ; query tiles
    int nsplit, rows_per_split;        // row splits, each with its own lists
    int kprime;                        // keys kept per (query, split)
    size_t lds_scan;
    BfPlan list;                       // the lists as launch_bf_rerank reads them (nsplit, cap = kprime, p2max)
    BfPlan fallback;                   // plan of the adaptive kernel for the fallback
};
BfL1Fast bf_l1_fast_plan(int n, int dim, int nq, int k);
// The copy as finalize leaves it: u8 [n_pad / 64][d4][64] dwords (dword j of row r at ((r / 64) * d4 + j) * 64 + r % 64),
// the columns' smallest and largest elements, their largest residuals and the common step (l1_quant.hpp)
struct BfL1Rows {
    const uint32_t* u8;
    const float *lo, *hi, *rmax;
    double step;
};
// Per-batch workspace: qt [d4][qpad] dwords, xe [qpad][2] doubles (excess, bound), cand / cnt of the lists
// ([qpad][nsplit][kprime] keys, [qpad][nsplit] counts), flags [nqt], fb: the adaptive fallback's survivors (f.fallback)
struct BfL1Ws {
    uint32_t* qt;
    double* xe;
    BfCand cand;
    int* flags;
    BfCand fb;
};
// range [2 * ld + 1] words: per column the smallest, then the largest element as ordered bits (larger float -> larger
// word: bits ^ 0x80000000 for positive floats, ~bits for negative ones), then a flag for non-finite elements.  ld <= 256.
hipError_t launch_l1_col_range(const float* rows, int n, int ld, int dim, uint32_t* range, hipStream_t s);
// rows -> the byte copy (bf_l1_rows_padded(n) rows) and rmax_bits [dim]: the largest residuals, f32 bits rounded up
hipError_t launch_l1_quantise_rows(const float* rows, int n, int ld, int dim, const float* lo, double step, uint32_t* out,
                                   uint32_t* rmax_bits, hipStream_t s);
hipError_t launch_bf_l1_fast(const BfL1Fast& f, int nq, int k, const BfF32Rows& rows, const BfL1Rows& copy,
                             const float* queries_raw, float* queries_padded, const BfL1Ws& ws, const BfOut& out,
                             const BfScanEvents& ev, hipStream_t s);

// one pair, one wave (nmslib_get_distance)
hipError_t launch_pair_distance(int space, const void* a, const void* b, int dim, float* out,
                                hipStream_t s);

// ---- HNSW search -------------------------------------------------------------------------
struct HnswDeviceGraph {
    const void* rows;          // f32 [n][ldv] or u8 [n][128]
    const int32_t* row_norm;   // u8: sum of squares per row
    const int32_t* links0;     // [n][maxM0+1]  (count, ids...)
    const int64_t* up_off;     // [n] offset into up_links (ints) or -1
    const int32_t* up_links;   // per node: level blocks of (maxM+1) ints
    const int32_t* ext_ids;    // internal position -> external id
    int n, dim, ldv;
    int maxM, maxM0, maxlevel, enterpoint;
    int space;                 // search-time SpaceCode (SP_L2SQR, SP_NORMCOS, ...)
    int normalize_query;       // cosine on the optimized index
    // fp16 traversal copy of the f32 rows (gpu_rows=f16; null without one): fp16(2^e * row), row stride ld16 halves (a
    // multiple of 8, zero padded), inv_scale16 = 2^-e
    const void* rows16;
    int ld16;
    float inv_scale16;
};
struct HnswSearchPlan {
    int nq, k, ef, cap;        // cap = max(ef, k)
    int table_size;            // LDS visited hash entries (power of two); 0 -> global bitset
    size_t lds_bytes;
    size_t bitset_words;       // per query, when table_size == 0
    int table_shift;           // hash -> slot of the LDS table: 32 - log2(table_size); 0 without a table
    // SearchOld kernel only (hnsw_make_plan_old): candidate heap and queue placement
    int heap_lds, heap_cap;    // heap entries in LDS / in total per query (the rest lives in the HBM workspace)
    int a_in_lds, r_in_lds;    // closest-queue values (ef floats) / result queue (k pairs) in LDS?
    int rows_f16;              // launch_hnsw_search: the walk reads g.rows16 and emits its array for the re-rank: array order,
                               // internal positions (set by the caller; the planners leave 0)
};
// entries of the frontier arrays: a multiple of 64 that holds the longest adjacency list (level 0 or above)
inline int hnsw_nbcap(const HnswDeviceGraph& g) {
    const int longest = g.maxM0 > g.maxM ? g.maxM0 : g.maxM;
    return longest <= 62 ? 64 : (longest + 64) / 64 * 64;
}
// Narrow or wide adjacency lists: a list of up to 62 entries is one word a lane (count, ids, one lane spare); the WIDE
// instantiations of every search kernel walk longer lists in chunks.  The launch functions choose by this alone.
inline bool hnsw_wide(const HnswDeviceGraph& g) { return g.maxM0 > 62 || g.maxM > 62; }
// 64-entry registers a lane of the LDS kernels' sorted array (their EMAX): 2, 4 or 16 for cap = max(ef, k) up to 128, 256, 1024
inline int hnsw_emax(int cap) { return cap <= 128 ? 2 : cap <= 256 ? 4 : 16; }

// the LDS search kernels hold frontiers of up to this many neighbours (lists up to 255 entries: hnsw_nbcap leaves one entry
// spare); longer lists go to the HBM-array kernel
constexpr int HNSW_NBCAP_LDS = 256;

// What a workgroup may take of a gfx950 CU's LDS.  Every search kernel stages the query row there, so rows beyond some
// 40 000 floats fit none of them: the launch functions refuse such a plan with hipErrorInvalidValue instead of launching.
constexpr size_t HNSW_LDS_LIMIT = 160 * 1024;
// dynamic LDS of the HBM-array kernel (hnsw_search_big_kernel): the query row, the frontier arrays, the accepted items
inline size_t hnsw_big_lds(const HnswDeviceGraph& g) {
    return (g.space == SP_L2SQR_SIFT ? 128 : (size_t)g.ldv * 4) + (size_t)(2 * hnsw_nbcap(g) + 2 * 64) * 4 + 16;
}

HnswSearchPlan hnsw_make_plan(const HnswDeviceGraph& g, int nq, int k, int ef, bool force_bitset);
// Plan of the SearchOld kernel (hnsw_distfunc_opt.cc:46-150): no limit on ef or k.  heap_cap = 0 picks the default
// bound on the candidate heap (queries that outgrow it report status 2 and are retried with heap_cap = n).
HnswSearchPlan hnsw_make_plan_old(const HnswDeviceGraph& g, int nq, int k, int ef, bool force_bitset, int heap_cap);
// per-query HBM workspace of the SearchOld kernel, in bytes (0 = nothing spills)
inline size_t hnsw_old_ws_a(const HnswSearchPlan& p) { return p.a_in_lds ? 0 : (size_t)p.ef * 4; }
inline size_t hnsw_old_ws_r(const HnswSearchPlan& p) { return p.r_in_lds ? 0 : (size_t)p.k * 8; }
inline size_t hnsw_old_ws_heap(const HnswSearchPlan& p) { return (size_t)(p.heap_cap - p.heap_lds) * 8; }

// ---- the named parts of a search launch (host side) ----
// Where a launch writes: k results per query, then one entry per query of the result count, the work counters (ndc, hops
// on the search level, hops above it; each optional) and the status (optional).
struct HnswOut {
    int32_t* ids;
    float* dists;
    int32_t *cnt, *ndc, *hops, *hops_up, *status;
    // the block of the queries from q0 on, k results each
    HnswOut at(size_t q0, size_t k) const {
        auto from = [q0](int32_t* p) { return p ? p + q0 : p; };
        return {ids + q0 * k, dists + q0 * k, from(cnt), from(ndc), from(hops), from(hops_up), from(status)};
    }
};
// Where the queries come from.  External: [nq][dim] f32 (row stride dim) or u8 [nq][128].  Construction mode
// (hnsw_build): the queries are stored rows (query_rows), the best-first phase runs on `level`, start_nodes[q] >= 0 gives
// the start node (else descend from the entry point to level + 1).
struct HnswQueries {
    const void* queries;
    const int32_t* query_rows;
    const int32_t* start_nodes;
    int level;
    static HnswQueries external(const void* queries) { return {queries, nullptr, nullptr, 0}; }
    static HnswQueries stored(const int32_t* query_rows, const int32_t* start_nodes, int level) {
        return {nullptr, query_rows, start_nodes, level};
    }
};
// Visited-table overflow handled on the device (no host round trip); null / zero = not in use:
//   1. LDS-table plan:  fix_slots = 0, fix_list / fix_count given -> overflowed queries are appended to fix_list;
//   2. bitset plan:     fix_slots = S > 0 -> S workgroups walk fix_list (count read on the device), each clearing and
//      using its own bitset slot (bitset must hold S * bitset_words words) and overwriting those queries' outputs.
struct HnswOverflow {
    int fix_slots;
    int32_t* fix_list;
    int32_t* fix_count;
};

// SearchV1Merge with max(ef, k) <= 1024 (the sorted array in LDS).  status[q] != 0 -> the visited table overflowed (a
// caller without an overflow list re-runs those with a bitset plan).
hipError_t launch_hnsw_search(const HnswDeviceGraph& g, const HnswSearchPlan& p, const HnswQueries& q, uint32_t* bitset,
                              const HnswOverflow& fix, const HnswOut& out, hipStream_t s);
// fp16(scale * rows) -> rows16 [n][ld16] (f16_pack.hpp's rounding; columns dim .. ld16 are zero)
hipError_t launch_hnsw_pack_rows16(const float* rows, int n, int ldv, int dim, float scale, void* rows16, int ld16,
                                   hipStream_t s);
// Exact f32 re-rank behind an fp16 walk.  cand [nq][cap]: the sorted arrays of the walk as internal positions (what a
// launch with rows_f16 and k = cap writes: the fp16 kernels emit array order and positions), cand_n [nq] their lengths.  One wave per query: f32 distances of
// the first min(rerank, cand_n) entries on g.rows (the bits the f32 walk computes for those rows), ordered by (distance,
// position); k results with external ids, -1 / +inf padding and the count go to out.
hipError_t launch_hnsw_rerank(const HnswDeviceGraph& g, int nq, int k, int cap, int rerank, const void* queries,
                              const int32_t* cand, const int32_t* cand_n, const HnswOut& out, hipStream_t s);
// A batch in which every query names its own filter: the filters of the batch as a device table, and per
// query of a launch its entry's index.  allow: the filter's bits over n_allow positions; list: its m ascending positions (the
// subset route; null on the walk route).  A workgroup serves one query: it reads slot[q] and the entry once, into scalars.
struct FilterSlot {
    const uint32_t* allow;
    const int32_t* list;
    int n_allow, m;
};
struct FilterEach {
    const FilterSlot* table;
    const int32_t* slot;  // [nq] of the launch (a slice passes slot + q0)
};
// Deleted rows and filtered batches (hnsw_live_kernels.hip): cand / cand_d [nq][cap] are the results of a search launched for
// cap results without ext_ids (internal positions, in the search's order), cand_n [nq] their counts.  One wave per query: the
// first k entries whose position is below n_allow with its bit in allow set (allow optional) and whose bit in tomb ([ceil(n /
// 32)] words, bit = position; optional; at least one of the two is given) is clear, in their order, with external ids; -1 /
// +inf padding and the count go to out (out.cnt is required).  Nothing beyond cand_n[q] entries is read.
hipError_t launch_hnsw_keep_topk(const int32_t* cand, const float* cand_d, const int32_t* cand_n, int nq, int cap,
                                 const uint32_t* allow, int n_allow, const uint32_t* tomb, int n, const int32_t* ext_ids,
                                 int k, const HnswOut& out, hipStream_t s);
// ... with query q filtered by the bits of each.table[each.slot[q]] (every slot names an entry with bits)
hipError_t launch_hnsw_keep_topk_each(const int32_t* cand, const float* cand_d, const int32_t* cand_n, int nq, int cap,
                                      const FilterEach& each, const uint32_t* tomb, int n, const int32_t* ext_ids, int k,
                                      const HnswOut& out, hipStream_t s);
// The same two tests inside the walk (hnsw_inwalk_kernels.hip): disallowed and deleted nodes are stepping
// stones, only eligible ones enter the result set of cap = max(ef, k) entries, and the walk goes on until that set is full.
// One wave per query on the f32 rows (u8 rows: the integer distance); bitset [nq][bitset_words >= ceil(n / 32)], cleared by
// the caller; allow / tomb as above (both optional).  k results with external ids in (distance, position) order, -1 / +inf
// padding, the count and the walk's counters go to out.  Served shapes: inwalk_served (hnsw_inwalk_plan.hpp); any other is
// hipErrorInvalidValue.
hipError_t launch_hnsw_inwalk(const HnswDeviceGraph& g, int nq, int k, int ef, const void* queries, uint32_t* bitset,
                              size_t bitset_words, const uint32_t* allow, int n_allow, const uint32_t* tomb, const HnswOut& out,
                              hipStream_t s);
// ... with query q's allow bits those of each.table[each.slot[q]]
hipError_t launch_hnsw_inwalk_each(const HnswDeviceGraph& g, int nq, int k, int ef, const void* queries, uint32_t* bitset,
                                   size_t bitset_words, const FilterEach& each, const uint32_t* tomb, const HnswOut& out,
                                   hipStream_t s);
// SearchOld; ws_a / ws_r / ws_heap: the per-query HBM workspaces above (may be unused)
hipError_t launch_hnsw_search_old(const HnswDeviceGraph& g, const HnswSearchPlan& p, const void* queries, uint32_t* bitset,
                                  void* ws_a, void* ws_r, void* ws_heap, const HnswOut& out, hipStream_t s);
// SearchV1Merge with max(ef, k) beyond the LDS kernels' 1024 items: the sorted array in a per-query HBM workspace
// (ws_keys / ws_idu: [nq][max(ef, k)]), visited set = HBM bitset [nq][ceil(n / 32)] (cleared by the caller).
hipError_t launch_hnsw_search_big(const HnswDeviceGraph& g, int nq, int k, int ef, const void* queries, uint32_t* bitset,
                                  float* ws_keys, int32_t* ws_idu, const HnswOut& out, hipStream_t s);

// ---- filtered search (filter_kernels.hip) ---------------------------------------
// the subset-scan kernel's capacity: 32 KB of 64-bit keys, which with the query stays under 64 KB of LDS
constexpr int HNSW_SUBSET_MAX = 4096;
// Ordered compaction of a bitset, in two steps (the caller sizes the list from the count in between).
// Device row r stands at position row_pos[r] (row_pos = nullptr: r itself).  A row is taken when its position is below n_pos,
// its bit in allow ([ceil(n_pos / 32)] words, bit = position) is set and its bit in tomb (optional; covers every position
// below n_pos) is clear.  Bits at or beyond n_pos are never read as set, also in the last word.
// count: mask / prefix [ceil(n_rows / 32)] words each (32 rows per word: who is taken, how many are taken in the words
// before), *count = rows taken.  write: list[0 .. *count) = the rows taken, ascending.
hipError_t launch_filter_count(const uint32_t* allow, int n_pos, const uint32_t* tomb, const int32_t* row_pos, int n_rows,
                               uint32_t* mask, int32_t* prefix, int32_t* count, hipStream_t s);
hipError_t launch_filter_write(const uint32_t* mask, const int32_t* prefix, int n_rows, int32_t* list, hipStream_t s);
// dst row i = src row list[i] for i < m; rows of row_bytes bytes (a multiple of 16; both matrices 16-byte aligned)
hipError_t launch_filter_gather_rows(const void* src, const int32_t* list, int m, size_t row_bytes, void* dst, hipStream_t s);
// dst[i] = src[list[i]]
hipError_t launch_filter_gather_ids(const int32_t* src, const int32_t* list, int m, int32_t* dst, hipStream_t s);
// (the walk route's result filter is launch_hnsw_keep_topk above)
// Exact k-NN over the m <= HNSW_SUBSET_MAX positions of list (ascending), one workgroup per query: the distances of the f32
// walk on g.rows (u8 rows: the integer distance), rows with their bit in tomb (optional) set left out, order (distance,
// position).  out: k results with external ids, -1 / +inf padding, the count; ndc = m, hops = hops_up = 0.
// the bytes of a staged query: ldv floats, or the 128 bytes of a u8 query (what filter_plan.hpp's LDS arithmetic takes)
inline size_t hnsw_subset_query_bytes(const HnswDeviceGraph& g) { return g.space == SP_L2SQR_SIFT ? 128 : (size_t)g.ldv * 4; }
hipError_t launch_hnsw_subset_knn(const HnswDeviceGraph& g, int nq, int k, const void* queries, const int32_t* list, int m,
                                  const uint32_t* tomb, const HnswOut& out, hipStream_t s);
// ... with query q scanning the list of each.table[each.slot[q]] (m may be 0: count 0).  One launch: the LDS is sized for
// m_max, the largest m among the launch's queries; a workgroup sorts the filter_subset_keys of its own m.
hipError_t launch_hnsw_subset_knn_each(const HnswDeviceGraph& g, int nq, int k, const void* queries, const FilterEach& each,
                                       int m_max, const uint32_t* tomb, const HnswOut& out, hipStream_t s);
// dst row i = src row list[i] for rows of any multiple of 4 bytes (results of k entries, counters): word by word
hipError_t launch_filter_gather_words(const void* src, const int32_t* list, int m, size_t row_bytes, void* dst, hipStream_t s);

// ---- HNSW construction on the GPU (hnsw_build_kernels.hip) ------------------------------------
struct HnswBuildGraph {          // mutable twin of HnswDeviceGraph
    HnswDeviceGraph g;           // rows, links0, up_off, up_links (written by the link kernels)
    int32_t* links0;             // same memory as g.links0, non-const
    int32_t* up_links;
    int M, delaunay;
};
// starts[i] = first (closest) candidate of pair src[i] (src[i] < 0 or empty -> -1 = descend from the entry point)
hipError_t launch_hnsw_build_starts(const int32_t* src, const int32_t* cand_ids, const int32_t* cand_n, int stride,
                                    int32_t* starts, int m, hipStream_t s);
// Heuristic neighbour selection (delaunay 2: heuristic 2, 1: heuristic 1, 0: the M closest; M <= 127, maxM0 <= 254)
// for the `npts` new nodes listed in pts at `level`: reads the sorted candidates
// (cand_ids/cand_d/cand_n, stride `stride`), writes each new node's forward list, and one reverse-link request per
// selected neighbour into the node's own M slots: req_key [npts][M] = target << 32 | new node (unused: ~0), req_dist.
hipError_t launch_hnsw_build_select(const HnswBuildGraph& bg, int level, const int32_t* pts, int npts,
                                    const int32_t* cand_ids, const float* cand_d, const int32_t* cand_n,
                                    int stride, const int32_t* extra_ids, const float* extra_d,
                                    const int32_t* extra_n, unsigned long long* req_key, float* req_dist,
                                    hipStream_t s);
// Batch-mates: for every new node of the level slice, the EARLIER nodes of the slice that are closer than its worst
// candidate (at most 64, ascending): extra_ids/extra_d [npts][64], extra_n [npts].  Merged by the select kernel.
hipError_t launch_hnsw_build_mates(const HnswBuildGraph& bg, int level, const int32_t* pts, int npts,
                                   const float* cand_d, const int32_t* cand_n, int stride, int32_t* extra_ids,
                                   float* extra_d, int32_t* extra_n, hipStream_t s);
// Device radix sort of the requests by (target, new node) + the index of each target's first request (active/nactive).
size_t hnsw_build_sort_temp_bytes(int max_requests, int n);
hipError_t launch_hnsw_build_sort_requests(const unsigned long long* req_key, const float* req_dist, int total,
                                           unsigned long long* key_sorted, float* dist_sorted, void* temp,
                                           size_t temp_bytes, int32_t* active, int32_t* nactive, hipStream_t s);
// Apply the sorted reverse links target by target (addFriendlevel + shrink, hnsw.h:258-314), any number per target.
hipError_t launch_hnsw_build_link(const HnswBuildGraph& bg, int level, const int32_t* active,
                                  const int32_t* nactive, int max_active, const unsigned long long* key_sorted,
                                  const float* dist_sorted, int total, hipStream_t s);
// Post-processing (hnsw.cc:251-330) over the level-0 lists ([n][maxM0 + 1]) of the graph built in reverse order
// (`second`) and the one built in insertion order (`first`), one wave per node: mode 1 writes the union (second's
// entries, then first's new ones; out_stride >= 2 * maxM0 + 1), mode 2 the union ranked again and cut to maxM0
// (delaunay 0: the closest, else heuristic 1), farthest first.  `out` must be cleared; max_len (or NULL) receives the
// longest list by atomicMax.  maxM0 <= 254.
hipError_t launch_hnsw_build_post(const HnswDeviceGraph& g, const int32_t* second, const int32_t* first, int maxM0,
                                  int mode, int delaunay, int32_t* out, int out_stride, int32_t* max_len,
                                  hipStream_t s);
// lists of stride sstride copied into lists of stride dstride (unused slots 0)
hipError_t launch_hnsw_build_repack(const int32_t* src, int sstride, int32_t* dst, int dstride, int n, hipStream_t s);

// ---- consolidating a graph with deleted rows (hnsw_consolidate_kernels.hip) ----
struct HnswConsolidate {
    HnswDeviceGraph g;           // the resident graph over all n rows, deleted ones included
    int32_t* links0;             // same memory as g.links0 / g.up_links, non-const: lists are repaired in place
    int32_t* up_links;
    const uint32_t* tomb;        // bit = position, [ceil(n / 32)] words
    const int32_t* levels;       // [n]
    int delaunay, P;             // selection (0, 1, 2); candidates kept per list (1 .. 1024)
    unsigned long long* ndist;   // optional (device): the repair adds its distance evaluations (rows fetched) to it
};
// Every (node, level) list of a live node that holds a deleted entry -> work [work_cap][2] (node, level), in any order;
// *nwork (cleared by the caller) counts them.
hipError_t launch_hnsw_cons_worklist(const HnswConsolidate& c, int32_t* work, int work_cap, int32_t* nwork, hipStream_t s);
// One wave per worklist entry: the list keeps its live entries and is filled up to its old length from the live
// neighbours of its deleted entries (the P closest, by (distance, position); delaunay 2 and 1: a candidate is taken unless
// a kept node is strictly closer to it than the list's node; 1: then the closest rejected ones; 0: the closest).  In place.
hipError_t launch_hnsw_cons_repair(const HnswConsolidate& c, const int32_t* work, int nwork, hipStream_t s);
// Rows of row_bytes (a multiple of 4) each: row r of src goes to row newpos[r] of dst unless its tombstone bit is set.
hipError_t launch_hnsw_cons_scatter_rows(const void* src, void* dst, size_t row_bytes, int n, const uint32_t* tomb,
                                         const int32_t* newpos, hipStream_t s);
// The same for level-0 lists of `stride` ints (count, entries): entries are renumbered by newpos, unused slots become 0.
hipError_t launch_hnsw_cons_links0(const int32_t* src, int32_t* dst, int stride, int n, const uint32_t* tomb,
                                   const int32_t* newpos, hipStream_t s);
// ... and for the upper-level blocks of the nup live nodes listed in up_nodes (old positions): block old_off[u] of
// levels[u] * (maxM + 1) ints goes to new_off[newpos[u]].
hipError_t launch_hnsw_cons_up_links(const int32_t* src, const int64_t* old_off, const int32_t* levels, int32_t* dst,
                                     const int64_t* new_off, const int32_t* up_nodes, int nup, int maxM, int n,
                                     const int32_t* newpos, hipStream_t s);

// ---- range search on the brute-force index (range_kernels.hip) ----------------------------------
// dist_ws[r] = the reference's distance of row r to the query, r < n
hipError_t launch_range_dist(int space, const void* rows, int ld, int n, const void* query_padded, int dim,
                             float* dist_ws, hipStream_t s);

// Exact scan for k > BF_MAX_K: per query one pass with the reference formula + one stable device radix sort of
// (distance, position).  Workspace: dist [n] floats, keys [4][n] u32, temp of bf_bigk_temp_bytes(n).
size_t bf_bigk_temp_bytes(int n);
struct BfBigkWs {
    float* dist;
    uint32_t* keys;
    void* temp;
    size_t temp_bytes;
};
hipError_t launch_bf_bigk(int space, const void* rows, int ld, int n, int dim, const void* queries_padded,
                          size_t query_stride_bytes, int nq, int k, const BfBigkWs& ws, const BfOut& out, hipStream_t s);

// count_ws: [range_count_elems(n)] ints, the last one receives the number of matches.
inline size_t range_count_elems(int n) { return (size_t)(n + 1023) / 1024 + 1; }
// Range selection over a precomputed distance array: the matches of `filter` (distance <= radius), in position order,
// the first `capacity` of them, each reported with report[position] (a symmetric distance passes filter twice).
hipError_t launch_range_select(const float* filter, const float* report, int n, float radius, const int32_t* ext_ids,
                               int* count_ws, int capacity, int32_t* out_ids, float* out_dists, hipStream_t s);

// ---- batched range search on the brute-force index (range_batch_kernels.hip) -----
// One slice of a batch (range_batch_plan.hpp): match bits of every (query, row), counts per 1024-row block, a scan per
// query, then the first `capacity` matches of every query in position order, -1 / +inf behind them.  Every distance is
// the value wave_exact_distance_f32 / _u8 returns, so row q equals launch_range_dist + launch_range_select for query q.
struct RangeBatchArgs {
    int space;
    const void* rows;        // [n][ld] floats, or [n][128] bytes (l2sqr_sift)
    int ld, n, dim;          // float rows: dim <= kRangeBatchMaxDim
    const void* queries;     // [nq][dim] elements, unpadded, element alignment
    int nq;                  // <= kRangeBatchMaxSliceQueries
    const float* radii;      // [nq], device
    size_t capacity;         // per query; 0: count only (out_ids / out_dists unused)
    int32_t* out_ids;        // [nq][capacity]
    float* out_dists;
    int32_t* out_counts;     // [nq] min(total, capacity); may be null
    int32_t* out_totals;     // [nq]; may be null
    const int32_t* ext_ids;  // [n]
    unsigned long long* masks;  // workspace: [nq][mask_words]
    size_t mask_words;          // ceil(n / 64)
    int* counts;                // workspace: [nq][ceil(n / 1024) + 1]
    unsigned grid_x, grid_y;    // the match-bit kernel's grid (the plan's)
    bool pad;                   // write -1 / +inf behind the entries a query gets (false: the caller pads)
};
hipError_t launch_range_batch(const RangeBatchArgs& a, hipStream_t s);
// Behind launch_range_select of one query into a row of a batch's outputs (*total = its count_ws total): the query's count
// and total (either may be null) and, with pad, the padding of its row.
hipError_t launch_range_batch_finish(const int* total, size_t capacity, int32_t* out_ids, float* out_dists,
                                     int32_t* out_count, int32_t* out_total, bool pad, hipStream_t s);

// ---- exact scans over sparse and string rows: the plan they share ---------------------------------
// A scan's grid is (row splits, query tiles); each workgroup keeps the best kl keys of its split per query of its tile
// (kernels/split_topk_dev.hpp) and writes them as ascending lists that launch_merge_topk_ex merges.
constexpr int kScanMaxKl = 4096;  // for k above this a split holds at most this many rows (its list keeps them all)
struct ScanPlan {
    int n, nq, k;
    int nsplit, rows_per_split;  // row ranges scanned by separate workgroups
    int kl;                      // keys kept per (split, query) = min(k, rows_per_split)
    int P;                       // LDS key buffer per query (power of two >= kl + 256)
    int tq;                      // queries per workgroup (the tq asked for, or 1 when k is large)
};
inline int pow2_at_least(int v) {
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}
inline ScanPlan scan_make_plan(int n, int nq, int k, int tq) {
    ScanPlan p{};
    p.n = n;
    p.nq = nq;
    p.k = k;
    // enough workgroups to fill the chip (256 CUs, 8 per CU) without splitting rows finer than 1024 per workgroup;
    // a workgroup takes a tile of tq queries when k is small
    const long long tiles = ((long long)nq + tq - 1) / tq;
    const long long want = (2048 + tiles - 1) / (tiles > 0 ? tiles : 1);
    long long rps = ((long long)n + want - 1) / (want > 0 ? want : 1);
    if (rps < 1024) rps = 1024;
    // the split lists of a query merge in LDS while nsplit * k <= 8192 (launch_merge_topk_ex)
    if (k <= 4096) {
        const long long per = 8192 / k;
        const long long rps_merge = ((long long)n + per - 1) / per;
        if (rps < rps_merge) rps = rps_merge;
    }
    if (k > kScanMaxKl) rps = kScanMaxKl;  // then a split's list holds every row of the split
    p.rows_per_split = (int)rps;
    p.nsplit = n > 0 ? (int)(((long long)n + rps - 1) / rps) : 1;
    p.kl = (int)(k < rps ? k : rps);
    p.P = pow2_at_least(p.kl + 256);
    p.tq = p.P <= 1024 ? tq : 1;  // the tile's key buffers: 8 x 8 KiB at most
    return p;
}

// ---- sparse vectors (sparse_kernels.hip) -----------------------------------------------------
// Rows and queries are CSR: row_ptr int64 [n+1], ids uint32, vals f32.  Spaces: SP_L2, SP_L1, SP_LINF, SP_COSINE,
// SP_ANGULAR, SP_NEGDOT, SP_QNORM_NEGDOT, each evaluated over the union of the two id lists.
constexpr int kSparseQCap = 4096;   // query elements staged in LDS by the k-NN scan (longer: read from HBM)
constexpr int kSparseTileQ = 8;     // queries per workgroup of the k-NN scan (k small enough for 8 key buffers in LDS)
// per-(split, query) lists, ascending (distance, position): split_d / split_pos [nsplit][nq][k]; merged by
// launch_merge_topk_ex with shard_stride nq*k
hipError_t launch_sparse_knn(int space, const ScanPlan& p, const int64_t* row_ptr, const uint32_t* ids,
                             const float* vals, const int64_t* q_ptr, const uint32_t* q_ids, const float* q_vals,
                             float* split_d, int32_t* split_pos, hipStream_t s);
// d_row_q[r] = distance(row r, query), d_q_row[r] = distance(query, row r)
hipError_t launch_sparse_dist(int space, const int64_t* row_ptr, const uint32_t* ids, const float* vals, int n,
                              const uint32_t* q_ids, const float* q_vals, int qn, float* d_row_q, float* d_q_row,
                              hipStream_t s);
// *out = distance(row p1, row p2)
hipError_t launch_sparse_pair(int space, const int64_t* row_ptr, const uint32_t* ids, const float* vals, int p1, int p2,
                              float* out, hipStream_t s);

// ---- strings (string_kernels.hip) -----------------------------------------------------------
// leven rows: CSR bytes (row_ptr int64 [n+1], data uint8).  Queries: Peq tables, [nw][256] uint64 per query at
// q_off[q] (uint64 units, q_off [nq+1]), nw = ceil(len / 64), and their lengths q_len.
// bit_hamming rows and queries: W uint32 words each (the reference's trailing count word is not stored).
constexpr int kStrTileQ = 8;              // queries per workgroup of a k-NN scan (one-block leven queries, bit_hamming)
constexpr size_t kStrPeqStage = 16384;    // bytes of Peq tables staged in LDS per workgroup (more: read from HBM)
constexpr size_t kStrRowStage = 16384;    // bytes of a 256-row chunk staged in LDS (a longer chunk: read from HBM)
constexpr int kStrMwLds = 4;              // multi-block leven: blocks whose state a lane keeps in LDS (more: HBM)
constexpr size_t kStrHamQStage = 16384;   // bytes of bit_hamming queries staged in LDS per workgroup
// HBM state of a multi-block leven scan (uint64 words; 0 when it fits LDS)
size_t leven_mw_ws_words(const ScanPlan& p, int nw);
// per-(split, query) lists, ascending (distance, position): split_d / split_pos [nsplit][nq][k]; merged by
// launch_merge_topk_ex with shard_stride nq*k.  nw = the batch's largest block count (nw > 1 needs p.tq == 1).
hipError_t launch_leven_knn(const ScanPlan& p, const int64_t* row_ptr, const uint8_t* data,
                            const int64_t* q_off, const int32_t* q_len, const uint64_t* peq, int nw, uint64_t* mw_ws,
                            float* split_d, int32_t* split_pos, hipStream_t s);
hipError_t launch_ham_knn(const ScanPlan& p, const uint32_t* rows, int W, const uint32_t* q, float* split_d,
                          int32_t* split_pos, hipStream_t s);
// d_out[r] = distance(row r, query); leven: mw_ws holds 2 * nw * 256 * leven_dist_grid(n) words when nw > 1
int leven_dist_grid(int n);
hipError_t launch_leven_dist(const int64_t* row_ptr, const uint8_t* data, int n, const uint64_t* peq, int m, int nw,
                             uint64_t* mw_ws, float* d_out, hipStream_t s);
hipError_t launch_ham_dist(const uint32_t* rows, int W, int n, const uint32_t* q, float* d_out, hipStream_t s);
// *out = distance(pattern, row p2), the pattern given by its Peq table (mw_ws: 2 * nw words when nw > 1)
hipError_t launch_leven_pair(const int64_t* row_ptr, const uint8_t* data, int p2, const uint64_t* peq, int m, int nw,
                             uint64_t* mw_ws, float* out, hipStream_t s);
hipError_t launch_ham_pair(const uint32_t* rows, int W, int p1, int p2, float* out, hipStream_t s);

// HNSW search over strings (baseSearchAlgorithmV1Merge / baseSearchAlgorithmOld), one wave per query.  Queries as
// for the scans (leven: Peq tables + lengths; bit_hamming: words).  Per query of a slice: vis_words of visited bits,
// ws_per_query u64 words (string_hnsw_ws_words) and 64 * 2 * nw_max u64 of leven block state.
struct StringHnswArgs {
    int space;
    const int64_t* row_ptr;
    const uint8_t* data;
    const uint32_t* words;
    int W;
    const int64_t* q_off;
    const int32_t* q_len;
    const unsigned long long* peq;
    const uint32_t* q_words;
    int nw_max;
    const int32_t* links0;
    const int64_t* up_off;
    const int32_t* up_links;
    const int32_t* ext_ids;
    int n, maxM, maxM0, maxlevel, enterpoint;
    int ef, k;
    uint32_t* visited;
    size_t vis_words;
    unsigned long long* ws;
    size_t ws_per_query;
    unsigned long long* mw_ws;
    int32_t* out_ids;
    float* out_d;
    int32_t* out_cnt;
    int32_t *ndc, *hops, *hops_up;
};
size_t string_hnsw_ws_words(const StringHnswArgs& a, bool old);
// queries [q0, q0 + nq) of the batch; workspaces hold nq queries
hipError_t launch_string_hnsw(const StringHnswArgs& a, bool old, int q0, int nq, hipStream_t s);

// ---- divergences over dense float rows (diverg_kernels.hip) ------------------------------------
// An object is its values and their logarithms (taken on the host), in groups of four elements, G = ceil(D / 4).
// Rows: two planes of [ceil(n / 64)][G][64][4] floats (diverg_row_plane_floats): group g of row r at float
// ((r / 64 * G + g) * 64 + r % 64) * 4.  Queries: planes of [G][stride][4] floats, group g of query q at
// (g * stride + q) * 4; inv = 1 / value, read by the k-NN scan of SP_ITAKURASAITO only.
constexpr int kDivergTileQ = 16;  // queries per workgroup of the k-NN scan (k small enough for 16 key buffers in LDS)
inline int diverg_groups(int D) { return (D + 3) / 4; }
inline size_t diverg_row_plane_floats(size_t n, int D) { return (n + 63) / 64 * (size_t)diverg_groups(D) * 256; }
struct DivergRows {
    const float *vals, *logs;
    int n, D, G;
};
struct DivergQueries {
    const float *vals, *logs, *inv;
    int stride;  // queries per group
};
// queries [q0, q0 + p.nq) of the pack, which holds kDivergTileQ more queries than the batch (a tile reads past its
// last query); per-(split, query) lists as for the sparse scan
hipError_t launch_diverg_knn(int space, const ScanPlan& p, const DivergRows& rows, const DivergQueries& q, int q0,
                             float* split_d, int32_t* split_pos, hipStream_t s);
// query 0 of the pack: d_row_q[r] = distance(row r, query), d_q_row[r] = distance(query, row r)
hipError_t launch_diverg_dist(int space, const DivergRows& rows, const DivergQueries& q, float* d_row_q, float* d_q_row,
                              hipStream_t s);
// *out = distance(object 0, object 1) of a pack with stride 2
hipError_t launch_diverg_pair(int space, const DivergQueries& objs, int D, float* out, hipStream_t s);

// ---- shard merge ---------------------------------------------------------------------------
// shard s's lists start at dists_in + s*shard_stride / ids_in + s*shard_stride (elements)
hipError_t launch_merge_topk(const float* dists_in, const int32_t* ids_in, size_t shard_stride, int nshards, int nq,
                             int k, float* dists_out, int32_t* ids_out, hipStream_t s);
// ... with the number of valid results per query (cnt_out, optional) and a final id map: ids in the lists are
// positions, ids_out[i] = ext_ids[position] (ext_ids optional)
hipError_t launch_merge_topk_ex(const float* dists_in, const int32_t* ids_in, size_t shard_stride, int nshards, int nq,
                                int k, float* dists_out, int32_t* ids_out, int32_t* cnt_out, const int32_t* ext_ids,
                                hipStream_t s);

}  // namespace gfxknn
