/*
 * nmslib_gpu.h -- device-resident extensions of the nmslib_c.h boundary.
 *
 * The reference's hot entry points (nmslib_knn_query_fill / _batch,
 * nmslib_c.cpp:941-1031) take host pointers and per-query result structs.  A
 * caller that already keeps its query batch in HBM (a serving loop, bench.py,
 * the multi-GPU shard merge) uses these entry points instead: same index handle,
 * same semantics, but plain *device* pointers in and out and an explicit HIP
 * stream, so nothing crosses PCIe inside the call.  No torch / C++ types in any
 * signature: pointers, sizes, and a `void*` that is a hipStream_t.
 *
 * Results layout: ids [query_count][k] int32 (external ids, -1 padding) and
 * distances [query_count][k] float32 (+inf padding), ascending per query, exactly
 * what nmslib_knn_query_fill would write into each nmslib_result_t
 * (extract_knn_results, nmslib_c.cpp:293-328); counts [query_count] int32.
 */
#ifndef NMSLIB_GPU_H
#define NMSLIB_GPU_H

#include "nmslib_c.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Number of HIP devices visible; 0 when the runtime finds none. */
int nmslib_gpu_device_count(void);

/* Make sure rows are resident in HBM and the index is built (what
 * nmslib_initialize_pool does lazily).  Returns the usual error codes. */
nmslib_error_t nmslib_gpu_finalize(nmslib_index_handle_t index);

/* Batched k-NN with queries already in device memory.
 *   d_queries : [query_count][elem_count] float32 (dense) or uint8 (l2sqr_sift), row-major
 *   d_ids / d_dists / d_counts : outputs in device memory (d_counts may be NULL)
 *   stream    : hipStream_t (NULL = default stream); the call only enqueues work -- with ONE exception: HNSW queries
 *               that the reference answers with SearchOld (algoType=old, or the default hybrid with efSearch >= 1000,
 *               hnsw.cc:724) read a per-query status word back and wait for the stream before returning (queues that
 *               outgrew their workspace are re-run with larger ones, at most twice).  Every other path -- brute force,
 *               both fast paths, SearchV1Merge incl. its visited-table overflow -- never blocks the caller.
 * Alignment: d_queries, d_ids, d_dists and d_counts need the alignment of their element type only (4 bytes; uint8
 *               queries: none).  Every kernel reads the caller's queries and writes the results element by element.
 * Order:     batches of one index are executed in the order of the calls, whatever streams they are given -- they
 *               share the index's workspaces.  A call on another stream than the index's previous work (a device batch,
 *               or a host-pointer entry of nmslib_c.h, which uses a stream of the index's own) first makes its stream
 *               wait for that work; the same stream again costs nothing.  The buffers passed to a call follow ordinary
 *               stream order on that call's stream: the queries must be ready there, the results are ready there.  A
 *               stream given to a call has to stay valid until the index has been given another one or is destroyed.
 * Replaces the per-query loop of nmslib_knn_query_batch (nmslib_c.cpp:1015-1023). */
nmslib_error_t nmslib_gpu_knn_query_batch_device(nmslib_index_handle_t index,
                                                 const void* d_queries, size_t query_count,
                                                 size_t elem_count, size_t k, int32_t* d_ids,
                                                 float* d_dists, int32_t* d_counts,
                                                 void* stream);

/* Per-query work counters of the most recent HNSW batch on this index (device
 * pointers, valid until the next batch; NULL for brute force):
 *   ndc  = distance computations (the DIST_CALC counters of hnsw_distfunc_opt.cc:76-78,128-130)
 *   hops = level-0 expansions, hops_up = upper-level adjacency reads. */
nmslib_error_t nmslib_gpu_last_batch_counters(nmslib_index_handle_t index,
                                              const int32_t** d_ndc, const int32_t** d_hops,
                                              const int32_t** d_hops_up);

/* Merge per-shard top-k lists (after an all-gather across ranks): for each query,
 * `nshards` ascending lists of k (distance, id) pairs -> the k smallest by
 * (distance, id).  Layout in: [nshards][query_count][k]; out: [query_count][k]. */
nmslib_error_t nmslib_gpu_merge_topk(const float* d_dists_in, const int32_t* d_ids_in,
                                     size_t nshards, size_t query_count, size_t k,
                                     float* d_dists_out, int32_t* d_ids_out, void* stream);

/* Same merge for per-shard lists that are not back to back: shard s starts at d_dists_in + s*shard_stride and
 * d_ids_in + s*shard_stride (elements).  Lets ONE all-gather move ids and distances together: every rank
 * contributes a packed [2][query_count][k] block (ids, then the distances' bit patterns), the gathered buffer is
 * [nshards][2][query_count][k] and shard_stride = 2*query_count*k. */
nmslib_error_t nmslib_gpu_merge_topk_strided(const float* d_dists_in, const int32_t* d_ids_in,
                                             size_t shard_stride, size_t nshards, size_t query_count,
                                             size_t k, float* d_dists_out, int32_t* d_ids_out,
                                             void* stream);

/* Live timing of the dominant kernel (bf_select_* for brute force, hnsw_search for HNSW) with
 * HIP events recorded on the stream the kernel is launched on.  enable != 0 starts recording
 * (one event pair per batch); a call with total_ms / launches non-NULL waits for the recorded
 * events, returns their summed duration and launch count, and clears the record. */
nmslib_error_t nmslib_gpu_kernel_timing(nmslib_index_handle_t index, int enable, double* total_ms,
                                        uint64_t* launches);

/* Engine statistics of the last finalize/build (host values). */
typedef struct {
    double upload_seconds;   /* host -> HBM copy of the rows            */
    double build_seconds;    /* index construction (HNSW graph)        */
    size_t hbm_bytes;        /* bytes resident in HBM for this index   */
    size_t rows;
    size_t dim;
    size_t shards;         /* row shards behind this handle (index parameter gpu_shards); 1 = single GPU */
    size_t last_path;      /* selection path of the last brute-force batch: 0 adaptive f32 MFMA, 1 bf16 fast path,
                              2 adaptive int8, 3 int8 fast path; 4 = HNSW; 5 = HNSW with the walk on the fp16 copy
                              of the rows and an f32 re-rank (gpu_rows=f16), and the brute-force scan for k > 512;
                              6 = l1 fast path (8-bit SAD filter, exact f32 re-rank); 7 = HNSW under a filter whose rows
                              were scanned exactly instead of walked (nmslib_gpu_filter_create); 8 = HNSW with the filter and
                              the tombstones tested inside the walk (query-time parameter gpu_inwalk=1); 9 = a batch with one
                              filter per query (nmslib_gpu_knn_query_batch_filtered_each: its `routes` has the paths).  A filtered
                              batch on an exact-scan index reports the path it took over the allowed rows; 10 = a batched
                              range query answered by the batched kernels (nmslib_gpu_range_query_batch), 11 = a batched
                              range query answered with the single-query launches, once per query */
    /* fast paths, last slice of the last batch (reading them waits for the stream): query tiles in the slice, tiles the
       threshold kernel sent through the split-bf16-product scan instead of the one-product scan (float rows only), and
       tiles whose verification failed and were redone by the adaptive kernel */
    size_t fast_tiles;
    size_t fast_tiles_precise;
    size_t fast_tiles_fallback;
    /* HNSW with the LDS visited table, last batch (reading it waits for the stream): queries whose table filled up and
       that the HBM-bitset kernel answered again.  0 on every BASELINE configuration.  SearchOld (algoType=old, hybrid from
       ef 1000 on): queries whose table filled up, on which the whole batch ran again with bitsets. */
    size_t hnsw_redone;
    /* the last finalize: rows it inserted into the graph that was resident (index parameter gpu_append=1; 0 = it built
       the index in full), and rows it copied from the host to HBM */
    size_t rows_appended;
    size_t rows_uploaded;
} nmslib_gpu_stats_t;
nmslib_error_t nmslib_gpu_get_stats(nmslib_index_handle_t index, nmslib_gpu_stats_t* out);

/* Which builder made the HNSW graph this index searches: *builder = 0 no graph (not built yet, not an HNSW index)
 * or a graph loaded from a file, 1 the host builder (the reference's graph at indexThreadQty=1), 2 the batched GPU
 * builder (index parameter gpu_build). */
nmslib_error_t nmslib_gpu_graph_builder(nmslib_index_handle_t index, int* builder);

/* The HNSW graph of a string index (data type 3), for inspection: *enterpoint, *maxlevel and, for node `node` at
 * `level`, its neighbour list (positions) in out[0 .. *count) when *count <= capacity.  level above the node's own
 * level -> NMSLIB_ERROR_INVALID_ARGUMENT.  Other indexes -> NMSLIB_ERROR_SPACE_INCOMPATIBLE. */
nmslib_error_t nmslib_gpu_string_hnsw_links(nmslib_index_handle_t index, size_t node, int level, int32_t* out,
                                            size_t capacity, size_t* count, int* enterpoint, int* maxlevel);

/* Deleted rows.  Marks every stored row whose external id is one of
 * ids[0 .. count) as deleted.  *marked (optional) = rows newly marked by this call.  Later k-NN and range results never contain
 * a marked row.
 *   A tombstone belongs to a position: the call marks the rows that carry the id when it is made (all of them -- ids need
 *   not be unique), and a row added later under the same id is live: "update" = delete the id, add the new row under it.
 *   An id no row carries, an id listed twice and a row marked already add nothing to *marked and are no errors.
 *   Positions do not move: nmslib_data_qty still counts the row, nmslib_get_data_point*, nmslib_borrow_data_dense and
 *   nmslib_get_distance still serve it.  nmslib_reset_index clears the marks with the rows; nmslib_create_index keeps them.
 *   nmslib_save_index on an index with a marked row -> NMSLIB_ERROR_DATA_IO_FAILED (no file format has a place for them).
 * Served: hnsw, brute_force and seq_search over the dense spaces (float rows and l2sqr_sift) on one device, before and after
 * nmslib_create_index, with or without a device (gpu_defer=1: host state until the index reaches the GPU).  Sparse, string
 * and divergence indexes and gpu_shards > 1 -> NMSLIB_ERROR_SPACE_INCOMPATIBLE.  ids == NULL with count > 0, or a NULL
 * handle -> NMSLIB_ERROR_NULL_POINTER.
 * hnsw: marked rows stay in the graph as stepping stones; a batch asked for k results is the first k unmarked entries of the
 * search for max(efSearch, k) results, so a count can fall below k when most of what the search finds is marked.  The call
 * is ordered with the index's other work like every host entry: a batch enqueued before it sees the old state.
 * hnsw with the query-time parameter gpu_inwalk=1 (nmslib_set_query_time_params; 0 or 1, default 0, stays as set; any other
 *   value -> NMSLIB_ERROR_INVALID_ARGUMENT; an unknown parameter for brute_force, seq_search and string or sparse graphs):
 *   a marked row does not count against efSearch.  The walk keeps two sets: the max(efSearch, k) closest unmarked rows found
 *   and the closest rows not yet expanded (at most 1024), marked ones among them; it goes on until no row left to expand is
 *   closer than the farthest result, so counts stay at k while the graph around the query holds k unmarked rows.  Served
 *   for max(efSearch, k) <= 1024 and maxM0 <= 254 on the f32 rows (also under gpu_rows=f16 and algoType=old: the rule is
 *   its own algorithm), last_path 8; any other batch runs the two stages above.  An index without marked rows, searched
 *   without a filter, runs what it runs without the parameter.
 * brute_force / seq_search: the index is prepared again at its next use, over the unmarked rows only. */
nmslib_error_t nmslib_gpu_delete_ids(nmslib_index_handle_t index, const int32_t* ids, size_t count, size_t* marked);
/* Rows of this index that are marked deleted. */
nmslib_error_t nmslib_gpu_deleted_rows(nmslib_index_handle_t index, size_t* count);

/* Consolidate: the rows marked by nmslib_gpu_delete_ids leave the
 * index.  *removed (optional) = rows dropped, *repaired (optional) = (node, level) adjacency lists that were rewritten.
 *   Positions move.  Live rows keep their relative order; the new position of a row is its rank among the live rows.
 *   nmslib_data_qty becomes the live count; nmslib_get_data_point*, nmslib_borrow_data_dense and nmslib_get_distance
 *   address the new positions.  External ids do not change.  nmslib_gpu_deleted_rows is 0 afterwards, nmslib_save_index
 *   works again, and a later nmslib_gpu_delete_ids works on the new positions.
 *   No marked row: NMSLIB_SUCCESS, *removed = *repaired = 0, nothing is launched and nothing changes.
 *   Every row marked: rows and marks go as with nmslib_reset_index, the index parameters stay; *removed = the row count.
 * hnsw with a resident graph (the index has been on the GPU; built in this process by either builder, any `post`,
 * gpu_rows=f16 included): every list of a live node that holds a deleted node keeps its live entries and is filled up to
 * its old length from the live neighbours of its deleted entries (one hop, the closest max(efConstruction, maxM0) <= 1024
 * of them, the graph's selection test); then rows, ids, norms, the fp16 copy and all lists are compacted in HBM and the
 * marks are released.  No row and no list crosses PCIe.  Searches afterwards run as on an index that never had a deleted
 * row: no filter, counts of k, and with gpu_append=1 later rows are appended.  Rows added since the last use are put into
 * the graph first, as a query would do.
 * hnsw without a resident graph (gpu_defer=1 before the first use, or no device), brute_force and seq_search: the host
 * rows, ids and marks are compacted and the index is built / prepared again at its next use: it is then the index of the
 * live rows alone.
 * The call is ordered behind the index's earlier work on whatever stream and returns when the device work is done: it is
 * a maintenance call and may block.
 * Sparse, string and divergence indexes, gpu_shards > 1, a graph loaded from a file, delaunay_type=3 and lists wider than
 * the GPU builder's (M or maxM > 127, maxM0 > 254) -> NMSLIB_ERROR_SPACE_INCOMPATIBLE, also when no row is marked: the
 * refusal is decided first, as in nmslib_gpu_delete_ids.  NULL handle -> NMSLIB_ERROR_NULL_POINTER. */
nmslib_error_t nmslib_gpu_consolidate(nmslib_index_handle_t index, size_t* removed, size_t* repaired);

/* Filtered k-NN: a search restricted to the rows a bitset allows.
 * A filter names POSITIONS (the order in which the rows were added; nmslib_data_qty of them when it is made) and is prepared
 * on the device once; any number of batches then run under it.  A filtered batch answers as the unfiltered entries do:
 * external ids, unused slots padded with -1 / +inf, counts reported; no result is a row whose bit is clear or that is deleted.
 *   nmslib_gpu_filter_create: allow_bits is host memory, one bit per position (bit p & 31 of word p >> 5, the layout of the
 *     tombstone bitset), allow_words >= ceil(nmslib_data_qty / 32); bits at or beyond the row count are ignored.  scan_rows:
 *     see "hnsw" below; 0 = default.  The call finalizes a dirty index first, as a query would, and returns when the device
 *     is done: it is a maintenance call and may block.
 *   nmslib_gpu_filter_info: rows the filter allows that are not deleted now (0 for a stale filter), and the device memory
 *     the filter holds.  That memory is reported here only: the index's hbm_bytes and nmslib_index_memory_usage do not
 *     count it.
 *   nmslib_gpu_filter_destroy: NULL is a no-op.  Filters belong to their index and are freed with it at the latest; a filter
 *     handle must not be used after nmslib_index_destroy.  Every entry runs under the index's mutex.
 * What a filter is: it stays valid as long as positions keep their meaning.  Rows added after it was made are not allowed
 * (appended with gpu_append=1 or put in by a full rebuild).  Rows deleted after it was made drop out of the results.  A
 * nmslib_gpu_consolidate that removed at least one row and nmslib_reset_index make it stale: a query with a stale filter, or
 * with a filter of another index -> NMSLIB_ERROR_INVALID_ARGUMENT, the message says which.
 * hnsw: a batch runs the search it would run anyway (whichever path: fp16 walk with its re-rank, SearchOld, the HBM-array
 *   kernel) for k' = max(efSearch, k) results and keeps the first k that are allowed and not deleted, so a count can fall
 *   below k when few of the rows the search finds are allowed -- as with deleted rows.  A filter that allows
 *   m <= max(efSearch, k, scan_rows) live rows (m counted when the filter is made; at most 4096) is answered instead by an
 *   exact scan of those rows: the f32 distances the walk returns for them, ordered by (distance, position), counts of
 *   min(k, m).  The walk evaluates at least k' distances, the scan m <= k': the rule needs no tuning; scan_rows (<= 4096)
 *   raises the bound for a caller who has measured.  A scan whose keys and query would not fit into the 160 KB of LDS of a
 *   workgroup (4096 rows of more than 32 252 dimensions) is left to the walk.  The scan reports ndc = m, hops = hops_up = 0 through
 *   nmslib_gpu_last_batch_counters, and last_path 7.
 *   With the query-time parameter gpu_inwalk=1 (see nmslib_gpu_delete_ids) a batch that would walk tests the filter and the
 *   tombstones inside the walk instead: rows that are not allowed are stepping stones and do not count against efSearch, the
 *   results are the walk's max(efSearch, k) closest allowed live rows cut to k, ordered by (distance, position), and
 *   last_path is 8.  The exact scan keeps precedence where the rule above chooses it.  Selective filters then return k
 *   results at the price of a longer walk (DESIGN.md 6 has the measurements); the choice is the caller's switch.
 * brute_force / seq_search: the filter is the index of the allowed live rows alone, gathered and prepared in HBM (no row
 *   crosses PCIe); a batch takes every path such an index would take.  When the index has been prepared again since (rows
 *   added or deleted), the next filtered batch gathers and prepares again before it runs and may block; every other batch
 *   only enqueues.
 * The device entry keeps the contract of nmslib_gpu_knn_query_batch_device (alignment, order across streams, d_counts may be
 * NULL); the host entry takes host pointers: ids / dists [query_count][k], counts [query_count] (may be NULL).
 * Served: hnsw, brute_force and seq_search over l2, l1, linf, cosinesimil, angulardist, negdotprod and l2sqr_sift on one
 * device.  Sparse, string and divergence indexes and gpu_shards > 1 -> NMSLIB_ERROR_SPACE_INCOMPATIBLE at create, decided
 * before a device is needed; an exact-scan index that automatic sharding has spread over several devices -> the same code,
 * at create and for a batch under a filter made before.  A NULL index, out, or allow_bits with rows present -> NMSLIB_ERROR_NULL_POINTER; too few words,
 * or scan_rows > 4096 -> NMSLIB_ERROR_INVALID_ARGUMENT; no device -> NMSLIB_ERROR_RUNTIME. */
typedef struct nmslib_gpu_filter* nmslib_gpu_filter_t;
nmslib_error_t nmslib_gpu_filter_create(nmslib_index_handle_t index, const uint32_t* allow_bits, size_t allow_words,
                                        size_t scan_rows, nmslib_gpu_filter_t* out);
void nmslib_gpu_filter_destroy(nmslib_gpu_filter_t f);
nmslib_error_t nmslib_gpu_filter_info(nmslib_gpu_filter_t f, size_t* allowed_live_rows, size_t* hbm_bytes);
nmslib_error_t nmslib_gpu_knn_query_batch_filtered(nmslib_index_handle_t index, nmslib_gpu_filter_t f, const void* queries,
                                                   size_t query_count, size_t elem_count, size_t k, int32_t* ids,
                                                   float* dists, int32_t* counts);
nmslib_error_t nmslib_gpu_knn_query_batch_filtered_device(nmslib_index_handle_t index, nmslib_gpu_filter_t f,
                                                          const void* d_queries, size_t query_count, size_t elem_count,
                                                          size_t k, int32_t* d_ids, float* d_dists, int32_t* d_counts,
                                                          void* stream);

/* One filter per query: a batch whose queries belong to different filters
 * of the same index -- tenants, categories, access lists -- in one call.  filter_of_query[q] is an index into filters
 * [n_filters], or -1 = query q is unfiltered; the same filter may stand at several indices.  Row q of the results is what
 * nmslib_gpu_knn_query_batch_filtered returns for query q under its filter (the unfiltered entries for -1), bit for bit, and
 * on hnsw nmslib_gpu_last_batch_counters describes the batch in the caller's order.
 *   filters and filter_of_query are host memory in both entries and are read before the call returns: the caller may free
 *   them at once.  The device entry otherwise keeps the contract of nmslib_gpu_knn_query_batch_filtered_device (it only
 *   enqueues; d_counts may be NULL); the host entry takes host pointers, counts may be NULL.
 *   routes (host, [query_count], optional): per query the last_path the single-filter entry reports for the batch formed by
 *   the queries of its filter -- hnsw: 4, 5, 7 or 8; exact scan: the path over the allowed rows; -1 queries: the unfiltered
 *   entry's.  The routing is host arithmetic: every value is there when the call returns, in both entries.  last_path is 9
 *   afterwards; the fast_tiles* and hnsw_redone statistics describe the part of the batch that ran last.
 * hnsw: the batch is run in plan order -- unfiltered queries, then those of the filters that walk, then those of the filters
 *   that are scanned exactly -- and costs one launch chain per such segment, whatever the number of filters: the kernels read
 *   each query's filter from a table that is uploaded with the batch.  A batch that is not in that order already is gathered
 *   into a workspace and its results gathered back (five small launches more).
 * brute_force / seq_search: one exact scan per filter that has queries, over that filter's queries, on the index of its
 *   allowed rows: the launch count grows with the number of distinct filters in the batch, and groups of fewer than 256
 *   queries stay off the fast paths.  A filter whose index was prepared again gathers again first (may block).
 * Checked before any device work: a NULL index, filter_of_query, queries or output, or filters with n_filters > 0 ->
 * NMSLIB_ERROR_NULL_POINTER; an entry of filter_of_query outside [-1, n_filters) -> NMSLIB_ERROR_INVALID_ARGUMENT (the
 * message names the query and the value); a stale filter or one of another index -> NMSLIB_ERROR_INVALID_ARGUMENT (the
 * message names its index in filters); the index kinds nmslib_gpu_filter_create refuses -> its refusal.  query_count == 0 ->
 * NMSLIB_SUCCESS, nothing is written.  On an error the outputs are untouched. */
nmslib_error_t nmslib_gpu_knn_query_batch_filtered_each(nmslib_index_handle_t index, const nmslib_gpu_filter_t* filters,
                                                        size_t n_filters, const int32_t* filter_of_query, const void* queries,
                                                        size_t query_count, size_t elem_count, size_t k, int32_t* ids,
                                                        float* dists, int32_t* counts, int32_t* routes);
nmslib_error_t nmslib_gpu_knn_query_batch_filtered_each_device(nmslib_index_handle_t index, const nmslib_gpu_filter_t* filters,
                                                               size_t n_filters, const int32_t* filter_of_query,
                                                               const void* d_queries, size_t query_count, size_t elem_count,
                                                               size_t k, int32_t* d_ids, float* d_dists, int32_t* d_counts,
                                                               int32_t* routes, void* stream);

/* Batched range queries on the exact scan: query_count range queries,
 * each with its own radius, in one call; the rows are read once per slice of the batch instead of once per query.
 * Row q of the results is, bit for bit, what nmslib_range_query_fill writes for query q with radii[q] into a result of
 * `capacity` entries: the first `capacity` rows with distance <= radius in insertion (position) order, external ids and the
 * reference formula's distance.  The radius is converted as that entry converts it ((float)radius; l2sqr_sift:
 * (float)(int)radius), so a negative or NaN radius matches here what it matches there.
 *   ids / dists : [query_count][capacity]; entries beyond counts[q] are -1 / +inf, as in nmslib_gpu_knn_query_batch_device
 *   counts      : [query_count], entries written = min(totals[q], capacity); may be NULL
 *   totals      : [query_count], every row within the radius, no cap; may be NULL unless capacity == 0
 *   capacity    : per query; 0 = count only, ids and dists may then be NULL
 *   radii       : [query_count] HOST memory in both entries, read before the call returns
 * Served: brute_force and seq_search over l2, l1, linf, cosinesimil, angulardist, negdotprod and l2sqr_sift.  Deleted rows
 * do not appear; after nmslib_gpu_consolidate the answers are on the new positions.  The host entry also serves a sharded
 * exact-scan index: the shards are asked in order, per query their lists are put back to back up to `capacity` and the
 * totals are summed, which is the unsharded answer bit for bit; the device entry on a sharded index ->
 * NMSLIB_ERROR_SPACE_INCOMPATIBLE.
 * The device entry keeps the contract of nmslib_gpu_knn_query_batch_device (alignment of the element type only, order across
 * streams, the stream's lifetime).  It only enqueues work; its workspaces are sized before the first kernel.  The radii
 * cross through two pinned blocks taken in turn: a call waits on the host only if the radii copy of the call before the
 * previous one has not run yet.
 * last_path afterwards: 10 = the batched kernels; 11 = the single-query launches, once per query, into the batch's rows
 * (float rows of more than 256 dimensions, or a workspace bound below one query's masks).  The bound of the mask workspace
 * is 256 MiB; the environment switch NMSLIB_GPU_RANGE_WS_BYTES, read per call, lowers it.
 * Checked before a device is needed, and on an error the outputs are untouched: a NULL index, queries or radii, or ids / dists
 * NULL with capacity > 0 -> NMSLIB_ERROR_NULL_POINTER; capacity == 0 with totals == NULL -> NMSLIB_ERROR_INVALID_ARGUMENT; an
 * index that was never built -> NMSLIB_ERROR_INDEX_BUILD_FAILED; hnsw -> NMSLIB_ERROR_SPACE_INCOMPATIBLE with the message of
 * nmslib_range_query_fill; sparse, string and divergence indexes -> NMSLIB_ERROR_SPACE_INCOMPATIBLE, the message names what
 * is served; a query length other than the index's -> NMSLIB_ERROR_INVALID_ARGUMENT; query_count == 0 -> NMSLIB_SUCCESS,
 * nothing is written. */
nmslib_error_t nmslib_gpu_range_query_batch(nmslib_index_handle_t index, const void* queries, size_t query_count,
                                            size_t elem_count, const double* radii, size_t capacity, int32_t* ids,
                                            float* dists, int32_t* counts, int32_t* totals);
nmslib_error_t nmslib_gpu_range_query_batch_device(nmslib_index_handle_t index, const void* d_queries, size_t query_count,
                                                   size_t elem_count, const double* radii, size_t capacity, int32_t* d_ids,
                                                   float* d_dists, int32_t* d_counts, int32_t* d_totals, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NMSLIB_GPU_H */
