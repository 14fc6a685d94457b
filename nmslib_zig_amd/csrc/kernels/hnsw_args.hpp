// Kernel arguments shared by the HNSW search kernels (hnsw_kernels.hip, hnsw_mw_kernels.hip, hnsw_q8_kernels.hip) and the
// host functions that fill them.
#pragma once
#include <cstdlib>

#include "common_dev.hpp"
#include "kernels.hpp"

namespace gfxknn {

struct HnswArgs {
    HnswDeviceGraph g;
    const void* queries;
    uint32_t* bitset;
    size_t bitset_words;
    int32_t* out_ids;
    float* out_dists;
    int32_t* out_cnt;
    int32_t* out_ndc;
    int32_t* out_hops;
    int32_t* out_hops_up;
    int32_t* status;
    int nq, k, ef, cap;
    int nbcap;  // SearchOld / HBM-array SearchV1Merge with wide lists: entries of the frontier arrays (hnsw_nbcap)
    int capa;  // cap rounded up to a multiple of 4 (keeps the LDS carve-up 16-byte aligned)
    // construction mode (hnsw_build_kernels.hip): the query is a stored row, the best-first phase runs
    // on `level`, and the start node is given (or found by descending from the entry point to level+1)
    const int32_t* query_rows;   // [nq] row index of each query, or NULL (external queries)
    const int32_t* start_nodes;  // [nq] start node (>= 0) or -1 = descend from the entry point; or NULL
    int level;
    int table_size, table_shift;
    int prof;  // NMSLIB_HNSW_PROF: accumulate per-phase cycles into g_hnsw_prof (experiments only)
    // visited-table overflow without the host: the LDS-table launch appends overflowed queries to fix_list; the
    // bitset launch that follows (fix_mode) walks that list, each workgroup with its own bitset slot
    int32_t* fix_list;
    int32_t* fix_count;
    int fix_mode;
    int no_pipe;  // NMSLIB_HNSW_PIPE=0: the one-wave kernel without its software pipeline (diagnostics)
};

constexpr uint32_t HT_EMPTY = 0xFFFFFFFFu;  // free slot of the LDS visited table

// What every search kernel reads: the graph, the queries, the visited bitset and where the results go.  Each launch entry
// adds what is its own (LDS carve-up, visited table, overflow list, diagnostics).
inline HnswArgs hnsw_args(const HnswDeviceGraph& g, int nq, int k, int ef, int cap, const HnswQueries& q, uint32_t* bitset,
                          size_t bitset_words, const HnswOut& out) {
    HnswArgs a{};
    a.g = g;
    a.nbcap = hnsw_nbcap(g);
    a.queries = q.queries;
    a.query_rows = q.query_rows;
    a.start_nodes = q.start_nodes;
    a.level = q.level;
    a.bitset = bitset;
    a.bitset_words = bitset_words;
    a.out_ids = out.ids;
    a.out_dists = out.dists;
    a.out_cnt = out.cnt;
    a.out_ndc = out.ndc;
    a.out_hops = out.hops;
    a.out_hops_up = out.hops_up;
    a.status = out.status;
    a.nq = nq;
    a.k = k;
    a.ef = ef;
    a.cap = cap;
    return a;
}

// The arguments of the one-wave SearchV1Merge kernels (hnsw_walk_dev.hpp) under plan p: hnsw_args and what the plan
// decides -- the LDS carve-up, the visited table, the overflow route and the pipeline's switch.
// (NMSLIB_HNSW_PIPE is read per launch: the tests switch it inside one process)
inline HnswArgs hnsw_walk_args(const HnswDeviceGraph& g, const HnswSearchPlan& p, const HnswQueries& q, uint32_t* bitset,
                               const HnswOverflow& fix, const HnswOut& out) {
    HnswArgs a = hnsw_args(g, p.nq, p.k, p.ef, p.cap, q, bitset, p.bitset_words, out);
    a.capa = (p.cap + 3) & ~3;
    a.table_size = p.table_size;
    a.table_shift = p.table_shift;
    a.fix_list = fix.fix_list;
    a.fix_count = fix.fix_count;
    a.fix_mode = (p.table_size == 0) ? fix.fix_slots : 0;
    const char* pipe = getenv("NMSLIB_HNSW_PIPE");
    a.no_pipe = pipe ? atoi(pipe) == 0 : 0;
    return a;
}

// hnsw_mw_kernels.hip: one workgroup per query (control wave + gather waves); sa_emax = sorted-array items per lane
// (2 or 4); rows_f16: the gather reads g.rows16.  Same results, bit for bit, as hnsw_search_kernel<SPACE, false, sa_emax,
// false, ROW> over the same rows.
hipError_t launch_hnsw_search_mw(const HnswArgs& a, size_t lds_bytes, int sa_emax, bool rows_f16, hipStream_t s);
// control-wave phase cycles accumulated since the last call (NMSLIB_HNSW_PROF), then cleared
void hnsw_mw_read_prof(unsigned long long out[12]);

}  // namespace gfxknn
