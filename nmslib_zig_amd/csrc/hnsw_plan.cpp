// Search plans of the HNSW kernels (kernels/hnsw_kernels.hip): how much LDS a query's workgroup takes and where its
// visited set and queues live.  Host only.
#include "kernels/kernels.hpp"

namespace gfxknn {

static int ilog2(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

static HnswSearchPlan plan_base(int nq, int k, int ef) {
    HnswSearchPlan p{};
    p.nq = nq;
    p.k = k;
    p.ef = ef;
    p.cap = ef > k ? ef : k;
    return p;
}

// The visited set of a kernel whose other LDS needs are `fixed` bytes: an exact hash table in LDS, or a per-query bitset
// in HBM.  Expected visited nodes ~ (maxM0 * expansions), expansions ~ ef: the table is sized for 2x that, halved while
// it does not fit `budget`.
static void plan_visited(HnswSearchPlan& p, const HnswDeviceGraph& g, size_t fixed, size_t budget, bool force_bitset) {
    int want = 1 << ilog2((g.maxM0 > 0 ? g.maxM0 : 32) * p.cap * 2);
    if (want < 2048) want = 2048;
    while ((size_t)want * 4 + fixed > budget && want > 2048) want >>= 1;
    // ~18 distance evaluations per unit of ef on 1M-row graphs: beyond half load
    // the exact hash set is replaced by a per-query bitset in HBM
    if (force_bitset || 18 * p.cap > want / 2 || (size_t)want * 4 + fixed > 64 * 1024) {
        p.table_size = 0;
        p.table_shift = 0;
        p.bitset_words = ((size_t)g.n + 31) / 32;
        p.lds_bytes = fixed + 16;
    } else {
        p.table_size = want;
        p.table_shift = 32 - ilog2(want);
        p.bitset_words = 0;
        p.lds_bytes = fixed + (size_t)want * 4;
    }
}

HnswSearchPlan hnsw_make_plan(const HnswDeviceGraph& g, int nq, int k, int ef, bool force_bitset) {
    HnswSearchPlan p = plan_base(nq, k, ef);
    const bool u8 = g.space == SP_L2SQR_SIFT;
    const size_t fixed = (size_t)((p.cap + 3) & ~3) * 8 + (u8 ? 128 : (size_t)g.ldv * 4) + (size_t)(2 * hnsw_nbcap(g) + 2 * 64) * 4;
    // never let LDS push residency below 4 waves per CU (160 KB / 4)
    plan_visited(p, g, fixed, 40 * 1024 - 64, force_bitset);
    return p;
}

HnswSearchPlan hnsw_make_plan_old(const HnswDeviceGraph& g, int nq, int k, int ef, bool force_bitset, int heap_cap) {
    HnswSearchPlan p = plan_base(nq, k, ef);
    const bool u8 = g.space == SP_L2SQR_SIFT;
    p.a_in_lds = ef <= 8192;
    p.r_in_lds = k <= 2048;
    // accepted items are a fraction of the evaluated ones (~18 per unit of ef on 1M-row graphs)
    long long hc = heap_cap > 0 ? heap_cap : 32ll * p.cap + 4096;
    if (hc > (long long)g.n + 1) hc = (long long)g.n + 1;
    p.heap_cap = (int)hc;
    p.heap_lds = p.heap_cap < 2048 ? p.heap_cap : 2048;
    const size_t fixed = (u8 ? 128 : (size_t)g.ldv * 4) + (size_t)(2 * hnsw_nbcap(g) + 64) * 4 + (size_t)p.heap_lds * 8 +
                         (p.a_in_lds ? (size_t)((ef + 1) & ~1) * 4 : 0) + (p.r_in_lds ? (size_t)k * 8 : 0);
    plan_visited(p, g, fixed, 64 * 1024, force_bitset);
    return p;
}

}  // namespace gfxknn
