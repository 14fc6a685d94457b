// The one-wave HNSW search, once: SearchV1Merge over whatever form of the rows a policy gathers.
//
// Restates Hnsw::SearchV1Merge (src/method/hnsw_distfunc_opt.cc:152-283) and its generic twin
// baseSearchAlgorithmV1Merge (src/method/hnsw.cc:1174-1300) step for step:
//   1. greedy descent through the upper levels (:173-198);
//   2. level-0 best-first over a bounded sorted array (SortArrBI, include/sort_arr_bi.h) of
//      max(ef, k) items: expand the first unused item, evaluate its unvisited neighbours,
//      keep those with d < topKey (or while fewer than ef items), insert them in ascending
//      order with SortArrBI::push_or_replace_non_empty_exp semantics (:159-199);
//   3. emit the first k items (:276-281) through KNNQueue ordering (knnqueue.h:55-64).
// Included by hnsw_kernels.hip (f32 / u8 rows and the fp16 copy: hnsw_search_kernel) and by hnsw_q8_kernels.hip (the 8-bit
// copy: hnsw_search_q8_kernel).  Each file instantiates the body for its own kernels in its own object, under its own
// compiler flags; nothing here depends on either flag set.
//
// A policy P says what differs between the forms of the rows and nothing else:
//   P::Loads                         the loads of one expansion in flight (FrontierLoads / Q8Loads)
//   P::slot_floats(g)                floats of LDS the staged query takes
//   p.stage(a, q, slot, lane)        puts query q into its LDS slot and keeps the scalars that go with it
//   p.distances(g, nbr, nd, m, lane) keys of the rows nbr[0..m) -> nd[0..m)
//   p.issue(L, g, nbr, m, lane)      the same, split: request the first loads of the first 32 rows ...
//   p.finish(L, g, nbr, nd, m, lane) ... consume them, fetch the rest, write nd[0..m)
//   P::kBuild   construction mode: a.query_rows, a.start_nodes and a.level are honoured (else: external queries, level 0)
//   P::kProf    the phase clocks (a.prof) are compiled in; P::prof_flush(pc) adds a query's cycles to the file's counters
//   P::kRaw     the result is the sorted array as it stands: array order, internal positions (for hnsw_rerank_kernel)
//   P::kPad     unused output slots, and the result over an empty index, are filled with -1 / +inf
// All four are compile-time constants: a form without construction mode has no a.level branch in its adjacency loads.
#pragma once
#include "hnsw_args.hpp"
#include "hnsw_common_dev.hpp"

namespace gfxknn {

// EMAX = sorted-array items per lane (cap <= 64*EMAX): 2 for ef <= 128, 4 for <= 256, 16 otherwise.
// WIDE: level-0 lists of more than 62 neighbours (maxM0 up to 126, i.e. M >= 32): second adjacency chunk,
// 128-entry neighbour staging, two insertion rounds.  Kept out of the common instantiation.
// (the chunked list walk of SearchOld and the HBM-array kernel: collect_unvisited_any, greedy_step_any in hnsw_common_dev.hpp)
template <class P, bool BITSET, int SA_EMAX, bool WIDE>
__device__ __forceinline__ void hnsw_walk_body(const HnswArgs& a, char* smem, const int q, uint32_t* const bits) {
    const HnswDeviceGraph& g = a.g;
    const int lane = threadIdx.x;

    // ---- LDS carve-up as hnsw_make_plan sizes it (all offsets multiples of 16 bytes) ----
    float* keys = reinterpret_cast<float*>(smem);                  // [capa]
    int* idu = reinterpret_cast<int*>(keys + a.capa);              // [capa]  id | used<<31
    float* slot = reinterpret_cast<float*>(idu + a.capa);          // the query (f32: [ldv]; u8: 128 bytes; 8-bit: its codes)
    const int nbcap = WIDE ? a.nbcap : 64;                         // neighbours of one expansion (wide lists: a multiple of 64 >= maxM0, maxM)
    int* nbr = reinterpret_cast<int*>(slot + P::slot_floats(g));   // [nbcap]
    float* nd = reinterpret_cast<float*>(nbr + nbcap);             // [nbcap]
    float* sk = nd + nbcap;                                        // [64] accepted keys, sorted
    int* si = reinterpret_cast<int*>(sk + 64);                     // [64] accepted ids
    uint32_t* table = reinterpret_cast<uint32_t*>(si + 64);        // [table_size]

    P row;
    row.stage(a, q, slot, lane);
    if constexpr (!BITSET) {
        for (int i = lane; i < a.table_size; i += 64) table[i] = HT_EMPTY;
    }
    __builtin_amdgcn_wave_barrier();
    // visited test-and-set: true when id was NOT visited before (exact)
    // (VisitedSet of hnsw_common_dev.hpp, written out: with the table's size and shift copied into that struct the probe
    //  loop below came out in another shape, and the fp16 walk measured 0.4 - 0.6 % slower than before)
    auto visit = [&](uint32_t id) -> bool {
        if constexpr (BITSET) {
            const uint32_t bit = 1u << (id & 31);
            const uint32_t old = atomicOr(&bits[id >> 5], bit);
            return (old & bit) == 0;
        } else {
            uint32_t hsh = (id * 2654435761u) >> a.table_shift;
            const uint32_t mask = (uint32_t)a.table_size - 1u;
            for (int probe = 0; probe < a.table_size; ++probe) {
                const uint32_t old = atomicCAS(&table[hsh], HT_EMPTY, id);
                if (old == HT_EMPTY) return true;
                if (old == id) return false;
                hsh = (hsh + 1) & mask;
            }
            return false;
        }
    };

    int ndc = 0, hops = 0, hops_up = 0, nvisited = 0;
    bool overflow = false;

    if (g.n == 0) {
        hnsw_empty_result<P::kPad>(a, q, lane);
        return;
    }

    // ---- entry point + greedy descent (hnsw_distfunc_opt.cc:168-198) ----
    // construction mode: a given start node, or the descent stops above a.level
    int start = -1, level = 0;
    if constexpr (P::kBuild) {
        start = a.start_nodes ? a.start_nodes[q] : -1;
        level = a.level;
    }
    // (greedy_descent of hnsw_common_dev.hpp, written out: the walk's code stays the one it had before the body was shared)
    int cur = start >= 0 ? start : g.enterpoint;
    if (lane == 0) nbr[0] = cur;
    __builtin_amdgcn_wave_barrier();
    row.distances(g, nbr, nd, 1, lane);
    float curdist = nd[0];
    ndc += 1;
    for (int lvl = (start >= 0 ? 0 : g.maxlevel); lvl > level; --lvl) {
        bool changed = true;
        while (changed) {
            changed = false;
            const int64_t off = g.up_off[cur] + (int64_t)(lvl - 1) * (g.maxM + 1);
            if (WIDE && g.maxM > 62) {   // upper-level lists longer than one word per lane
                hops_up++;
                ndc += greedy_step_any(g.up_links + off, nbr, nd, lane, cur, curdist, changed,
                                       [&](const int* ids, float* out, int m)
                                           __attribute__((always_inline)) { row.distances(g, ids, out, m, lane); });
                continue;
            }
            const int v = (lane <= g.maxM) ? g.up_links[off + lane] : 0;
            const int cntl = __builtin_amdgcn_readfirstlane(v);
            const int nb = __shfl(v, lane + 1, 64);
            if (lane < cntl) nbr[lane] = nb;
            __builtin_amdgcn_wave_barrier();
            hops_up++;
            if (cntl > 0) {
                row.distances(g, nbr, nd, cntl, lane);
                ndc += cntl;
                // sequential "if (d < curdist)" scan == first index attaining the minimum
                u64 key = ~0ull;
                if (lane < cntl) key = ((u64)f32_ord(nd[lane]) << 32) | (uint32_t)lane;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const u64 other = __shfl_xor(key, o, 64);
                    key = other < key ? other : key;
                }
                const float dmin = ord_f32((uint32_t)(key >> 32));
                if (dmin < curdist) {
                    curdist = dmin;
                    cur = nbr[(uint32_t)key];
                    changed = true;
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }

    // ---- level 0 (hnsw_distfunc_opt.cc:200-274) ----
    int n = 1;
    if (lane == 0) {
        keys[0] = curdist;
        idu[0] = cur;
    }
    // (the f32 copy visited the entry node in a statement of its own, the 8-bit copy inside the block above: the same
    //  effect, one lane and one test-and-set; this is the f32 copy's form for both)
    if (lane == 0) (void)visit((uint32_t)cur);
    nvisited = 1;
    __builtin_amdgcn_wave_barrier();

    // cursor: every item before it is used (the reference's currElem).  pre_*: adjacency of the item
    // that will most likely be expanded next, requested one expansion early (its latency hides
    // behind this expansion's gather); a wrong guess only costs the normal load.
    // adjacency word `lane` of node c on the level being searched ([count][ids...])
    auto load_adj = [&](int c) -> int {
        if (!P::kBuild || a.level == 0) return (lane <= g.maxM0) ? g.links0[(size_t)c * (g.maxM0 + 1) + lane] : 0;
        return (lane <= g.maxM) ? g.up_links[g.up_off[c] + (int64_t)(a.level - 1) * (g.maxM + 1) + lane] : 0;
    };
    int cursor = 0;
    int pre_node = -1, pre_v = 0, pre2_node = -1, pre2_v = 0;
    float pre_key = INFINITY;
    bool pre_ok = false;            // pre_node is the first unused item of the array, at a position below ef
    // Software pipeline across expansions: when the NEXT node to expand is already certain before the accepted items of
    // this expansion are merged in (it is the array's next unused item and every accepted key is larger), its visited
    // filter runs and its row gather is issued first, and the merge executes while those rows are in flight.
    int pipe_node = -1, pipe_m = 0;
    typename P::Loads fl;
    long long pc[6] = {0, 0, 0, 0, 0, 0};
    long long pt = 0;
    if constexpr (P::kProf) pt = a.prof ? (long long)__builtin_readcyclecounter() : 0;
    auto lap = [&](int ph) __attribute__((always_inline)) {
        if constexpr (P::kProf) {
            if (a.prof) {
                const long long now = (long long)__builtin_readcyclecounter();
                pc[ph] += now - pt;
                pt = now;
            }
        }
    };
    lap(0);
    while (true) {
        const int lim = n < a.ef ? n : a.ef;
        // first unused item at or after cursor
        int fu = n;
        for (int base = cursor; base < n && fu == n; base += 64) {
            const int i = base + lane;
            const u64 mk = __ballot(i < n && idu[i] >= 0);
            if (mk) fu = base + (__ffsll((long long)mk) - 1);
        }
        if (fu >= lim) break;
        const int c = idu[fu] & 0x7FFFFFFF;
        if (lane == 0) idu[fu] |= (int)0x80000000;
        cursor = fu + 1;
        hops++;
        const float topKey = keys[n - 1];
        const int size0 = n;

        int m;
        if (c == pipe_node) {
            // visited filter done and rows requested during the previous expansion; the guess for the expansion after
            // this one was made there too
            m = pipe_m;
            pipe_node = -1;
            lap(1);
            lap(2);
        } else {
            // adjacency of c: [count][ids...]
            int v;
            if (c == pre_node) v = pre_v;
            else if (c == pre2_node) v = pre2_v;
            else v = load_adj(c);
            // Adjacency of the NEXT expansion, requested early so that its latency (a random HBM read under
            // load: ~2 us) hides behind this expansion's gather and inserts.  Two guesses: (A) now, the next
            // unused item of the array -- right unless this expansion finds something closer; (B) after the
            // distances, the best newly accepted item when it is closer than (A).
            const int cntn = __builtin_amdgcn_readfirstlane(v);
            lap(1);
            const int nb = __shfl(v, lane + 1, 64);   // neighbours 0..62 (list words 1..63)
            bool isn = false;
            if (lane < cntn && (!WIDE || lane < 63)) isn = visit((uint32_t)nb);
            const u64 nmask = __ballot(isn);
            m = __popcll(nmask);
            if (isn) nbr[__popcll(nmask & ((1ull << lane) - 1ull))] = nb;
            if (WIDE) {
                // wide level-0 lists (maxM0 > 62, i.e. M >= 32): neighbours 63.. are list words 64.., read on demand in chunks
                // of 64 (round 3: any number of chunks the frontier arrays hold -- a.nbcap)
                // (construction mode above level 0, maxM > 62: the same walk over the node's list on that level)
                const bool l0 = !P::kBuild || a.level == 0;
                const int32_t* Lc = l0 ? g.links0 + (size_t)c * (g.maxM0 + 1)
                                       : g.up_links + g.up_off[c] + (int64_t)(a.level - 1) * (g.maxM + 1);
                const int Lmax = l0 ? g.maxM0 : g.maxM;
                for (int c0 = 63; c0 < cntn; c0 += 64) {
                    int nb2 = 0;
                    if (c0 + 1 + lane <= Lmax) nb2 = Lc[c0 + 1 + lane];
                    bool isn2 = false;
                    if (c0 + lane < cntn) isn2 = visit((uint32_t)nb2);
                    const u64 nmask2 = __ballot(isn2);
                    if (isn2) nbr[m + __popcll(nmask2 & ((1ull << lane) - 1ull))] = nb2;
                    m += __popcll(nmask2);
                }
            }
            nvisited += m;
            if (!BITSET && nvisited > (a.table_size - (a.table_size >> 3))) {
                overflow = true;  // visited table nearly full: give up, the bitset variant re-runs the query
                break;
            }
            __builtin_amdgcn_wave_barrier();
            lap(2);
            // (issued only now: v had to be waited for first, and vmcnt retires in order -- a younger
            //  outstanding load in front of that wait would put its whole latency into it)
            {
                int fu2 = n;
                for (int base = cursor; base < n && fu2 == n; base += 64) {
                    const int i = base + lane;
                    const u64 mk = __ballot(i < n && idu[i] >= 0);
                    if (mk) fu2 = base + (__ffsll((long long)mk) - 1);
                }
                if (fu2 < lim) {
                    pre_node = idu[fu2] & 0x7FFFFFFF;
                    pre_key = keys[fu2];
                    pre_v = load_adj(pre_node);
                    pre_ok = true;
                } else {
                    pre_node = -1;
                    pre_key = INFINITY;
                    pre_ok = false;
                }
                pre2_node = -1;
            }
            if (m > 0) row.issue(fl, g, nbr, m, lane);
        }
        if (m == 0) continue;
        ndc += m;
        row.finish(fl, g, nbr, nd, m, lane);
        lap(3);

        // (more than 64 new rows only with wide lists: rounds of 64; without equal keys the final array does
        //  not depend on the order in which accepted items are merged in)
        for (int r0 = 0; r0 < (WIDE ? m : 1); r0 += 64) {  // one trip unless the lists are wide
            // accept d < topKey || size < ef   (:240)
            float dj = INFINITY;
            int idj = -1;
            bool acc = false;
            if (r0 + lane < m) {
                dj = nd[r0 + lane];
                idj = nbr[r0 + lane];
                acc = (dj < topKey) || (size0 < a.ef);
            }
            const u64 amask = __ballot(acc);
            const int m2 = __popcll(amask);
            if (m2 == 0) continue;
            // ascending order of the accepted items (std::sort, :251); ties keep list order
            int rank = 0;
            for (u64 mm = amask; mm;) {
                const int j = __ffsll((long long)mm) - 1;
                mm &= mm - 1;
                // (j comes from the ballot mask, so it is wave-uniform: v_readlane, not an LDS-routed shuffle)
                const float dother = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(dj), j));
                rank += (dother < dj || (dother == dj && j < lane)) ? 1 : 0;
            }
            __builtin_amdgcn_wave_barrier();
            if (acc) {
                sk[rank] = dj;
                si[rank] = idj;
            }
            __builtin_amdgcn_wave_barrier();

            if (sk[0] <= pre_key) {  // guess (B)
                pre2_node = si[0];
                pre2_v = load_adj(pre2_node);
            } else if (!WIDE && pre_ok && !a.no_pipe) {
                // Every accepted key is larger than the key of the array's next unused item: that item (pre_node,
                // adjacency already here) IS the next expansion, whatever the merge below does to the positions
                // behind it.  Run its visited filter now and request its rows; the merge overlaps the gather.
                const int cntp = __builtin_amdgcn_readfirstlane(pre_v);
                const int nbp = __shfl(pre_v, lane + 1, 64);
                bool isp = false;
                if (lane < cntp) isp = visit((uint32_t)nbp);
                const u64 pmask = __ballot(isp);
                const int mp = __popcll(pmask);
                __builtin_amdgcn_wave_barrier();  // (nbr/nd of this expansion were consumed into registers above)
                if (isp) nbr[__popcll(pmask & ((1ull << lane) - 1ull))] = nbp;
                nvisited += mp;
                if (!BITSET && nvisited > (a.table_size - (a.table_size >> 3))) {
                    overflow = true;
                    break;
                }
                __builtin_amdgcn_wave_barrier();
                pipe_node = pre_node;
                pipe_m = mp;
                // guess for the expansion after that: the second unused item of the array, or the best accepted
                // key if that is closer (then its position is only known after the merge: no pipelining on it)
                int second = n;
                {
                    int seen = 0;
                    for (int base = cursor; base < n && second == n; base += 64) {
                        const int i = base + lane;
                        u64 mk = __ballot(i < n && idu[i] >= 0);
                        if (seen == 0 && mk) {
                            mk &= mk - 1;
                            seen = 1;
                        }
                        if (mk) second = base + (__ffsll((long long)mk) - 1);
                    }
                }
                const float k2 = second < n ? keys[second] : INFINITY;
                if (second < n && second < a.ef && k2 < sk[0]) {
                    pre_node = idu[second] & 0x7FFFFFFF;
                    pre_key = k2;
                    pre_ok = true;
                    pre_v = load_adj(pre_node);
                } else if (sk[0] < k2) {
                    pre_node = si[0];
                    pre_key = sk[0];
                    pre_ok = false;
                    pre_v = load_adj(pre_node);
                } else {
                    pre_node = -1;
                    pre_key = INFINITY;
                    pre_ok = false;
                }
                pre2_node = -1;
                if (mp > 0) row.issue(fl, g, nbr, mp, lane);
            }
            lap(4);
            // All accepted items at once when no two keys involved are equal (the normal case with f32 keys): the result
            // of the reference's sequential push_or_replace_non_empty_exp calls is then the merge of the two sorted
            // sequences cut at the capacity, so every old item moves up by the number of new keys below it and
            // new item t lands at (#old keys below it) + t; the scan cursor rewinds to the first new position
            // (hnsw_distfunc_opt.cc:261-266).  Equal keys (rare with f32 keys, the rule with the 8-bit form's integer
            // keys) take the exact sequential replay below.
            bool tie = false;
            float kreg[SA_EMAX];
            int cntv[SA_EMAX];
#pragma unroll
            for (int e = 0; e < SA_EMAX; ++e) {
                const int i = lane + 64 * e;
                kreg[e] = (e * 64 < n && i < n) ? keys[i] : INFINITY;
                cntv[e] = 0;
            }
            const float mykey = lane < m2 ? sk[lane] : INFINITY;
            const int myid = lane < m2 ? si[lane] : -1;
            int myless = 0;
            for (int t = 0; t < m2; ++t) {
                const float skt = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mykey), t));
                int less = 0;
#pragma unroll
                for (int e = 0; e < SA_EMAX; ++e) {
                    if (e * 64 < n) {
                        less += __popcll(__ballot(kreg[e] < skt));
                        cntv[e] += (skt < kreg[e]) ? 1 : 0;
                        tie |= (skt == kreg[e]);
                    }
                }
                if (lane == t) myless = less;
            }
            // (the shuffle runs in ALL lanes: under the short-circuit `&&` it sat in a divergent branch, lane m2-2 read
            //  its inactive neighbour as 0 and a tie between the two largest accepted keys went unnoticed -- found in
            //  round 3 by tests/test_gpu_hnsw_mw.py against the oracle)
            const float next_key = __shfl_down(mykey, 1, 64);
            tie |= (lane + 1 < m2) & (mykey == next_key);
            if (!__any(tie)) {
                int ireg[SA_EMAX];
#pragma unroll
                for (int e = 0; e < SA_EMAX; ++e) {
                    const int i = lane + 64 * e;
                    ireg[e] = (e * 64 < n && i < n) ? idu[i] : 0;
                }
                const int newn = n + m2 < a.cap ? n + m2 : a.cap;
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int e = 0; e < SA_EMAX; ++e) {
                    const int i = lane + 64 * e;
                    if (e * 64 < n && i < n && cntv[e] > 0) {
                        const int np = i + cntv[e];
                        if (np < newn) {
                            keys[np] = kreg[e];
                            idu[np] = ireg[e];
                        }
                    }
                }
                if (lane < m2) {
                    const int np = myless + lane;
                    if (np < newn) {
                        keys[np] = mykey;
                        idu[np] = myid;
                    }
                }
                const int first = __builtin_amdgcn_readlane(myless, 0);
                if (first < cursor) cursor = first;
                n = newn;
                __builtin_amdgcn_wave_barrier();
            } else {
                // SortArrBI::push_or_replace_non_empty_exp for each, in order (sort_arr_bi.h:159-199)
                for (int t = 0; t < m2; ++t) {
                    const float key = sk[t];
                    const int id = si[t];
                    const float lastk = keys[n - 1];
                    if (lastk <= key) {
                        if (n < a.cap) {
                            if (lane == 0) {
                                keys[n] = key;
                                idu[n] = id;
                            }
                            n++;
                        }
                    } else {
                        // insertion index.  Without a key equal to the new one in the array, the reference's
                        // exponential probe + lower_bound (sort_arr_bi.h:172-186) is simply the number of
                        // smaller keys: one parallel count.  With equal keys present the probe is
                        // replayed so the item lands inside the run exactly where the reference puts it.
                        int less = 0, leq = 0;
#pragma unroll
                        for (int e = 0; e < SA_EMAX; ++e) {
                            if (e * 64 < n) {
                                const int i = lane + 64 * e;
                                const float kv = i < n ? keys[i] : INFINITY;
                                less += __popcll(__ballot(kv < key));
                                leq += __popcll(__ballot(kv <= key));
                            }
                        }
                        int p = less;
                        if (leq != less) {
                            int curr = n - 1, prev = curr, dstep = 1;
                            while (curr > 0 && keys[curr] > key) {
                                prev = curr;
                                curr -= dstep;
                                dstep *= 2;
                                if (dstep > curr) dstep = curr;
                            }
                            p = curr;
                            for (int i = curr; i < prev && keys[i] < key; ++i) p = i + 1;
                        }
                        const int newn = n < a.cap ? n + 1 : a.cap;
                        float rk[SA_EMAX];
                        int ri[SA_EMAX];
#pragma unroll
                        for (int e = 0; e < SA_EMAX; ++e) {
                            if (e * 64 < newn) {
                                const int i = lane + 64 * e;
                                if (i > p && i < newn) {
                                    rk[e] = keys[i - 1];
                                    ri[e] = idu[i - 1];
                                }
                            }
                        }
                        __builtin_amdgcn_wave_barrier();
#pragma unroll
                        for (int e = 0; e < SA_EMAX; ++e) {
                            if (e * 64 < newn) {
                                const int i = lane + 64 * e;
                                if (i > p && i < newn) {
                                    keys[i] = rk[e];
                                    idu[i] = ri[e];
                                }
                            }
                        }
                        if (lane == 0) {
                            keys[p] = key;
                            idu[p] = id;
                        }
                        n = newn;
                        if (p < cursor) cursor = p;  // :261-266
                    }
                    __builtin_amdgcn_wave_barrier();
                }
            }
        }
        if (overflow) break;  // (set inside the round loop by the pipelined visited filter)
        lap(5);
    }
    if constexpr (P::kProf) {
        if (a.prof && lane == 0) P::prof_flush(pc);
    }

    // ---- results: first k items, ties ordered by internal id (KNNQueue holds
    //      pair<dist, Object*> and data_rearranged_ addresses grow with the id) ----
    // kRaw (the fp16 and 8-bit copies): the array goes to the f32 re-rank as it stands, array order, internal positions.
    // kPad: the fp16 form was written into the f32 epilogue and fills the slots past the count as that does; the 8-bit
    // form asks for the whole array (a.k == a.cap) into the candidate workspace, of which the re-rank reads only the
    // first out_cnt entries, and never had the padding loop.
    const int kk = overflow ? 0 : (a.k < n ? a.k : n);
    for (int i = lane; i < (P::kPad ? a.k : kk); i += 64) {
        if (i < kk) {
            const float ki = keys[i];
            const int id = idu[i] & 0x7FFFFFFF;
            int r = i;
            if constexpr (!P::kRaw) {
                for (int j = i - 1; j >= 0 && keys[j] == ki; --j) r -= ((idu[j] & 0x7FFFFFFF) > id) ? 1 : 0;
                for (int j = i + 1; j < kk && keys[j] == ki; ++j) r += ((idu[j] & 0x7FFFFFFF) < id) ? 1 : 0;
            }
            a.out_ids[(size_t)q * a.k + r] = (!P::kRaw && g.ext_ids) ? g.ext_ids[id] : id;
            a.out_dists[(size_t)q * a.k + r] = ki;
        } else if constexpr (P::kPad) {
            a.out_ids[(size_t)q * a.k + i] = -1;
            a.out_dists[(size_t)q * a.k + i] = INFINITY;
        }
    }
    if (lane == 0) {
        a.out_cnt[q] = kk;
        if (a.out_ndc) a.out_ndc[q] = ndc;
        if (a.out_hops) a.out_hops[q] = hops;
        if (a.out_hops_up) a.out_hops_up[q] = hops_up;
        if (a.status) a.status[q] = overflow ? 1 : 0;
        if (!BITSET && overflow && a.fix_list) a.fix_list[atomicAdd(a.fix_count, 1)] = q;
    }
}

}  // namespace gfxknn

// What a search kernel of one wave per query is, around the body: workgroup b walks query b; in fix_mode (a bitset launch
// after a table launch) the workgroups share out the queries whose LDS visited table filled up: workgroup b owns bitset
// slot b and clears it before every query it takes from the list.  The LAST statement of a kernel in namespace gfxknn with
// HnswArgs `a` and the dynamic LDS `smem`; P is the policy's type name.  NOTE: in fix_mode the macro RETURNS from the
// enclosing kernel after its loop.
// (a macro and no function: with the kernel's arguments handed to the body through one more inlined function, template or
//  callable, the register allocation of the bitset instantiations came out two VGPRs larger, for some of them past the 256
//  that two waves per SIMD may have)
#define HNSW_WALK_QUERIES(P, BITSET, SA_EMAX, WIDE, a, smem)                                                                \
    do {                                                                                                                    \
        if constexpr (BITSET) {                                                                                             \
            if ((a).fix_mode) {                                                                                             \
                const int cnt_ = *(a).fix_count;                                                                            \
                uint32_t* bits_ = (a).bitset + (size_t)blockIdx.x * (a).bitset_words;                                       \
                for (int slot_ = blockIdx.x; slot_ < cnt_; slot_ += gridDim.x) {                                            \
                    for (size_t i_ = threadIdx.x; i_ < (a).bitset_words; i_ += 64) bits_[i_] = 0u;                          \
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");                                                  \
                    __builtin_amdgcn_wave_barrier();                                                                        \
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");                                                  \
                    gfxknn::hnsw_walk_body<P, true, SA_EMAX, WIDE>(a, smem, (a).fix_list[slot_], bits_);                    \
                    __builtin_amdgcn_wave_barrier();                                                                        \
                }                                                                                                           \
                return;                                                                                                     \
            }                                                                                                               \
            gfxknn::hnsw_walk_body<P, true, SA_EMAX, WIDE>(a, smem, blockIdx.x, (a).bitset + (size_t)blockIdx.x * (a).bitset_words); \
        } else {                                                                                                            \
            gfxknn::hnsw_walk_body<P, false, SA_EMAX, WIDE>(a, smem, blockIdx.x, nullptr);                                  \
        }                                                                                                                   \
    } while (0)
