// What the two matrix-core scans over packed bit rows share on the device (ham_mfma_kernels.hip: u32 keys, DESIGN.md 4.10a;
// jaccard_mfma_kernels.hip: u64 keys, 4.10b): the four words of a block's four row groups, and the cut of the tile's lists.
#pragma once
#include "common_dev.hpp"

namespace gfxknn {

// x[rb][j] = word w0 + j of the row at rp[rb] (0 beyond W); VEC: one 16-byte load per row (W % 4 == 0)
template <bool VEC>
__device__ __forceinline__ void bit_rows_load(const uint32_t* const (&rp)[4], int w0, int W, uint32_t (&x)[4][4]) {
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        if constexpr (VEC) {
            const uint4 v = *reinterpret_cast<const uint4*>(rp[rb] + w0);
            x[rb][0] = v.x;
            x[rb][1] = v.y;
            x[rb][2] = v.z;
            x[rb][3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[rb][j] = w0 + j < W ? rp[rb][w0 + j] : 0u;
        }
    }
}

// Every list ([cap][QT] keys in LDS, s_cnt[QT] counts; one wave of QT lanes) cut to its k smallest keys, ascending: lane t
// sorts the list of query t of the tile (the same network for all lanes).  The network is the bitonic sorter with every
// comparator ascending (a merge's first step pairs i with its mirror), over the power of two P >= cap: the places at and
// beyond cap stand for keys above every real one (`none`), which an ascending comparator never moves, so comparators that
// reach them are skipped.  A count of k or more becomes k.  Barriers before (the appends) and after (the callers' reads).
template <typename Key, int QT>
__device__ __forceinline__ void bit_list_cut(Key* s_keys, int* s_cnt, int lane, int cap, int k, Key none) {
    __syncthreads();
    Key* s = s_keys + lane;
    const int c = s_cnt[lane];
    for (int e = 0; e < cap; ++e)
        if (e >= c) s[(size_t)e * QT] = none;
    auto order = [&](int i, int l) __attribute__((always_inline)) {
        if (l < cap) {
            const Key a = s[(size_t)i * QT], b = s[(size_t)l * QT];
            s[(size_t)i * QT] = min(a, b);
            s[(size_t)l * QT] = max(a, b);
        }
    };
    int P = 2;
    while (P < cap) P <<= 1;
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        const int hk = k2 >> 1;
        for (int t = 0; t < (P >> 1); ++t) {
            const int i = (t / hk) * k2 + (t & (hk - 1));
            order(i, i ^ (k2 - 1));
        }
        for (int j = k2 >> 2; j > 0; j >>= 1)
            for (int t = 0; t < (P >> 1); ++t) {
                const int i = 2 * t - (t & (j - 1));
                order(i, i + j);
            }
    }
    if (c >= k) s_cnt[lane] = k;
    __syncthreads();
}

}  // namespace gfxknn
