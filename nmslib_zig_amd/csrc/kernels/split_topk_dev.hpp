// Per-split top-k of (distance, position) keys in LDS, shared by the exact scans over sparse and string rows.
//
// A workgroup of 256 threads scans a row range for a tile of TQ queries.  Per query it keeps a buffer of P u64 keys
// ((ordered distance << 32) | position, P a power of two >= kl + 256): the candidates of one 256-row chunk are
// appended below the running threshold, a buffer that could overflow with the next chunk is compacted by a bitonic
// sort to its best kl keys (and every buffer after the last chunk), and the kl-th key becomes the threshold.
// LDS layout of a kernel: the keys first ([TQ][P]), then the kernel's own staging.
#pragma once
#include "common_dev.hpp"

namespace gfxknn {

template <int TQ>
struct SplitTopK {
    u64* keys;  // [TQ][P]
    int* cnt;   // [TQ]
    int P, kl, tile_n;
    u64 thr[TQ];

    __device__ void init(int tid) {
#pragma unroll
        for (int t = 0; t < TQ; ++t) thr[t] = ~0ull;
        for (int i = tid; i < TQ * P; i += 256) keys[i] = ~0ull;
        if (tid < TQ) cnt[tid] = 0;
    }
    // hi: the distance as 32 bits that order as the distances do
    __device__ __forceinline__ void offer(int t, uint32_t hi, int r) {
        const u64 key = ((u64)hi << 32) | (uint32_t)r;
        if (key < thr[t]) keys[(size_t)t * P + atomicAdd(&cnt[t], 1)] = key;
    }
    // after a chunk's offers; every thread of the group calls it
    __device__ void chunk_done(int tid, bool last) {
        __syncthreads();
        // every thread takes the counts BEFORE any thread can change one (the next chunk's atomics, a compaction's
        // reset): the compaction decisions below, and the barriers inside them, are then the same for the whole group
        int cnts[TQ];
#pragma unroll
        for (int t = 0; t < TQ; ++t) cnts[t] = cnt[t];
        __syncthreads();
#pragma unroll
        for (int t = 0; t < TQ; ++t) {
            const int c = cnts[t];
            if (t < tile_n && (c + 256 > P || last)) {  // the next chunk could overflow, or the range is done
                u64* kt = keys + (size_t)t * P;
                block_bitonic_u64_asc(kt, P, tid, 256);
                const int kept = c < kl ? c : kl;
                if (kept == kl) thr[t] = kt[kl - 1];
                __syncthreads();
                for (int i = kl + tid; i < P; i += 256) kt[i] = ~0ull;
                if (tid == 0) cnt[t] = kept;
                __syncthreads();
            }
        }
    }
    // the split's lists, ascending, padded to k with (-1, INFINITY); decode: a key's upper 32 bits -> the distance
    template <typename Decode>
    __device__ void write(int tid, int split, int nq, int q_first, int k, float* out_d, int32_t* out_pos,
                          Decode decode) {
        for (int t = 0; t < tile_n; ++t) {
            const size_t o = ((size_t)split * nq + q_first + t) * (size_t)k;
            for (int i = tid; i < k; i += 256) {
                const u64 key = i < kl ? keys[(size_t)t * P + i] : ~0ull;
                const bool ok = key != ~0ull;
                out_pos[o + i] = ok ? (int32_t)(uint32_t)key : -1;
                out_d[o + i] = ok ? decode((uint32_t)(key >> 32)) : INFINITY;
            }
        }
    }
};

// A 256-thread kernel with `lds` bytes of dynamic LDS (above the default limit: the attribute is raised first).
template <typename K, typename... Args>
hipError_t launch_with_lds(K kernel, dim3 grid, size_t lds, hipStream_t s, Args... args) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(256), lds, s, args...);
    return hipGetLastError();
}

}  // namespace gfxknn
