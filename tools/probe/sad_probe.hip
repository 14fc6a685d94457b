// Micro-benchmark (gfx950): the sustained issue rate of v_sad_u8 per SIMD, beside v_add_u32 in the same loop (a full-rate
// VALU instruction: one wave64 instruction per 4 cycles).  Register-only: 32 independent accumulators per lane, operands
// in registers, nothing read or written inside the timed loop.  Prints ns per wave-instruction per SIMD for 1, 2 and 4
// waves per SIMD, and the ratio SAD / ADD (1.0 = full rate, 4.0 = quarter rate).
//   hipcc --offload-arch=gfx950 -O3 tools/probe/sad_probe.hip -o sad_probe && ./sad_probe
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>

constexpr int NACC = 32;

// KIND 0: v_add_u32; 1: v_sad_u8 with three vector operands; 2: v_sad_u8 with a scalar second operand (the scan's form)
template <int KIND>
__global__ __launch_bounds__(256) void probe(uint32_t* out, int iters, uint32_t seed) {
    uint32_t acc[NACC];
    for (int i = 0; i < NACC; ++i) acc[i] = threadIdx.x + i;
    const uint32_t a = threadIdx.x * 0x01010101u + seed;
    const uint32_t sq = __builtin_amdgcn_readfirstlane(seed * 0x9E3779B9u);
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < NACC; ++i) {
            if (KIND == 0) asm volatile("v_add_u32 %0, %1, %0" : "+v"(acc[i]) : "v"(a));
            if (KIND == 1) asm volatile("v_sad_u8 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(a), "v"(a ^ 0x55u));
            if (KIND == 2) asm volatile("v_sad_u8 %0, %1, %2, %0" : "+v"(acc[i]) : "v"(a), "s"(sq));
        }
    }
    uint32_t s = 0;
    for (int i = 0; i < NACC; ++i) s += acc[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int KIND>
double run(uint32_t* out, int wgs) {
    const int iters = 20000;
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    probe<KIND><<<wgs, 256>>>(out, 10, 1u);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    probe<KIND><<<wgs, 256>>>(out, iters, 2u);
    hipEventRecord(e1);
    hipDeviceSynchronize();
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return ms;
}

int main() {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 1;
    const int cus = prop.multiProcessorCount;
    uint32_t* out;
    if (hipMalloc(&out, (size_t)cus * 4 * 256 * 4) != hipSuccess) return 1;
    const char* names[3] = {"v_add_u32", "v_sad_u8 vvv", "v_sad_u8 vsv"};
    printf("%d CUs, %d kHz\n", cus, prop.clockRate);
    for (int wps : {1, 2, 4}) {   // waves per SIMD: a workgroup of 4 waves per CU puts one on each SIMD
        const int wgs = cus * wps;
        double ns[3];
        const double ms[3] = {run<0>(out, wgs), run<1>(out, wgs), run<2>(out, wgs)};
        for (int kd = 0; kd < 3; ++kd) {
            // wave-instructions one SIMD issued: wps waves x iters x NACC
            ns[kd] = ms[kd] * 1e6 / ((double)wps * 20000 * NACC);
            printf("waves/SIMD %d  %-13s %.3f ns per wave-instruction per SIMD  (%.2f x v_add_u32)\n", wps, names[kd], ns[kd],
                   ns[kd] / ns[0]);
        }
    }
    hipFree(out);
    return 0;
}
