// How far is the raw logarithm instruction (v_log_f32, __builtin_amdgcn_logf) from log2?  Sweeps every f32 in [2^-100, 2^128)
// and reports the largest error against the f64 log2, in ulp of the result.  The Jensen-Shannon filter's bound
// (nmslib_zig_amd/csrc/diverg_js_filter.hpp) assumes at most djs::kHwLog2Ulps.
//   hipcc --offload-arch=gfx950 -O3 tools/probe/hwlog_probe.hip -o hwlog_probe && ./hwlog_probe
// (the library's Makefile builds it as csrc/build/hwlog_probe; tests/test_gpu_js_fast.py runs that)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../nmslib_zig_amd/csrc/diverg_js_filter.hpp"

// one thread per 2^12 consecutive floats
__global__ __launch_bounds__(256) void hwlog_probe_kernel(uint32_t first, uint32_t chunks, double* worst, uint32_t* at) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= chunks) return;
    double w = 0;
    uint32_t wa = 0;
    for (uint32_t i = 0; i < 4096; ++i) {
        const uint32_t bits = first + c * 4096u + i;
        const float s = __uint_as_float(bits);
        const float l = __builtin_amdgcn_logf(s);
        const double t = log2((double)s);
        // ulp of the result: the spacing of f32 at |t| (t = 0 only at s = 1, where any error counts against the least normal)
        int e;
        frexp(t == 0 ? 1.17549435e-38 : t, &e);
        const double err = fabs((double)l - t) / ldexp(1.0, e - 24);
        if (err > w) w = err, wa = bits;
    }
    worst[c] = w;
    at[c] = wa;
}

int main() {
    const uint32_t first = (127u - 100u) << 23, last = 0x7F800000u;   // 2^-100 .. below +inf
    const uint32_t chunks = (last - first) / 4096u;
    double* d_w;
    uint32_t* d_at;
    if (hipMalloc(&d_w, chunks * sizeof(double)) != hipSuccess || hipMalloc(&d_at, chunks * 4) != hipSuccess) return 2;
    hipLaunchKernelGGL(hwlog_probe_kernel, dim3((chunks + 255) / 256), dim3(256), 0, 0, first, chunks, d_w, d_at);
    double* w = new double[chunks];
    uint32_t* at = new uint32_t[chunks];
    if (hipMemcpy(w, d_w, chunks * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(at, d_at, chunks * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        std::printf("hwlog_probe: %s\n", hipGetErrorString(hipGetLastError()));
        return 2;
    }
    double worst = 0;
    uint32_t where = 0;
    for (uint32_t c = 0; c < chunks; ++c)
        if (w[c] > worst) worst = w[c], where = at[c];
    std::printf("{\"floats\": %llu, \"max_ulp\": %.9f, \"at_bits\": \"0x%08x\", \"kHwLog2Ulps\": %.1f}\n",
                (unsigned long long)chunks * 4096ull, worst, where, gfxknn::djs::kHwLog2Ulps);
    return 0;
}
