// mfma_f64_rate.hip -- what a bare loop of v_mfma_f64_16x16x4_f64 reaches on this chip: the flop roof tools/bench_pca.py judges
// acav_rows_scatter by.  Every wave keeps eight independent accumulators and issues `iters` rounds of eight MFMAs on register
// operands: no memory traffic inside the loop.  Prints one JSON line.
//   hipcc --offload-arch=gfx950 -O3 tools/exp/mfma_f64_rate.hip -o tools/exp/mfma_f64_rate && tools/exp/mfma_f64_rate [iters] [waves per SIMD]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define CHECK(e)                                                                        \
    do {                                                                                \
        hipError_t _e = (e);                                                            \
        if (_e != hipSuccess) {                                                         \
            fprintf(stderr, "%s failed: %s\n", #e, hipGetErrorString(_e));              \
            return 1;                                                                   \
        }                                                                               \
    } while (0)

__global__ __launch_bounds__(256) void k_mfma_f64(int iters, double seed, double *out)
{
    f64x4 acc[8];
    for (int i = 0; i < 8; ++i) acc[i] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double a = seed + threadIdx.x * 1e-3, b = seed - threadIdx.x * 1e-3;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[i], 0, 0, 0);
    }
    double s = 0.0;
    for (int i = 0; i < 8; ++i) s += acc[i][0] + acc[i][1] + acc[i][2] + acc[i][3];
    out[(size_t)blockIdx.x * 256 + threadIdx.x] = s;
}

int main(int argc, char **argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 20000;
    const int wps = argc > 2 ? atoi(argv[2]) : 2;  // waves per SIMD = workgroups of four waves per compute unit
    int cus = 0;
    CHECK(hipSetDevice(0));
    CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const int grid = cus * wps;
    double *out = nullptr;
    CHECK(hipMalloc(&out, sizeof(double) * (size_t)grid * 256));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int rep = 0; rep < 7; ++rep) {  // the first two warm up
        CHECK(hipEventRecord(e0, nullptr));
        hipLaunchKernelGGL(k_mfma_f64, dim3(grid), dim3(256), 0, nullptr, iters, 1.0, out);
        CHECK(hipEventRecord(e1, nullptr));
        CHECK(hipEventSynchronize(e1));
        float t = 0.f;
        CHECK(hipEventElapsedTime(&t, e0, e1));
        if (rep >= 2) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    const double med = ms[ms.size() / 2];
    const double flops = 2.0 * 16 * 16 * 4 * 8.0 * iters * 4.0 * grid;  // per MFMA x per round x rounds x waves
    printf("{\"cus\": %d, \"waves_per_simd\": %d, \"iters\": %d, \"ms\": %.4f, \"tflops\": %.3f}\n", cus, wps, iters, med, flops / med / 1e9);
    CHECK(hipFree(out));
    return 0;
}
