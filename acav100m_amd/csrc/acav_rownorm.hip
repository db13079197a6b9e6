// acav_rownorm.hip -- L2 normalisation of feature rows in place: the third front-end stage of the clustering stage
// (clustering.normalize, clustering/normalize.py) and the centre renormalisation of spherical Lloyd k-means
// (clustering.spherical, clustering/lloyd.py: finish_iteration).  faiss: normalize_L2 and Kmeans(spherical=True), the clusterer
// the reference's correspondence_retrieval/code/clustering.py runs by default.
//
// Arithmetic (the definition in full: include/acav_hip.h).  One wave takes one row.  Lane l takes the 16-byte piece
// 4l .. 4l+3 of every 256-column BLOCK of the row, so lane l owns the four float64 chains 4l .. 4l+3 of the 256: chain q sums
// (double)x_j * (double)x_j (exact products, no FMA) over the columns j = q, q + 256, ... in ascending order from +0.0.  The lane
// folds its four chains as (c0 + c1) + (c2 + c3), six xor-butterfly steps (1, 2, 4, 8, 16, 32) leave the same ss in every lane,
// norm = sqrt(ss), and every element becomes (float)((double)x / norm): one IEEE double division, one rounding to fp32.
// A column past d loads as +0.0 and adds exactly 0.  ss == 0: the row is left alone and counted as a zero row; ss not finite:
// left alone and counted as a bad row.
//
// Shape.  A row is read from HBM once and written once.  Up to RN_REG_BLOCKS blocks (4096 columns) the wave keeps the row in
// registers (k_rows_normalize: four waves, i.e. four rows at a time per workgroup; rows of at most 1024 columns have the next
// row's loads in flight under the reduction and the divisions of the current one); wider rows (k_rows_normalize_lds: one wave per
// workgroup) park the row in LDS, each lane reading back exactly the pieces it wrote, so the wave needs no barrier.  16-byte
// loads and stores when d % 4 == 0 and the table starts on a 16-byte boundary (then every row does), guarded single elements
// otherwise: both fill the same registers, the arithmetic is one piece of code.  No atomics but the two integer counters, one
// add per wave at most.  Nothing depends on n, the row's place, the grid or the path.
#include <algorithm>
#include <cmath>

#include "acav_common.h"

using namespace acav;

namespace {

constexpr int RN_BLOCK = 256;        // columns of a block: 4 per lane
constexpr int RN_REG_BLOCKS = 16;    // blocks of a row the register path holds: 4096 columns
constexpr int RN_PF_BLOCKS = 4;      // ... and up to which it loads the next row ahead
constexpr int RN_WAVES = 4;          // rows a workgroup of the register path takes at a time
constexpr int RN_PER_CU = 8;         // workgroups per compute unit the grid is capped at
constexpr int RN_LDS_PER_CU = 160 * 1024;
constexpr int RN_MAX_D = 16384;
constexpr int64_t RN_MAX_N = (int64_t)1 << 37;

// the launch shape, a function of (n, d, cus) alone: workgroup b takes the rows b * wg_rows + wave, then grid * wg_rows further on
struct RownormPlan {
    int blocks;
    bool lds;
    int wg_rows;
    int grid;
    size_t lds_bytes;
};

RownormPlan rownorm_plan(int64_t n, int d, int cus)
{
    RownormPlan p;
    p.blocks = (d + RN_BLOCK - 1) / RN_BLOCK;
    p.lds = p.blocks > RN_REG_BLOCKS;
    p.wg_rows = p.lds ? 1 : RN_WAVES;
    p.lds_bytes = p.lds ? sizeof(float) * RN_BLOCK * (size_t)p.blocks : 0;
    const int per_cu = p.lds ? std::max(1, std::min(RN_PER_CU, (int)(RN_LDS_PER_CU / p.lds_bytes))) : RN_PER_CU;
    p.grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + p.wg_rows - 1) / p.wg_rows, (int64_t)cus * per_cu));
    return p;
}

template <bool VEC>
__device__ __forceinline__ float4 rn_load(const float *row, int j, int d)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {
        if (j < d) v = *reinterpret_cast<const float4 *>(row + j);  // d % 4 == 0: j + 3 < d
        return v;
    }
    if (j < d) v.x = row[j];
    if (j + 1 < d) v.y = row[j + 1];
    if (j + 2 < d) v.z = row[j + 2];
    if (j + 3 < d) v.w = row[j + 3];
    return v;
}

template <bool VEC>
__device__ __forceinline__ void rn_store(float *row, int j, int d, float4 v)
{
    if (VEC) {
        if (j < d) *reinterpret_cast<float4 *>(row + j) = v;
        return;
    }
    if (j < d) row[j] = v.x;
    if (j + 1 < d) row[j + 1] = v.y;
    if (j + 2 < d) row[j + 2] = v.z;
    if (j + 3 < d) row[j + 3] = v.w;
}

// one block's four squares onto the lane's four chains
__device__ __forceinline__ void rn_square(double c[4], float4 v)
{
    const double x0 = (double)v.x, x1 = (double)v.y, x2 = (double)v.z, x3 = (double)v.w;
    c[0] = c[0] + x0 * x0;
    c[1] = c[1] + x1 * x1;
    c[2] = c[2] + x2 * x2;
    c[3] = c[3] + x3 * x3;
}

// the lane's four chains -> ss, the same in all 64 lanes
__device__ __forceinline__ double rn_fold(const double c[4])
{
    double p = (c[0] + c[1]) + (c[2] + c[3]);
#pragma unroll
    for (int m = 1; m < 64; m *= 2) p = p + __shfl_xor(p, m, 64);
    return p;
}

__device__ __forceinline__ float4 rn_divide(float4 v, double norm)
{
    return make_float4((float)((double)v.x / norm), (float)((double)v.y / norm), (float)((double)v.z / norm),
                       (float)((double)v.w / norm));
}

// counters[0] += zero rows, counters[1] += bad rows of this wave
__device__ __forceinline__ void rn_count(unsigned long long *counters, int lane, unsigned zero, unsigned bad)
{
    if (lane == 0 && zero) atomicAdd(&counters[0], (unsigned long long)zero);
    if (lane == 0 && bad) atomicAdd(&counters[1], (unsigned long long)bad);
}

// rows of at most NB blocks, in registers
template <int NB, bool VEC>
__global__ __launch_bounds__(64 * RN_WAVES) void k_rows_normalize(float *__restrict__ x, int64_t n, int d, unsigned long long *counters)
{
    constexpr bool PF = NB <= RN_PF_BLOCKS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t step = (int64_t)gridDim.x * RN_WAVES;
    unsigned zero = 0, bad = 0;
    int64_t i = (int64_t)blockIdx.x * RN_WAVES + wave;
    float4 v[NB], w[PF ? NB : 1];
    if (i < n) {
#pragma unroll
        for (int b = 0; b < NB; ++b) v[b] = rn_load<VEC>(x + (size_t)i * d, b * RN_BLOCK + lane * 4, d);
    }
    while (i < n) {
        float *row = x + (size_t)i * d;
        const int64_t nxt = i + step;
        if (PF && nxt < n) {
#pragma unroll
            for (int b = 0; b < NB; ++b) w[b] = rn_load<VEC>(x + (size_t)nxt * d, b * RN_BLOCK + lane * 4, d);
        }
        double c[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (b * RN_BLOCK < d) rn_square(c, v[b]);
        const double ss = rn_fold(c);
        if (ss == 0.0) {
            ++zero;
        } else if (!(ss <= 1.7976931348623157e308)) {  // inf or NaN
            ++bad;
        } else {
            const double norm = sqrt(ss);
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (b * RN_BLOCK < d) rn_store<VEC>(row, b * RN_BLOCK + lane * 4, d, rn_divide(v[b], norm));
        }
        if (PF) {
#pragma unroll
            for (int b = 0; b < NB; ++b) v[b] = w[b];
        } else if (nxt < n) {
#pragma unroll
            for (int b = 0; b < NB; ++b) v[b] = rn_load<VEC>(x + (size_t)nxt * d, b * RN_BLOCK + lane * 4, d);
        }
        i = nxt;
    }
    rn_count(counters, lane, zero, bad);
}

// wider rows: one wave per workgroup, the row parked in LDS as [block][lane] pieces of 16 bytes
template <bool VEC>
__global__ __launch_bounds__(64) void k_rows_normalize_lds(float *__restrict__ x, int64_t n, int d, int blocks, unsigned long long *counters)
{
    extern __shared__ float4 rn_row[];
    const int lane = threadIdx.x;
    unsigned zero = 0, bad = 0;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        float *row = x + (size_t)i * d;
        double c[4] = {0.0, 0.0, 0.0, 0.0};
        int b = 0;
        for (; b + 8 <= blocks; b += 8) {  // eight blocks' loads in flight
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = rn_load<VEC>(row, (b + u) * RN_BLOCK + lane * 4, d);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                rn_square(c, v[u]);
                rn_row[(b + u) * 64 + lane] = v[u];
            }
        }
        for (; b < blocks; ++b) {
            const float4 v = rn_load<VEC>(row, b * RN_BLOCK + lane * 4, d);
            rn_square(c, v);
            rn_row[b * 64 + lane] = v;
        }
        const double ss = rn_fold(c);
        if (ss == 0.0) {
            ++zero;
        } else if (!(ss <= 1.7976931348623157e308)) {
            ++bad;
        } else {
            const double norm = sqrt(ss);
            for (b = 0; b < blocks; ++b)  // the lane reads back what it wrote itself
                rn_store<VEC>(row, b * RN_BLOCK + lane * 4, d, rn_divide(rn_row[b * 64 + lane], norm));
        }
    }
    rn_count(counters, lane, zero, bad);
}

template <bool VEC>
void rn_launch(const RownormPlan &p, hipStream_t st, float *x, int64_t n, int d, unsigned long long *counters)
{
    const dim3 grid((unsigned)p.grid), wg(64 * p.wg_rows);
    if (p.lds)
        hipLaunchKernelGGL(k_rows_normalize_lds<VEC>, grid, wg, p.lds_bytes, st, x, n, d, p.blocks, counters);
    else if (p.blocks <= 1)
        hipLaunchKernelGGL((k_rows_normalize<1, VEC>), grid, wg, 0, st, x, n, d, counters);
    else if (p.blocks <= 2)
        hipLaunchKernelGGL((k_rows_normalize<2, VEC>), grid, wg, 0, st, x, n, d, counters);
    else if (p.blocks <= 4)
        hipLaunchKernelGGL((k_rows_normalize<4, VEC>), grid, wg, 0, st, x, n, d, counters);
    else if (p.blocks <= 8)
        hipLaunchKernelGGL((k_rows_normalize<8, VEC>), grid, wg, 0, st, x, n, d, counters);
    else
        hipLaunchKernelGGL((k_rows_normalize<RN_REG_BLOCKS, VEC>), grid, wg, 0, st, x, n, d, counters);
}

int rn_use_device(int device, int *cus)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0) {
        (void)hipGetLastError();
        set_error("no HIP device available: this library does not fall back to the CPU");
        return ACAV_EHIP;
    }
    ACAV_REQUIRE(device >= 0 && device < n, ACAV_EINVAL, "device %d out of range (have %d)", device, n);
    ACAV_HIP_TRY(hipSetDevice(device));
    ACAV_HIP_TRY(hipDeviceGetAttribute(cus, hipDeviceAttributeMultiprocessorCount, device));
    return ACAV_OK;
}

}  // namespace

ACAV_EXPORT int acav_rows_normalize_plan(int64_t n, int d, int cus, int64_t *out)
{
    ACAV_REQUIRE(out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < RN_MAX_N && d >= 1 && d <= RN_MAX_D && cus > 0, ACAV_EINVAL, "bad sizes");
    const RownormPlan p = rownorm_plan(n, d, cus);
    out[0] = p.wg_rows, out[1] = p.blocks, out[2] = p.lds ? 1 : 0, out[3] = p.grid, out[4] = (int64_t)p.lds_bytes;
    out[5] = (int64_t)p.grid * p.wg_rows;
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_normalize(int device, float *x_dev, int64_t n, int d, int64_t *zero_rows_host, int64_t *bad_rows_host,
                                    void *stream)
{
    ACAV_REQUIRE(zero_rows_host && bad_rows_host && (n == 0 || x_dev), ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < RN_MAX_N, ACAV_EINVAL, "n must be in [0, 2^37)");
    ACAV_REQUIRE(d >= 1 && d <= RN_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, RN_MAX_D);
    if (n == 0) {
        *zero_rows_host = *bad_rows_host = 0;
        return ACAV_OK;
    }
    int cus = 0;
    ACAV_TRY(rn_use_device(device, &cus));
    ACAV_REQUIRE(is_device_ptr(x_dev), ACAV_EINVAL, "x is normalised in place on the device: a device pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RownormPlan plan = rownorm_plan(n, d, cus);
    DevBuf dcount;
    StreamDrain drain = {st};
    ACAV_TRY(dcount.ensure(2 * sizeof(unsigned long long)));
    ACAV_HIP_TRY(hipMemsetAsync(dcount.p, 0, 2 * sizeof(unsigned long long), st));
    const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(x_dev) & 15) == 0;
    if (vec)
        rn_launch<true>(plan, st, x_dev, n, d, dcount.as<unsigned long long>());
    else
        rn_launch<false>(plan, st, x_dev, n, d, dcount.as<unsigned long long>());
    ACAV_HIP_TRY(hipGetLastError());
    unsigned long long got[2] = {0, 0};
    ACAV_HIP_TRY(hipMemcpyAsync(got, dcount.p, sizeof(got), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    *zero_rows_host = (int64_t)got[0], *bad_rows_host = (int64_t)got[1];
    return ACAV_OK;
}
