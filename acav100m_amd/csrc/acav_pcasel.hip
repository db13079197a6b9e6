// acav_pcasel.hip -- the PCA selection measures (pca, pca_ip, pca_cs, pca_l1, pca_l2; subset_selection/measures/pca.py): every
// clip is scored by how well its projected views agree, the best subset_size clips are kept.  acav_pair_scores computes the
// scores, acav_rank_desc ranks them.  The reference's measures/pca.py (PCAOptim) does the same with one torch reduction per
// clustering pair and torch.topk.
//
// Arithmetic.  For clip v and pair (c1, c2), a = y_c1[v], b = y_c2[v] (p columns each):
//   inner product      sum_j a_j b_j
//   cosine similarity  sum_j a_j b_j / (max(sqrt(sum_j a_j a_j), 1e-8) * max(sqrt(sum_j b_j b_j), 1e-8))
//   l1                 -(sum_j |a_j - b_j|)
//   l2                 -(sum_j (a_j - b_j)^2)
// every operation an individually rounded fp32 operation, every sum ONE chain from +0 over j ascending;
// score[v] = (d_0 + d_1 + ... + d_{P-1}) / (float)P with the pairs in list order (the sum starts AT d_0: a single pair of equal
// rows under l1 / l2 scores -0).  A score is a pure function of the clip's D rows and the pair list: not of n, the clip's place,
// the grid or the pointers' alignment.  No atomics.
//
// Tiling.  A workgroup of 256 lanes owns PS_R = 32 consecutive clips at a time; lane (r, g) keeps PS_NPT = 8 chains of clip r
// in registers: the chains g, g + 8, ... of the clip's list.  The list is the pairs -- for the cosine, one (c, c) chain per
// view first (the squared norms: D chains, not 2 P), then the pairs.  64 chains per clip form a PASS; a list longer than that
// takes further passes over the tile's columns, which come out of L2 then (a tile is 32 D p floats).  Within a pass the columns
// of all D views go through LDS a chunk at a time (32, 16, 8 or 4 columns, the widest that keeps the chunk within 48 KB), and a
// chain only ever advances in j: chunking leaves its order alone.  Every clip's D p floats are read from HBM once and all P
// distances come from LDS: n D p 4 bytes of traffic, where one reduction per pair reads every view 2 P / D times.
// Tail rows and columns are zero-filled IN LDS only: a chain that started at +0 is never -0, and x + (+0) leaves every other x
// alone, so the filled columns change no bit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "acav_common.h"

using namespace acav;

namespace {

constexpr int PS_R = 32;                       // clips of a tile
constexpr int PS_G = 256 / PS_R;               // chain groups of a workgroup
constexpr int PS_NPT = 8;                      // chains a lane keeps in registers
constexpr int PS_SLOTS = PS_G * PS_NPT;        // chains per clip and pass
constexpr int PS_BUF_ST = PS_SLOTS + 1;        // stride of the distances' rows in LDS (odd: the 32 clips hit 32 banks)
constexpr int PS_MAX_CHUNK = 32;
constexpr size_t PS_CHUNK_BUDGET = 48 << 10;   // LDS bytes a chunk of all views may take
constexpr int PS_PER_CU = 4;                   // workgroups per compute unit the grid is capped at
constexpr size_t PS_LDS_CU = 160 << 10;
constexpr int PS_MAX_P = 16384, PS_MAX_VIEWS = 64, PS_MAX_PAIRS = 4096;
constexpr int64_t PS_MAX_N = (int64_t)1 << 37;

// LDS row stride of a chunk: chunk + 4, an odd number of float4s, so that the 16 lanes a ds_read_b128 serves together (rows
// {0-3, 12-15, 20-27} and the like: every residue mod 16 once) fall on 16 different bank quads.  4 columns: 8 (two-way, D > 32 only)
constexpr int ps_stride(int chunk) { return chunk == 4 ? 8 : chunk + 4; }

// the launch shape, a function of (n, nviews, npairs, cus) alone
struct PairPlan {
    int chunk, stride;
    int64_t tiles;
    int per_cu, grid;
    size_t lds, scratch;
    int passes, passes_cos;
};

PairPlan pair_plan(int64_t n, int nviews, int npairs, int cus)
{
    PairPlan pl;
    pl.chunk = PS_MAX_CHUNK;
    while (pl.chunk > 4 && sizeof(float) * nviews * PS_R * ps_stride(pl.chunk) > PS_CHUNK_BUDGET) pl.chunk /= 2;
    pl.stride = ps_stride(pl.chunk);
    pl.tiles = (n + PS_R - 1) / PS_R;
    // the chunk, with the pass's distances [PS_R][PS_BUF_ST] on top of it once the chains are done; the norms [PS_R][nviews]
    pl.lds = sizeof(float) * (std::max<size_t>((size_t)nviews * PS_R * pl.stride, (size_t)PS_R * PS_BUF_ST) + (size_t)PS_R * nviews);
    pl.per_cu = (int)std::min<size_t>(PS_PER_CU, PS_LDS_CU / pl.lds);
    pl.grid = (int)std::min<int64_t>(pl.tiles, (int64_t)cus * pl.per_cu);
    pl.scratch = sizeof(void *) * (size_t)nviews + sizeof(int) * 2 * (size_t)npairs;  // the pointer table and the pair list
    pl.passes = (npairs + PS_SLOTS - 1) / PS_SLOTS;
    pl.passes_cos = (npairs + nviews + PS_SLOTS - 1) / PS_SLOTS;
    return pl;
}

enum { OP_DOT = 0, OP_L1 = 1, OP_L2 = 2 };

template <int OP>
__device__ __forceinline__ float ps_step(float acc, float a, float b)
{
    if (OP == OP_DOT) return __fadd_rn(acc, __fmul_rn(a, b));
    const float e = __fsub_rn(a, b);
    if (OP == OP_L1) return __fadd_rn(acc, fabsf(e));
    return __fadd_rn(acc, __fmul_rn(e, e));
}

template <bool VEC>
__device__ __forceinline__ float4 ps_load(const float *row, int j, int p)
{
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {
        if (j < p) v = *reinterpret_cast<const float4 *>(row + j);  // p % 4 == 0: j + 3 < p
        return v;
    }
    if (j < p) v.x = row[j];
    if (j + 1 < p) v.y = row[j + 1];
    if (j + 2 < p) v.z = row[j + 2];
    if (j + 3 < p) v.w = row[j + 3];
    return v;
}

// the first N chains of a lane over the jn columns of the chunk in LDS, four columns at a time
template <int OP, int N>
__device__ __forceinline__ void ps_advance(const float *tile, const int (&o1)[PS_NPT], const int (&o2)[PS_NPT], float (&acc)[PS_NPT], int jn)
{
    for (int jj = 0; jj < jn; jj += 4) {
        float4 a[N], b[N];
#pragma unroll
        for (int i = 0; i < N; ++i) {
            a[i] = *reinterpret_cast<const float4 *>(&tile[o1[i] + jj]);
            b[i] = *reinterpret_cast<const float4 *>(&tile[o2[i] + jj]);
        }
#pragma unroll
        for (int i = 0; i < N; ++i) {
            float s = acc[i];
            s = ps_step<OP>(s, a[i].x, b[i].x);
            s = ps_step<OP>(s, a[i].y, b[i].y);
            s = ps_step<OP>(s, a[i].z, b[i].z);
            s = ps_step<OP>(s, a[i].w, b[i].w);
            acc[i] = s;
        }
    }
}

// views[nviews]: device pointers [n][p]; pairs[npairs][2]; cosine: OP_DOT chains divided by the norms at the end of a pass
template <int OP, bool VEC>
__global__ __launch_bounds__(256) void k_pair_scores(const float *const *__restrict__ views, int nviews, int64_t n, int p,
                                                     const int *__restrict__ pairs, int npairs, int cosine, int chunk, int stride,
                                                     float *__restrict__ scores)
{
    extern __shared__ float4 ps_lds[];
    float *tile = reinterpret_cast<float *>(ps_lds);  // [nviews][PS_R][stride]
    float *buf = tile;                                // [PS_R][PS_BUF_ST]: a pass's distances, once its chains are done
    float *nrm = tile + max(nviews * PS_R * stride, PS_R * PS_BUF_ST);  // [PS_R][nviews]
    const int t = threadIdx.x, r = t & (PS_R - 1), g = t / PS_R;
    const int nnorm = cosine ? nviews : 0, nvirt = nnorm + npairs;
    const int q4 = chunk >> 2, per_view = PS_R * q4, items = nviews * per_view;
    const int64_t ntiles = (n + PS_R - 1) / PS_R;
    for (int64_t ti = blockIdx.x; ti < ntiles; ti += gridDim.x) {
        const int64_t row0 = ti * PS_R;
        float score = 0.f;
        for (int v0 = 0; v0 < nvirt; v0 += PS_SLOTS) {
            int o1[PS_NPT], o2[PS_NPT], cc[PS_NPT];
            float acc[PS_NPT];
#pragma unroll
            for (int i = 0; i < PS_NPT; ++i) {
                const int v = v0 + i * PS_G + g;
                int c1 = 0, c2 = 0;
                if (v < nnorm)
                    c1 = c2 = v;
                else if (v < nvirt)
                    c1 = pairs[2 * (v - nnorm)], c2 = pairs[2 * (v - nnorm) + 1];
                o1[i] = (c1 * PS_R + r) * stride, o2[i] = (c2 * PS_R + r) * stride, cc[i] = c1 | (c2 << 8);
                acc[i] = 0.f;
            }
            const int left = nvirt - v0 - (g & ~1);  // chains of the wave's first group (the second one has as many, or one less)
            const int nact = left <= 0 ? 0 : min(PS_NPT, (left + PS_G - 1) / PS_G);
            for (int j0 = 0; j0 < p; j0 += chunk) {
                __syncthreads();  // the previous chunk (or pass: its distances) has been read
                for (int idx = t; idx < items; idx += 256) {
                    const int c = idx / per_view, rem = idx - c * per_view, row = rem / q4, q = rem - row * q4;
                    const int64_t gr = row0 + row;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (gr < n) v = ps_load<VEC>(views[c] + (size_t)gr * p, j0 + 4 * q, p);
                    *reinterpret_cast<float4 *>(&tile[(c * PS_R + row) * stride + 4 * q]) = v;
                }
                __syncthreads();
                const int jn = min(chunk, p - j0);
                // no branch between the chains: their LDS reads are in flight together.  nact is the same for a whole wave; a
                // chain past the lane's own list advances over view 0 and is never looked at
                if (nact <= 2)
                    ps_advance<OP, 2>(tile, o1, o2, acc, jn);
                else if (nact <= 4)
                    ps_advance<OP, 4>(tile, o1, o2, acc, jn);
                else if (nact <= 6)
                    ps_advance<OP, 6>(tile, o1, o2, acc, jn);
                else
                    ps_advance<OP, 8>(tile, o1, o2, acc, jn);
            }
            __syncthreads();  // every chain of the pass is done: the chunk's LDS takes the distances
            if (cosine) {
                if (v0 == 0) {  // the norms are the first nviews <= PS_SLOTS chains
#pragma unroll
                    for (int i = 0; i < PS_NPT; ++i) {
                        const int v = i * PS_G + g;
                        // __builtin_sqrtf: correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt); __fsqrt_rn is the
                        // native, approximate root in this toolchain's headers
                        if (v < nnorm) nrm[r * nviews + v] = fmaxf(__builtin_sqrtf(acc[i]), 1e-8f);
                    }
                }
                __syncthreads();
            }
#pragma unroll
            for (int i = 0; i < PS_NPT; ++i) {
                const int v = v0 + i * PS_G + g;
                if (v >= nnorm && v < nvirt) {
                    float d = acc[i];
                    if (OP != OP_DOT)
                        d = -d;
                    else if (cosine)
                        d = __fdiv_rn(d, __fmul_rn(nrm[r * nviews + (cc[i] & 255)], nrm[r * nviews + (cc[i] >> 8)]));
                    buf[r * PS_BUF_ST + (v - v0)] = d;
                }
            }
            __syncthreads();
            if (t < PS_R) {  // the pairs in list order
                const int lo = max(v0, nnorm), hi = min(v0 + PS_SLOTS, nvirt);
                for (int v = lo; v < hi; ++v) {
                    const float d = buf[t * PS_BUF_ST + (v - v0)];
                    score = v == nnorm ? d : __fadd_rn(score, d);
                }
            }
        }
        if (t < PS_R && row0 + t < n) scores[row0 + t] = __fdiv_rn(score, (float)npairs);
    }
}

// key = (order-preserving image of the score, -0 taken for +0) << 32 | ~index: descending keys are descending scores, equal
// scores by ascending index
__global__ __launch_bounds__(256) void k_rank_keys(const float *__restrict__ scores, uint32_t n, unsigned long long *__restrict__ keys,
                                                   int *__restrict__ bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint32_t bits = __float_as_uint(scores[i]);
    if ((bits & 0x7f800000u) == 0x7f800000u) *bad = 1;  // inf or NaN (every writer stores the same value)
    if ((bits << 1) == 0) bits = 0;
    const uint32_t o = (bits >> 31) ? ~bits : (bits | 0x80000000u);
    keys[i] = ((unsigned long long)o << 32) | (uint32_t)~(uint32_t)i;
}

__global__ __launch_bounds__(256) void k_rank_unpack(const unsigned long long *__restrict__ keys, const float *__restrict__ scores,
                                                     uint32_t k, int64_t *__restrict__ ids, float *__restrict__ top)
{
    const uint64_t j = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= k) return;
    const uint32_t id = ~(uint32_t)keys[j];
    ids[j] = (int64_t)id;
    top[j] = scores[id];  // the score as stored (a -0 stays -0)
}

int use_device(int device, int *cus)
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

template <int OP, bool VEC>
int launch_pair_scores(const PairPlan &pl, hipStream_t st, const float *const *views, int nviews, int64_t n, int p, const int *pairs,
                       int npairs, int cosine, float *scores)
{
    if (pl.lds > (64u << 10))  // more dynamic LDS than a kernel gets without asking (nviews > 56)
        ACAV_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_pair_scores<OP, VEC>),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
    hipLaunchKernelGGL((k_pair_scores<OP, VEC>), dim3((unsigned)pl.grid), dim3(256), pl.lds, st, views, nviews, n, p, pairs, npairs,
                       cosine, pl.chunk, pl.stride, scores);
    return ACAV_OK;
}

}  // namespace

ACAV_EXPORT int acav_pair_scores_plan(int64_t n, int p, int nviews, int npairs, int cus, int64_t *out)
{
    ACAV_REQUIRE(out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < PS_MAX_N && p >= 1 && p <= PS_MAX_P && nviews >= 1 && nviews <= PS_MAX_VIEWS && npairs >= 1 &&
                     npairs <= PS_MAX_PAIRS && cus > 0,
                 ACAV_EINVAL, "bad sizes");
    const PairPlan pl = pair_plan(n, nviews, npairs, cus);
    out[0] = PS_R, out[1] = pl.chunk, out[2] = pl.tiles, out[3] = pl.grid, out[4] = (int64_t)pl.lds, out[5] = (int64_t)pl.scratch;
    out[6] = pl.per_cu, out[7] = pl.passes, out[8] = pl.passes_cos;
    return ACAV_OK;
}

ACAV_EXPORT int acav_pair_scores(int device, const float *const *views, int nviews, int64_t n, int p, const int *pairs, int npairs,
                                 int distance, float *scores_dev, void *stream)
{
    ACAV_REQUIRE(views && pairs && (n == 0 || scores_dev), ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < PS_MAX_N, ACAV_EINVAL, "n must be in [0, 2^37)");
    ACAV_REQUIRE(p >= 1 && p <= PS_MAX_P, ACAV_EINVAL, "p=%d must be in [1, %d]", p, PS_MAX_P);
    ACAV_REQUIRE(nviews >= 1 && nviews <= PS_MAX_VIEWS, ACAV_EINVAL, "nviews=%d must be in [1, %d]", nviews, PS_MAX_VIEWS);
    ACAV_REQUIRE(npairs >= 1 && npairs <= PS_MAX_PAIRS, ACAV_EINVAL, "npairs=%d must be in [1, %d]", npairs, PS_MAX_PAIRS);
    ACAV_REQUIRE(distance >= ACAV_PAIR_INNER_PRODUCT && distance <= ACAV_PAIR_L2, ACAV_EINVAL, "unknown distance %d", distance);
    ACAV_REQUIRE(!is_device_ptr(views) && !is_device_ptr(pairs), ACAV_EINVAL, "views and pairs are host arrays");
    for (int q = 0; q < npairs; ++q)
        ACAV_REQUIRE(pairs[2 * q] >= 0 && pairs[2 * q] < nviews && pairs[2 * q + 1] >= 0 && pairs[2 * q + 1] < nviews, ACAV_EINVAL,
                     "pair %d = (%d, %d) names a view outside [0, %d)", q, pairs[2 * q], pairs[2 * q + 1], nviews);
    if (n == 0) return ACAV_OK;
    bool vec = p % 4 == 0;
    for (int c = 0; c < nviews; ++c) {
        ACAV_REQUIRE(views[c], ACAV_EINVAL, "view %d is NULL", c);
        ACAV_REQUIRE(is_device_ptr(views[c]), ACAV_EINVAL, "view %d is read on the device: a device pointer", c);
        vec = vec && (reinterpret_cast<uintptr_t>(views[c]) & 15) == 0;
    }
    ACAV_REQUIRE(is_device_ptr(scores_dev), ACAV_EINVAL, "scores are written on the device: a device pointer");
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const PairPlan pl = pair_plan(n, nviews, npairs, cus);
    DevBuf dviews, dpairs;
    StreamDrain drain = {st};
    ACAV_TRY(upload(dviews, views, sizeof(void *) * (size_t)nviews, st));
    ACAV_TRY(upload(dpairs, pairs, sizeof(int) * 2 * (size_t)npairs, st));
    const float *const *dv = dviews.as<const float *>();
    const int *dp = dpairs.as<int>();
    const int cosine = distance == ACAV_PAIR_COSINE;
    int rc;
    if (distance == ACAV_PAIR_L1)
        rc = vec ? launch_pair_scores<OP_L1, true>(pl, st, dv, nviews, n, p, dp, npairs, 0, scores_dev)
                 : launch_pair_scores<OP_L1, false>(pl, st, dv, nviews, n, p, dp, npairs, 0, scores_dev);
    else if (distance == ACAV_PAIR_L2)
        rc = vec ? launch_pair_scores<OP_L2, true>(pl, st, dv, nviews, n, p, dp, npairs, 0, scores_dev)
                 : launch_pair_scores<OP_L2, false>(pl, st, dv, nviews, n, p, dp, npairs, 0, scores_dev);
    else
        rc = vec ? launch_pair_scores<OP_DOT, true>(pl, st, dv, nviews, n, p, dp, npairs, cosine, scores_dev)
                 : launch_pair_scores<OP_DOT, false>(pl, st, dv, nviews, n, p, dp, npairs, cosine, scores_dev);
    ACAV_TRY(rc);
    ACAV_HIP_TRY(hipGetLastError());
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}

ACAV_EXPORT int acav_rank_desc(int device, const float *scores_dev, int64_t n, int64_t k, int64_t *ids_dev, float *top_dev, void *stream)
{
    ACAV_REQUIRE(n >= 0 && n < ((int64_t)1 << 32), ACAV_EINVAL, "n must be in [0, 2^32)");
    ACAV_REQUIRE(k >= 0 && k <= n, ACAV_EINVAL, "k=%lld must be in [0, n=%lld]", (long long)k, (long long)n);
    ACAV_REQUIRE((n == 0 || scores_dev) && (k == 0 || (ids_dev && top_dev)), ACAV_EINVAL, "NULL argument");
    if (n == 0) return ACAV_OK;
    ACAV_REQUIRE(is_device_ptr(scores_dev) && (k == 0 || (is_device_ptr(ids_dev) && is_device_ptr(top_dev))), ACAV_EINVAL,
                 "scores, ids and top live on the device: device pointers");
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf keys, sorted, tmp, dbad;
    StreamDrain drain = {st};
    ACAV_TRY(keys.ensure(sizeof(unsigned long long) * (size_t)n));
    ACAV_TRY(dbad.ensure(sizeof(int)));
    ACAV_HIP_TRY(hipMemsetAsync(dbad.p, 0, sizeof(int), st));
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_rank_keys, dim3(grid), dim3(256), 0, st, scores_dev, (uint32_t)n, keys.as<unsigned long long>(), dbad.as<int>());
    ACAV_HIP_TRY(hipGetLastError());
    int bad = 0;
    ACAV_HIP_TRY(hipMemcpyAsync(&bad, dbad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(!bad, ACAV_ERANGE, "a score is not finite (inf or NaN): such scores are not ranked");
    if (k == 0) return ACAV_OK;
    ACAV_TRY(sorted.ensure(sizeof(unsigned long long) * (size_t)n));
    size_t tbytes = 0;
    ACAV_HIP_TRY(rocprim::radix_sort_keys_desc(nullptr, tbytes, keys.as<unsigned long long>(), sorted.as<unsigned long long>(), (size_t)n, 0,
                                               64, st));
    ACAV_TRY(tmp.ensure(std::max<size_t>(tbytes, 16)));
    ACAV_HIP_TRY(rocprim::radix_sort_keys_desc(tmp.p, tbytes, keys.as<unsigned long long>(), sorted.as<unsigned long long>(), (size_t)n, 0, 64,
                                               st));
    hipLaunchKernelGGL(k_rank_unpack, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, sorted.as<unsigned long long>(), scores_dev,
                       (uint32_t)k, ids_dev, top_dev);
    ACAV_HIP_TRY(hipGetLastError());
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}
