// acav_pca.hip -- the two device primitives of the PCA front-end of the clustering stage (clustering/pca.py, clustering.pca_dim):
// acav_rows_scatter, the float64 sum and scatter matrix of shifted rows, and acav_rows_project, y = (x - mean) comps^T in fp32.
// The reference runs sklearn.decomposition.PCA(n_components=dim).fit_transform on every view
// (correspondence_retrieval/code/clustering.py:62-78, pca.py: pca_features).
//
// Scatter, arithmetic.  e = (double)x - (double)shift, exact.  A SEGMENT (one shard's rows) is cut into SLICES of SC_SLICE rows
// that start at its first row and never cross its end.  The output is cut into 64 x 64 blocks; a block PAIR (bi <= bj) of one
// slice is one workgroup's work: a chain of v_mfma_f64_16x16x4_f64 over the slice's rows in row order, four rows a step, from a
// zero accumulator.  Tail rows and tail columns of e are zero-filled when a stage is loaded: they add exactly 0.  The column
// sums of a slice are one float64 chain per column in row order (taken by the diagonal pairs from the same stage).
// k_scatter_fold adds a segment's slice partials in slice order, G_s = (P_0 + P_1) + P_2 ..., and then the accumulator becomes
// accumulator + G_s, one segment after another.  Only the pairs bi <= bj -- and of a diagonal pair only i <= j -- are computed;
// element (j, i) is stored from the value of element (i, j): the matrix is symmetric to the bit.
//
// Scatter, invariance.  A slice partial depends on the slice's rows and the shift alone, G_s on the segment's slices in order,
// the accumulators on the segments in order: nothing depends on the grid, the compute-unit count, how many slices a round of
// launches takes, how the segments are spread over calls, or host / device / unaligned input (the guarded load path feeds the
// same values into the same chain).  No floating-point atomics.
//
// Projection.  y_ik = sum_j (x_ij (-) mean_j) comp_kj: one fp32 subtraction when a stage is loaded, then a chain of
// v_mfma_f32_16x16x4_f32 over the columns 0, 4, 8, ... from a zero accumulator.  Tails in n, d and p are zero-filled.  ONE code
// path for every shape: a row's outputs depend on the row, mean and comps alone -- not on n, the row's place in the call, the
// grid, or the pointer's alignment.
#include <algorithm>
#include <cmath>
#include <vector>

#include "acav_common.h"

using namespace acav;

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int PCA_MAX_D = 16384;
constexpr int64_t PCA_MAX_N = (int64_t)1 << 37;

// ---------------------------------------------------------------------------------------------------------------- scatter
constexpr int SC_SLICE = 1024;   // rows of a slice: 9.4 MB of the widest view (2304 columns) -- resident in the last-level cache
                                 // while the 666 block pairs of the slice read their two panels each
constexpr int SC_B = 64;         // rows and columns of an output block: 16 rows x 64 columns per wave
constexpr int SC_RS = 32;        // rows of a stage
constexpr int SC_ST = SC_B + 16; // float64 stage, row stride: the two rows of a half-wave's 8-byte reads fall into different banks
constexpr int SC_BB = SC_B * SC_B;
constexpr int SC_MIN_ROUND = 4, SC_MAX_ROUND = 1024;
constexpr size_t SC_PART_BYTES = (size_t)512 << 20;  // the slice partials of a round stay under this (one slice at least)
constexpr int SC_DESC_BATCH = 65536;                 // slice descriptors uploaded at a time

// the launch shape, a function of (d, cus) alone.  A ROUND is `round` consecutive slices: k_scatter_partial runs one workgroup
// per (slice of the round, block pair), k_scatter_fold then folds the round's partials in slice order.
struct ScatterPlan {
    int nb;            // blocks per side
    int64_t npairs;    // nb (nb + 1) / 2
    int64_t per_slice; // float64 values a slice's partials take: npairs * 64 * 64 + nb * 64 (the column sums)
    int round;
    size_t lds, scratch;
};

ScatterPlan scatter_plan(int d, int cus)
{
    ScatterPlan p;
    p.nb = (d + SC_B - 1) / SC_B;
    p.npairs = (int64_t)p.nb * (p.nb + 1) / 2;
    p.per_slice = p.npairs * SC_BB + (int64_t)p.nb * SC_B;
    int64_t r = (2 * (int64_t)cus + p.npairs - 1) / p.npairs;  // two workgroups per compute unit
    r = std::max<int64_t>(SC_MIN_ROUND, std::min<int64_t>(SC_MAX_ROUND, r));
    const int64_t fit = (int64_t)(SC_PART_BYTES / (sizeof(double) * (size_t)p.per_slice));
    p.round = (int)std::max<int64_t>(1, std::min<int64_t>(r, fit));
    p.lds = sizeof(double) * 2 * SC_RS * SC_ST;
    // the round's partials, the running G_s and accumulator in block form, the descriptors of a batch
    p.scratch = sizeof(double) * (size_t)p.per_slice * ((size_t)p.round + 2) + sizeof(int64_t) * 2 * SC_DESC_BATCH;
    return p;
}

__device__ __forceinline__ void pair_of(int64_t p, int nb, int &bi, int &bj)
{
    int b = 0;
    while (p >= nb - b) {
        p -= nb - b;
        ++b;
    }
    bi = b;
    bj = b + (int)p;
}

// four columns col .. col + 3 of one row as e = (double)x - (double)shift; 0 past the row count or the width
template <bool VEC>
__device__ __forceinline__ void sc_load(const float *__restrict__ x, int64_t row, bool row_ok, int d, int col, const double *sh, double *e)
{
    e[0] = e[1] = e[2] = e[3] = 0.0;
    if (!row_ok || col >= d) return;
    const float *r = x + (size_t)row * d + col;
    if (VEC) {  // d % 4 == 0 and col < d: col + 3 < d
        const float4 v = *reinterpret_cast<const float4 *>(r);
        e[0] = (double)v.x - sh[0], e[1] = (double)v.y - sh[1], e[2] = (double)v.z - sh[2], e[3] = (double)v.w - sh[3];
    } else {
        for (int c = 0; c < 4; ++c)
            if (col + c < d) e[c] = (double)r[c] - sh[c];
    }
}

// desc[2 s] = first row, desc[2 s + 1] = rows | flags << 32 of slice s of the round (flags: 1 first, 2 last of its segment)
// parts[s][pair][64][64] (the pair's block in row-major form), psums[s][nb * 64]
template <bool VEC>
__global__ __launch_bounds__(256) void k_scatter_partial(const float *__restrict__ x, int d, const float *__restrict__ shift,
                                                         const int64_t *__restrict__ desc, int nb, int64_t npairs,
                                                         double *__restrict__ parts, double *__restrict__ psums)
{
    __shared__ double stage[2][SC_RS * SC_ST];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int64_t s = blockIdx.x / npairs, pair = blockIdx.x - s * npairs;
    int bi, bj;
    pair_of(pair, nb, bi, bj);
    const int64_t row0 = desc[2 * s];
    const int rows = (int)(desc[2 * s + 1] & 0xffffffff);
    const bool diag = bi == bj;
    const int q = t & 15, r_in = t >> 4;  // this thread stages columns 4 q .. 4 q + 3 of the rows r_in and r_in + 16
    const int ci = bi * SC_B + 4 * q, cj = bj * SC_B + 4 * q;
    double shi[4], shj[4];
    for (int c = 0; c < 4; ++c) {
        shi[c] = ci + c < d ? (double)shift[ci + c] : 0.0;
        shj[c] = cj + c < d ? (double)shift[cj + c] : 0.0;
    }
    const double *sa = stage[0], *sb = diag ? stage[0] : stage[1];
    f64x4 acc[4];
    for (int ct = 0; ct < 4; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
    double colsum = 0.0;
    for (int k0 = 0; k0 < rows; k0 += SC_RS) {
        __syncthreads();  // the previous stage has been read
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = r_in + 16 * u;
            const bool ok = k0 + r < rows;
            double e[4];
            sc_load<VEC>(x, row0 + k0 + r, ok, d, ci, shi, e);
            for (int c = 0; c < 4; ++c) stage[0][r * SC_ST + 4 * q + c] = e[c];
            if (!diag) {
                sc_load<VEC>(x, row0 + k0 + r, ok, d, cj, shj, e);
                for (int c = 0; c < 4; ++c) stage[1][r * SC_ST + 4 * q + c] = e[c];
            }
        }
        __syncthreads();
        if (diag && t < SC_B)  // the column sums of block bi: the stage's rows in row order
            for (int r = 0; r < SC_RS; ++r) colsum = colsum + sa[r * SC_ST + t];
#pragma unroll
        for (int kk = 0; kk < SC_RS / 4; ++kk) {
            const double a = sa[(kk * 4 + fq) * SC_ST + wave * 16 + fr];
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const double b = sb[(kk * 4 + fq) * SC_ST + ct * 16 + fr];
                acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[ct], 0, 0, 0);
            }
        }
    }
    // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
    double *out = parts + ((size_t)s * npairs + pair) * SC_BB;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) out[(wave * 16 + fq + 4 * r) * SC_B + ct * 16 + fr] = acc[ct][r];
    if (diag && t < SC_B) psums[(size_t)s * nb * SC_B + bi * SC_B + t] = colsum;
}

// one thread per element of the block form (the pairs' blocks, then the column sums): the round's `cnt` slices in slice order.
// G / A: the running G_s and accumulator between rounds.  first / last: the call's first / last round -- the accumulator comes
// from, and goes back to, the caller's arrays (element (j, i) from the value of element (i, j)).
__global__ __launch_bounds__(256) void k_scatter_fold(const double *__restrict__ parts, const double *__restrict__ psums,
                                                      const int64_t *__restrict__ desc, int cnt, int d, int nb, int64_t npairs,
                                                      double *__restrict__ G, double *__restrict__ A, double *__restrict__ scatter,
                                                      double *__restrict__ sum, int first, int last)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t nmat = npairs * SC_BB, per_slice = nmat + (int64_t)nb * SC_B;
    if (e >= per_slice) return;
    const double *src;
    int64_t stride;
    size_t o0, o1;
    if (e < nmat) {
        const int64_t pair = e / SC_BB;
        const int loc = (int)(e - pair * SC_BB), i = loc / SC_B, j = loc % SC_B;
        int bi, bj;
        pair_of(pair, nb, bi, bj);
        const int gi = bi * SC_B + i, gj = bj * SC_B + j;
        if (gi >= d || gj >= d || (bi == bj && i > j)) return;
        src = parts + e;
        stride = nmat;
        o0 = (size_t)gi * d + gj, o1 = (size_t)gj * d + gi;
    } else {
        const int64_t c = e - nmat;
        if (c >= d) return;
        src = psums + c;
        stride = (int64_t)nb * SC_B;
        o0 = o1 = (size_t)c;
    }
    double *dst = e < nmat ? scatter : sum;
    double a = first ? dst[o0] : A[e];
    double g = first ? 0.0 : G[e];
    for (int s = 0; s < cnt; ++s) {
        const int flags = (int)(desc[2 * s + 1] >> 32);
        const double p = src[(size_t)s * stride];
        g = (flags & 1) ? p : g + p;
        if (flags & 2) a = a + g;
    }
    if (last) {
        dst[o0] = a;
        dst[o1] = a;
    } else {
        A[e] = a;
        G[e] = g;
    }
}

// ------------------------------------------------------------------------------------------------------------- projection
constexpr int PJ_M = 64;         // rows of a tile: 16 per wave
constexpr int PJ_P = 256;        // components of a pass: sixteen 16 x 16 accumulators per wave
constexpr int PJ_K = 32;         // columns of a panel
constexpr int PJ_ST = PJ_K + 4;  // fp32 stage, row stride: the 16 rows x 4 columns of a fragment fall into 64 different banks
#ifndef ACAV_PJ_MIN_WAVES
#define ACAV_PJ_MIN_WAVES 2      // waves per SIMD the projection kernel is compiled for; 1 (an experiment build) is 2.4 x slower, DESIGN 6h
#endif
constexpr int PJ_PER_CU = 2;     // two waves per SIMD (__launch_bounds__): one workgroup stages while the other multiplies

// columns j .. j + 3 of a row of x (or of the mean: row 0 of a one-row matrix), as they are stored.  No branch: the load goes
// to a clamped address inside the array, so a thread's loads leave back to back; pj_centre masks what was clamped
template <bool VEC>
__device__ __forceinline__ float4 pj_fetch(const float *__restrict__ x, int64_t row, int64_t n, int d, int j)
{
    const float *r = x + (size_t)min(row, n - 1) * d;
    if (VEC) return *reinterpret_cast<const float4 *>(r + min(j, d - 4));  // d % 4 == 0: j < d means j + 3 < d
    return make_float4(r[min(j, d - 1)], r[min(j + 1, d - 1)], r[min(j + 2, d - 1)], r[min(j + 3, d - 1)]);
}

// x (-) mean, ONE fp32 subtraction per element; 0 past the row count or the width.  Applied when the prefetched registers go to
// LDS, a panel after they were loaded
__device__ __forceinline__ float4 pj_centre(float4 a, float4 m, bool row_ok, int d, int j)
{
    float4 v;
    v.x = (row_ok && j < d) ? __fsub_rn(a.x, m.x) : 0.f;
    v.y = (row_ok && j + 1 < d) ? __fsub_rn(a.y, m.y) : 0.f;
    v.z = (row_ok && j + 2 < d) ? __fsub_rn(a.z, m.z) : 0.f;
    v.w = (row_ok && j + 3 < d) ? __fsub_rn(a.w, m.w) : 0.f;
    return v;
}

// columns j .. j + 3 of component k (the library's own copy: 16-byte aligned); 0 past p or the width.  Branch-free likewise
template <bool VEC>
__device__ __forceinline__ float4 pj_load_c(const float *__restrict__ comps, int k, int p, int d, int j)
{
    const float *r = comps + (size_t)min(k, p - 1) * d;
    float v[4];
    if (VEC) {
        const float4 q = *reinterpret_cast<const float4 *>(r + min(j, d - 4));
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    } else {
        for (int c = 0; c < 4; ++c) v[c] = r[min(j + c, d - 1)];
    }
    for (int c = 0; c < 4; ++c) v[c] = (k < p && j + c < d) ? v[c] : 0.f;
    return make_float4(v[0], v[1], v[2], v[3]);
}

// one panel: acc[pt] += the wave's 16 rows x the 16 components of tile pt, the panel's columns in ascending order.  FULL: all
// sixteen tiles; otherwise the first npt (the same chain per output either way)
template <bool FULL>
__device__ __forceinline__ void pj_multiply(const float *xw, const float *cs, int fr, int fq, int npt, f32x4 *acc)
{
    // the fragments of step kk + 1 are read from LDS while the MFMAs of step kk run
    float a[2], b[2][PJ_P / 16];
    a[0] = xw[fr * PJ_ST + fq];
#pragma unroll
    for (int pt = 0; pt < PJ_P / 16; ++pt) b[0][pt] = (FULL || pt < npt) ? cs[(pt * 16 + fr) * PJ_ST + fq] : 0.f;
#pragma unroll
    for (int kk = 0; kk < PJ_K / 4; ++kk) {
        const int cur = kk & 1, nxt = cur ^ 1;
        if (kk + 1 < PJ_K / 4) {
            a[nxt] = xw[fr * PJ_ST + (kk + 1) * 4 + fq];
#pragma unroll
            for (int pt = 0; pt < PJ_P / 16; ++pt) b[nxt][pt] = (FULL || pt < npt) ? cs[(pt * 16 + fr) * PJ_ST + (kk + 1) * 4 + fq] : 0.f;
        }
#pragma unroll
        for (int pt = 0; pt < PJ_P / 16; ++pt)
            if (FULL || pt < npt) acc[pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur], b[cur][pt], acc[pt], 0, 0, 0);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256, ACAV_PJ_MIN_WAVES) void k_rows_project(const float *__restrict__ x, int64_t n, int d, const float *__restrict__ mean,
                                                      const float *__restrict__ comps, int p, float *__restrict__ y)
{
    __shared__ float xs[PJ_M * PJ_ST];
    __shared__ float cs[PJ_P * PJ_ST];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    const int lq = t & 7, lr = t >> 3;  // this thread stages columns 4 lq .. 4 lq + 3 of the rows lr + 32 u
    const int64_t ntiles = (n + PJ_M - 1) / PJ_M;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * PJ_M;
        for (int pc0 = 0; pc0 < p; pc0 += PJ_P) {
            const int npt = (min(PJ_P, p - pc0) + 15) / 16;  // 16-component tiles of this pass: the same for every lane
            f32x4 acc[PJ_P / 16];
#pragma unroll
            for (int pt = 0; pt < PJ_P / 16; ++pt) acc[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
            float4 px[2], pm;  // the rows' next panel (HBM) and its means as stored, in flight while the current one is multiplied
#pragma unroll
            for (int u = 0; u < 2; ++u) px[u] = pj_fetch<VEC>(x, row0 + lr + 32 * u, n, d, 4 * lq);
            pm = pj_fetch<VEC>(mean, 0, 1, d, 4 * lq);
            for (int j0 = 0; j0 < d; j0 += PJ_K) {
                __syncthreads();  // the previous panel has been read
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    *reinterpret_cast<float4 *>(&xs[(lr + 32 * u) * PJ_ST + 4 * lq]) = pj_centre(px[u], pm, row0 + lr + 32 * u < n, d, j0 + 4 * lq);
#pragma unroll
                for (int u = 0; u < 8; ++u)  // the components' panel comes out of L2: the other workgroup of the CU multiplies meanwhile
                    *reinterpret_cast<float4 *>(&cs[(lr + 32 * u) * PJ_ST + 4 * lq]) =
                        pj_load_c<VEC>(comps, pc0 + lr + 32 * u, min(p, pc0 + npt * 16), d, j0 + 4 * lq);
                __syncthreads();
                if (j0 + PJ_K < d) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) px[u] = pj_fetch<VEC>(x, row0 + lr + 32 * u, n, d, j0 + PJ_K + 4 * lq);
                    pm = pj_fetch<VEC>(mean, 0, 1, d, j0 + PJ_K + 4 * lq);
                }
                if (npt == PJ_P / 16)  // a full pass: no branch between the MFMAs, the LDS reads run ahead of them
                    pj_multiply<true>(xs + wave * 16 * PJ_ST, cs, fr, fq, npt, acc);
                else
                    pj_multiply<false>(xs + wave * 16 * PJ_ST, cs, fr, fq, npt, acc);
            }
            // C/D of the f32 MFMA: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
            for (int pt = 0; pt < PJ_P / 16; ++pt)
                if (pt < npt) {
                    const int k = pc0 + pt * 16 + fr;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int64_t row = row0 + wave * 16 + fq * 4 + r;
                        if (row < n && k < p) y[(size_t)row * p + k] = acc[pt][r];
                    }
                }
        }
    }
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

}  // namespace

ACAV_EXPORT int acav_rows_scatter_plan(int64_t n, int d, int cus, int64_t *out)
{
    ACAV_REQUIRE(out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < PCA_MAX_N && d >= 1 && d <= PCA_MAX_D && cus > 0, ACAV_EINVAL, "bad sizes");
    const ScatterPlan p = scatter_plan(d, cus);
    const int64_t least = (n + SC_SLICE - 1) / SC_SLICE;  // the slices of ONE segment
    out[0] = SC_SLICE, out[1] = SC_B, out[2] = p.npairs, out[3] = p.round;
    out[4] = std::min<int64_t>(least, p.round) * p.npairs;  // workgroups of the largest launch
    out[5] = (int64_t)p.lds, out[6] = (int64_t)p.scratch;
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_scatter(int device, const float *x, int64_t n, int d, const int64_t *prefix, int nseg, const float *shift,
                                  double *sum_dev, double *scatter_dev, void *stream)
{
    ACAV_REQUIRE(prefix && shift && sum_dev && scatter_dev && (n == 0 || x), ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < PCA_MAX_N, ACAV_EINVAL, "n must be in [0, 2^37)");
    ACAV_REQUIRE(d >= 1 && d <= PCA_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, PCA_MAX_D);
    ACAV_REQUIRE(nseg >= 1, ACAV_EINVAL, "nseg=%d must be at least 1", nseg);
    ACAV_REQUIRE(prefix[0] == 0 && prefix[nseg] == n, ACAV_EINVAL, "prefix must run from 0 to n=%lld, not from %lld to %lld",
                 (long long)n, (long long)prefix[0], (long long)prefix[nseg]);
    for (int s = 0; s < nseg; ++s)
        ACAV_REQUIRE(prefix[s] <= prefix[s + 1], ACAV_EINVAL, "prefix decreases at segment %d", s);
    for (int j = 0; j < d; ++j)
        ACAV_REQUIRE(std::isfinite(shift[j]), ACAV_EINVAL, "shift[%d] = %g is not finite", j, (double)shift[j]);
    if (n == 0) return ACAV_OK;

    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    ACAV_REQUIRE(is_device_ptr(sum_dev) && is_device_ptr(scatter_dev), ACAV_EINVAL,
                 "sum and scatter are accumulators on the device: device pointers");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ScatterPlan plan = scatter_plan(d, cus);
    DevBuf stage_x, dshift, ddesc, parts, gbuf, abuf;
    StreamDrain drain = {st};
    const void *dx = nullptr;
    ACAV_TRY(to_device(x, sizeof(float) * (size_t)n * d, stage_x, st, &dx));
    ACAV_TRY(upload(dshift, shift, sizeof(float) * (size_t)d, st));
    ACAV_TRY(parts.ensure(sizeof(double) * (size_t)plan.per_slice * plan.round));
    ACAV_TRY(gbuf.ensure(sizeof(double) * (size_t)plan.per_slice));
    ACAV_TRY(abuf.ensure(sizeof(double) * (size_t)plan.per_slice));
    ACAV_TRY(ddesc.ensure(sizeof(int64_t) * 2 * SC_DESC_BATCH));
    const float *xd = static_cast<const float *>(dx);
    const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(xd) & 15) == 0;
    double *pm = parts.as<double>(), *ps = pm + (size_t)plan.npairs * SC_BB * plan.round;
    const unsigned fold_grid = (unsigned)((plan.per_slice + 255) / 256);

    // slices start at a segment's first row and end at its last; their descriptors go up a batch at a time
    int64_t total = 0;
    for (int s = 0; s < nseg; ++s) total += (prefix[s + 1] - prefix[s] + SC_SLICE - 1) / SC_SLICE;
    std::vector<int64_t> desc;
    desc.reserve((size_t)2 * std::min<int64_t>(total, SC_DESC_BATCH));
    int64_t done = 0;
    int seg = 0;
    int64_t row = 0;
    bool first = true;
    while (done < total) {
        desc.clear();
        while ((int64_t)desc.size() < 2 * SC_DESC_BATCH && done + (int64_t)desc.size() / 2 < total) {
            while (row >= prefix[seg + 1]) ++seg;  // (skips empty segments)
            const int64_t rows = std::min<int64_t>(SC_SLICE, prefix[seg + 1] - row);
            const int64_t flags = (row == prefix[seg] ? 1 : 0) | (row + rows == prefix[seg + 1] ? 2 : 0);
            desc.push_back(row);
            desc.push_back(rows | (flags << 32));
            row += rows;
        }
        const int64_t batch = (int64_t)desc.size() / 2;
        ACAV_HIP_TRY(hipMemcpyAsync(ddesc.p, desc.data(), sizeof(int64_t) * desc.size(), hipMemcpyHostToDevice, st));
        for (int64_t b0 = 0; b0 < batch; b0 += plan.round) {
            const int cnt = (int)std::min<int64_t>(plan.round, batch - b0);
            const int64_t *dd = ddesc.as<int64_t>() + 2 * b0;
            const unsigned grid = (unsigned)(cnt * plan.npairs);
            if (vec)
                hipLaunchKernelGGL(k_scatter_partial<true>, dim3(grid), dim3(256), 0, st, xd, d, dshift.as<float>(), dd, plan.nb,
                                   plan.npairs, pm, ps);
            else
                hipLaunchKernelGGL(k_scatter_partial<false>, dim3(grid), dim3(256), 0, st, xd, d, dshift.as<float>(), dd, plan.nb,
                                   plan.npairs, pm, ps);
            const int last = done + b0 + cnt == total;
            hipLaunchKernelGGL(k_scatter_fold, dim3(fold_grid), dim3(256), 0, st, pm, ps, dd, cnt, d, plan.nb, plan.npairs,
                               gbuf.as<double>(), abuf.as<double>(), scatter_dev, sum_dev, first ? 1 : 0, last);
            first = false;
        }
        ACAV_HIP_TRY(hipGetLastError());
        ACAV_HIP_TRY(hipStreamSynchronize(st));  // the batch's descriptors have been read: the host and device copies are free
        done += batch;
    }
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_project(int device, const float *x, int64_t n, int d, const float *mean, const float *comps, int p,
                                  float *y_dev, void *stream)
{
    ACAV_REQUIRE(mean && comps && (n == 0 || (x && y_dev)), ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < PCA_MAX_N, ACAV_EINVAL, "n must be in [0, 2^37)");
    ACAV_REQUIRE(d >= 1 && d <= PCA_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, PCA_MAX_D);
    ACAV_REQUIRE(p >= 1 && p <= PCA_MAX_D, ACAV_EINVAL, "p=%d must be in [1, %d]", p, PCA_MAX_D);
    if (n == 0) return ACAV_OK;
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    ACAV_REQUIRE(is_device_ptr(y_dev), ACAV_EINVAL, "y is written on the device: a device pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf stage_x, dmean, dcomps;
    StreamDrain drain = {st};
    const void *dx = nullptr;
    ACAV_TRY(to_device(x, sizeof(float) * (size_t)n * d, stage_x, st, &dx));
    ACAV_TRY(upload(dmean, mean, sizeof(float) * (size_t)d, st));
    ACAV_TRY(upload(dcomps, comps, sizeof(float) * (size_t)p * d, st));
    const float *xd = static_cast<const float *>(dx);
    const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(xd) & 15) == 0;
    const int64_t ntiles = (n + PJ_M - 1) / PJ_M;
    const unsigned grid = (unsigned)std::min<int64_t>(ntiles, (int64_t)cus * PJ_PER_CU);
    if (vec)
        hipLaunchKernelGGL(k_rows_project<true>, dim3(grid), dim3(256), 0, st, xd, n, d, dmean.as<float>(), dcomps.as<float>(), p, y_dev);
    else
        hipLaunchKernelGGL(k_rows_project<false>, dim3(grid), dim3(256), 0, st, xd, n, d, dmean.as<float>(), dcomps.as<float>(), p, y_dev);
    ACAV_HIP_TRY(hipGetLastError());
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}
