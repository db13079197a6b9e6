// acav_colstats.hip -- per-column moments of feature rows and the in-place division by a per-column constant: the whitening
// front-end of the clustering stage (acav_colstats, acav_rows_scale; clustering/whiten.py).  The reference whitens with
// scipy.cluster.vq.whiten (correspondence_retrieval/code/clustering.py:54-63): x / std(x, axis=0), no centring.
//
// Arithmetic.  Float64 on the stored fp32 values.  A SEGMENT is a run of consecutive rows (one shard's rows of one view); it is
// cut into TILES of CS_TILE rows that start at the segment's first row and never cross its end.  A tile yields, per column,
// (mean, M2 = sum (x - mean)^2) of its rows in a fixed order:
//   wave w of the workgroup takes the tile's rows 64 w .. 64 w + 63 in sub-blocks of CS_R rows; a sub-block of m valid rows
//   gives mean_b = (x_0 + x_1 + ...) / m (one IEEE division, never a multiplication by 1 / m: m equal values give exactly
//   that value back) and M2_b = sum (x_i - mean_b)^2 (an FMA chain in row order); the sub-blocks are merged in row order,
//   the four waves in wave order, with Chan's step
//     n = n_a + n_b, delta = mean_b - mean_a, mean = mean_a + delta * (n_b / n), M2 = (M2_a + M2_b) + delta^2 * (n_a n_b / n).
// k_colstats_fold merges a segment's tiles in tile order with the same step.  A column of equal values has delta == 0 and
// M2_b == 0 at every step: its M2 is exactly 0 whatever the value and the number of rows.
//
// Invariance.  Tail rows and columns are masked, never zero-filled.  A (tile, column) partial depends on the tile's rows alone,
// a segment's moments on its tiles in order: nothing depends on the grid, the compute-unit count, the other segments of the
// call, or whether the rows came from the host or the device.  No floating-point atomics.
#include <algorithm>
#include <cmath>
#include <vector>

#include "acav_common.h"

using namespace acav;

namespace {

constexpr int CS_TILE = 256;     // rows of a tile: 64 per wave
constexpr int CS_R = 16;         // rows of a sub-block held in registers
constexpr int CS_STRIP = 256;    // columns of a strip: 4 per lane
constexpr int CS_PER_CU = 8;     // workgroups per compute unit the grid is capped at
constexpr int CS_MAX_D = 16384;
constexpr int64_t CS_MAX_N = (int64_t)1 << 37;

// the launch shape of k_colstats, a function of (tiles, d, cus) alone: work item w = (tile w / strips, strip w % strips),
// workgroup b takes the items b, b + grid, ...
struct ColstatsPlan {
    int64_t tiles;
    int strips;
    int64_t items;
    int grid;
    size_t lds;
    size_t scratch;  // [tiles][2][d] float64 partials + [tiles][2] int64 descriptors
};

ColstatsPlan colstats_plan(int64_t tiles, int d, int cus)
{
    ColstatsPlan p;
    p.tiles = tiles;
    p.strips = (d + CS_STRIP - 1) / CS_STRIP;
    p.items = tiles * p.strips;
    p.grid = (int)std::min<int64_t>(p.items, (int64_t)cus * CS_PER_CU);
    p.lds = sizeof(double) * 2 * 4 * CS_STRIP;
    p.scratch = sizeof(double) * 2 * (size_t)tiles * d + sizeof(int64_t) * 2 * (size_t)tiles;
    return p;
}

struct Mom {
    double mean, m2;
};

// Chan's step with the factors f1 = n_b / n and f2 = n_a n_b / n (the same for every column)
__device__ __forceinline__ void chan(Mom &a, double mean_b, double m2_b, double f1, double f2)
{
    const double delta = mean_b - a.mean;
    a.mean = a.mean + delta * f1;
    a.m2 = (a.m2 + m2_b) + (delta * delta) * f2;
}

template <bool VEC>
__device__ __forceinline__ float4 cs_load(const float *row, int j, int d)
{
    if (VEC) return *reinterpret_cast<const float4 *>(row + j);  // d % 4 == 0 and j < d: j + 3 < d
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < d) v.x = row[j];
    if (j + 1 < d) v.y = row[j + 1];
    if (j + 2 < d) v.z = row[j + 2];
    if (j + 3 < d) v.w = row[j + 3];
    return v;
}

// desc[tile] = (first row, rows); parts[tile][0][d] = mean, parts[tile][1][d] = M2
template <bool VEC>
__global__ __launch_bounds__(256) void k_colstats(const float *__restrict__ x, int d, const int64_t *__restrict__ desc, int64_t items,
                                                  int strips, double *__restrict__ parts)
{
    __shared__ double wm[2][4][CS_STRIP];  // [mean | M2][wave][column of the strip]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t tile = item / strips;
        const int strip = (int)(item - tile * strips);
        const int64_t row0 = desc[2 * tile];
        const int rows = (int)desc[2 * tile + 1];
        const int j = strip * CS_STRIP + lane * 4;
        const int wrows = min(64, max(0, rows - wave * 64));  // rows of this wave: the same for all its lanes
        Mom acc[4];
        for (int c = 0; c < 4; ++c) acc[c].mean = acc[c].m2 = 0.0;
        if (j < d) {
            const float *base = x + (size_t)(row0 + wave * 64) * d;
            for (int r0 = 0; r0 < wrows; r0 += CS_R) {
                const int m = min(CS_R, wrows - r0);
                float4 v[CS_R];
                if (m == CS_R) {
#pragma unroll
                    for (int i = 0; i < CS_R; ++i) v[i] = cs_load<VEC>(base + (size_t)(r0 + i) * d, j, d);
                } else {
#pragma unroll
                    for (int i = 0; i < CS_R; ++i)
                        v[i] = i < m ? cs_load<VEC>(base + (size_t)(r0 + i) * d, j, d) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int i = 0; i < CS_R; ++i)
                    if (i < m) {
                        s[0] = s[0] + (double)v[i].x;
                        s[1] = s[1] + (double)v[i].y;
                        s[2] = s[2] + (double)v[i].z;
                        s[3] = s[3] + (double)v[i].w;
                    }
                const double dm = (double)m;
                double mu[4], q[4] = {0.0, 0.0, 0.0, 0.0};
                for (int c = 0; c < 4; ++c) mu[c] = s[c] / dm;
#pragma unroll
                for (int i = 0; i < CS_R; ++i)
                    if (i < m) {
                        const double e0 = (double)v[i].x - mu[0], e1 = (double)v[i].y - mu[1];
                        const double e2 = (double)v[i].z - mu[2], e3 = (double)v[i].w - mu[3];
                        q[0] = fma(e0, e0, q[0]);
                        q[1] = fma(e1, e1, q[1]);
                        q[2] = fma(e2, e2, q[2]);
                        q[3] = fma(e3, e3, q[3]);
                    }
                const double na = (double)r0, n = (double)(r0 + m);
                const double f1 = dm / n, f2 = na * dm / n;  // the first sub-block: f1 = 1, f2 = 0 -> (mu, q) itself
                for (int c = 0; c < 4; ++c) chan(acc[c], mu[c], q[c], f1, f2);
            }
        }
        __syncthreads();  // the previous item's sums have been read
        for (int c = 0; c < 4; ++c) {
            wm[0][wave][lane * 4 + c] = acc[c].mean;
            wm[1][wave][lane * 4 + c] = acc[c].m2;
        }
        __syncthreads();
        const int col = strip * CS_STRIP + t;  // thread t folds column t of the strip: the waves in wave order
        if (col < d) {
            Mom a = {wm[0][0][t], wm[1][0][t]};
            for (int w = 1; w < 4; ++w) {
                const int nb = min(64, max(0, rows - w * 64));
                if (nb == 0) break;
                const double na = (double)(w * 64), n = (double)(w * 64 + nb);
                chan(a, wm[0][w][t], wm[1][w][t], (double)nb / n, na * (double)nb / n);
            }
            parts[((size_t)tile * 2) * d + col] = a.mean;
            parts[((size_t)tile * 2 + 1) * d + col] = a.m2;
        }
    }
}

// one workgroup per (segment, 256 columns): the segment's tiles in tile order.  The factors of a step depend on the tile's
// place in the segment alone: 256 of them at a time are computed side by side (one division per thread) into LDS.
// tprefix[nseg + 1]: first tile of every segment; moments[seg][0][d] = mean, moments[seg][1][d] = M2 (zeros: an empty segment)
__global__ __launch_bounds__(256) void k_colstats_fold(const double *__restrict__ parts, int d, const int64_t *__restrict__ prefix,
                                                       const int64_t *__restrict__ tprefix, double *__restrict__ moments)
{
    __shared__ double f1[256], f2[256];
    const int t = threadIdx.x, col = blockIdx.y * 256 + t;
    const int64_t seg = blockIdx.x;
    const int64_t t0 = tprefix[seg], t1 = tprefix[seg + 1], nrows = prefix[seg + 1] - prefix[seg];
    Mom a = {0.0, 0.0};
    for (int64_t b0 = t0; b0 < t1; b0 += 256) {
        __syncthreads();
        if (b0 + t < t1) {
            const int64_t na = (b0 + t - t0) * CS_TILE;
            const int64_t nb = nrows - na < CS_TILE ? nrows - na : CS_TILE;
            const double n = (double)(na + nb);
            f1[t] = (double)nb / n;
            f2[t] = (double)na * (double)nb / n;
        }
        __syncthreads();
        const int cnt = t1 - b0 < 256 ? (int)(t1 - b0) : 256;
        if (col < d) {
            const double *p = parts + ((size_t)b0 * 2) * d + col;
            int k = 0;
            for (; k + 8 <= cnt; k += 8) {  // eight tiles' loads in flight, merged in tile order
                double pm[8], pq[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    pm[u] = p[(size_t)(k + u) * 2 * d];
                    pq[u] = p[((size_t)(k + u) * 2 + 1) * d];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) chan(a, pm[u], pq[u], f1[k + u], f2[k + u]);
            }
            for (; k < cnt; ++k) chan(a, p[(size_t)k * 2 * d], p[((size_t)k * 2 + 1) * d], f1[k], f2[k]);
        }
    }
    if (col < d) {
        moments[((size_t)seg * 2) * d + col] = a.mean;
        moments[((size_t)seg * 2 + 1) * d + col] = a.m2;
    }
}

// x[i][j] <- x[i][j] / s[j] in place.  A row takes `lpr` lanes of 4 columns each (a power of two, 256 at most), a workgroup
// walks 256 / lpr rows at a time; the lane keeps the divisors of its columns in registers for the whole walk.
template <bool VEC>
__global__ __launch_bounds__(256) void k_rows_scale(float *__restrict__ x, int64_t n, int d, const float *__restrict__ s, int lpr)
{
    const int t = threadIdx.x, lc = t & (lpr - 1), lr = t / lpr, rpp = 256 / lpr;
    const int j = (blockIdx.y * lpr + lc) * 4;
    if (j >= d) return;
    float sj[4];
    for (int c = 0; c < 4; ++c) sj[c] = j + c < d ? s[j + c] : 1.f;
    const int64_t step = (int64_t)gridDim.x * rpp;
    int64_t i = (int64_t)blockIdx.x * rpp + lr;
    if (VEC) {
        for (; i + 3 * step < n; i += 4 * step) {  // four rows' loads in flight
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4 *>(x + (size_t)(i + u * step) * d + j);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                v[u].x = v[u].x / sj[0], v[u].y = v[u].y / sj[1], v[u].z = v[u].z / sj[2], v[u].w = v[u].w / sj[3];
                *reinterpret_cast<float4 *>(x + (size_t)(i + u * step) * d + j) = v[u];
            }
        }
        for (; i < n; i += step) {
            float4 v = *reinterpret_cast<const float4 *>(x + (size_t)i * d + j);
            v.x = v.x / sj[0], v.y = v.y / sj[1], v.z = v.z / sj[2], v.w = v.w / sj[3];
            *reinterpret_cast<float4 *>(x + (size_t)i * d + j) = v;
        }
    } else {
        for (; i < n; i += step) {
            float *row = x + (size_t)i * d;
            for (int c = 0; c < 4; ++c)
                if (j + c < d) row[j + c] = row[j + c] / sj[c];
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

ACAV_EXPORT int acav_colstats_plan(int64_t n, int d, int tiles, int cus, int64_t *out)
{
    ACAV_REQUIRE(out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < CS_MAX_N && d >= 1 && d <= CS_MAX_D && cus > 0, ACAV_EINVAL, "bad sizes");
    const int64_t least = (n + CS_TILE - 1) / CS_TILE;  // one segment; every further non-empty segment may add one tile
    ACAV_REQUIRE(tiles < 0 || (tiles >= least && tiles <= n), ACAV_EINVAL, "%d tiles cannot hold %lld rows in tiles of %d", tiles,
                 (long long)n, CS_TILE);
    const ColstatsPlan p = colstats_plan(tiles < 0 ? least : tiles, d, cus);
    out[0] = CS_TILE, out[1] = p.tiles, out[2] = p.strips, out[3] = p.grid, out[4] = (int64_t)p.lds, out[5] = (int64_t)p.scratch;
    return ACAV_OK;
}

ACAV_EXPORT int acav_colstats(int device, const float *x, int64_t n, int d, const int64_t *prefix, int nseg, double *moments,
                              void *stream)
{
    ACAV_REQUIRE(prefix && moments && (n == 0 || x), ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < CS_MAX_N, ACAV_EINVAL, "n must be in [0, 2^37)");
    ACAV_REQUIRE(d >= 1 && d <= CS_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, CS_MAX_D);
    ACAV_REQUIRE(nseg >= 1, ACAV_EINVAL, "nseg=%d must be at least 1", nseg);
    ACAV_REQUIRE(prefix[0] == 0 && prefix[nseg] == n, ACAV_EINVAL, "prefix must run from 0 to n=%lld, not from %lld to %lld",
                 (long long)n, (long long)prefix[0], (long long)prefix[nseg]);
    for (int s = 0; s < nseg; ++s)
        ACAV_REQUIRE(prefix[s] <= prefix[s + 1], ACAV_EINVAL, "prefix decreases at segment %d", s);
    memset(moments, 0, sizeof(double) * 2 * (size_t)nseg * d);
    if (n == 0) return ACAV_OK;

    // tiles start at a segment's first row and end at its last
    std::vector<int64_t> tprefix((size_t)nseg + 1, 0), desc;
    for (int s = 0; s < nseg; ++s) tprefix[s + 1] = tprefix[s] + (prefix[s + 1] - prefix[s] + CS_TILE - 1) / CS_TILE;
    const int64_t tiles = tprefix[nseg];
    desc.reserve((size_t)tiles * 2);
    for (int s = 0; s < nseg; ++s)
        for (int64_t r = prefix[s]; r < prefix[s + 1]; r += CS_TILE) {
            desc.push_back(r);
            desc.push_back(std::min<int64_t>(CS_TILE, prefix[s + 1] - r));
        }

    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ColstatsPlan plan = colstats_plan(tiles, d, cus);
    // scratch of this call only (parked blocks of the library's pool)
    DevBuf stage_x, ddesc, dprefix, dtprefix, parts, out;
    StreamDrain drain = {st};
    const void *dx = nullptr;
    ACAV_TRY(to_device(x, sizeof(float) * (size_t)n * d, stage_x, st, &dx));
    ACAV_TRY(upload(ddesc, desc.data(), sizeof(int64_t) * desc.size(), st));
    ACAV_TRY(upload(dprefix, prefix, sizeof(int64_t) * ((size_t)nseg + 1), st));
    ACAV_TRY(upload(dtprefix, tprefix.data(), sizeof(int64_t) * tprefix.size(), st));
    ACAV_TRY(parts.ensure(sizeof(double) * 2 * (size_t)tiles * d));
    ACAV_TRY(out.ensure(sizeof(double) * 2 * (size_t)nseg * d));
    const float *xd = static_cast<const float *>(dx);
    const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(xd) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_colstats<true>, dim3((unsigned)plan.grid), dim3(256), 0, st, xd, d, ddesc.as<int64_t>(), plan.items,
                           plan.strips, parts.as<double>());
    else
        hipLaunchKernelGGL(k_colstats<false>, dim3((unsigned)plan.grid), dim3(256), 0, st, xd, d, ddesc.as<int64_t>(), plan.items,
                           plan.strips, parts.as<double>());
    hipLaunchKernelGGL(k_colstats_fold, dim3((unsigned)nseg, (unsigned)plan.strips), dim3(256), 0, st, parts.as<double>(), d,
                       dprefix.as<int64_t>(), dtprefix.as<int64_t>(), out.as<double>());
    ACAV_HIP_TRY(hipGetLastError());
    ACAV_HIP_TRY(hipMemcpyAsync(moments, out.p, sizeof(double) * 2 * (size_t)nseg * d, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_scale(int device, float *x_dev, int64_t n, int d, const float *std_host, void *stream)
{
    ACAV_REQUIRE(std_host && (n == 0 || x_dev), ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < CS_MAX_N, ACAV_EINVAL, "n must be in [0, 2^37)");
    ACAV_REQUIRE(d >= 1 && d <= CS_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, CS_MAX_D);
    for (int j = 0; j < d; ++j)
        ACAV_REQUIRE(std::isfinite(std_host[j]) && std_host[j] > 0.f, ACAV_EINVAL, "std[%d] = %g: every divisor must be finite and > 0",
                     j, (double)std_host[j]);
    if (n == 0) return ACAV_OK;
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    ACAV_REQUIRE(is_device_ptr(x_dev), ACAV_EINVAL, "x is scaled in place on the device: a device pointer");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf ds;
    StreamDrain drain = {st};
    ACAV_TRY(upload(ds, std_host, sizeof(float) * (size_t)d, st));
    const int quads = (d + 3) / 4;
    int lpr = 1;
    while (lpr < quads && lpr < 256) lpr *= 2;
    const int rpp = 256 / lpr, ystrips = (quads + lpr - 1) / lpr;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + rpp - 1) / rpp, (int64_t)cus * CS_PER_CU / ystrips + 1));
    const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(x_dev) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL(k_rows_scale<true>, dim3(grid, (unsigned)ystrips), dim3(256), 0, st, x_dev, n, d, ds.as<float>(), lpr);
    else
        hipLaunchKernelGGL(k_rows_scale<false>, dim3(grid, (unsigned)ystrips), dim3(256), 0, st, x_dev, n, d, ds.as<float>(), lpr);
    ACAV_HIP_TRY(hipGetLastError());
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}
