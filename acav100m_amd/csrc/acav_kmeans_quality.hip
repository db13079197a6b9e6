// acav_kmeans_quality.hip -- "how far, and how far to the next one": per-row and per-cluster distance statistics of labelled
// rows (acav_kmeans_quality; KMeans.quality, clustering/evaluate.py).  No counterpart in the reference, which throws the
// mean min-distance of KMeans.add away (run_clustering.py:171-175).
//
// Arithmetic.  Everything is float64 on the stored fp32 values: D_ik = (||x_i||^2 + ||c_k||^2) - 2 x_i.c_k, clamped at 0,
// with x_i.c_k on v_mfma_f64_16x16x4_f64.  The rows are widened in registers on their way from the LDS stage (fp32) into the
// A operand; the centres are widened once per call (k_quality_centres, which also sums ||c_k||^2).
//
// Split invariance.  ONE code path for every shape: tails in n, d and K are zero-filled when a stage is loaded (a zero
// operand adds an exact 0 to a dot) and masked in the epilogue.  A row's dot with centre k is the same chain of MFMAs over the
// columns 0, 4, 8, ... whatever tile, launch or call the row sits in, ||x_i||^2 is four interleaved FMA chains (columns
// q, q + 4, ...) folded (p0 + p1) + (p2 + p3), and the minimum over k is order-free: row_stats do not depend on how the rows
// are split into calls.
//
// Reduction order.  No floating-point atomics.  A workgroup takes the row tiles b, b + grid, ... in that order and adds each
// tile's rows, in row order, to its [K][ACAV_QUALITY_COLS] sums in LDS (one lane per column); the sums leave as per-workgroup
// partials and k_quality_fold adds them in workgroup order: the same call gives the same bits.
//
// acav_kmeans_probes (KMeans.probe_centers, the multi-probe dedup) is the same sweep keeping, per row, the m - 1 nearest other
// centres instead of the nearest one: k_probes below.
#include <algorithm>

#include "acav_kmeans_shared.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int QM = 64;        // rows of a tile: 16 per wave
constexpr int QN = 64;        // centres of a pass: four 16 x 16 accumulators per wave
constexpr int QD = 32;        // columns of a stage
constexpr int QXS = QD + 4;   // fp32 row stage, row stride: the 16 rows x 4 columns of an A fragment fall into 64 different banks
constexpr int QCS = QD + 2;   // f64 centre stage, row stride: the 32 lanes of a half-wave's 8-byte reads fall into different bank pairs
constexpr int QC = ACAV_QUALITY_COLS;
constexpr int QV = 8;         // per-row values of a tile kept in LDS: a2, b2, then the QC columns' addends (count is implicit)
constexpr int QUALITY_MAX_K = 2048;  // [K][QC] sums + stages: 126 KB of a workgroup's 160 KB

constexpr size_t quality_lds(int K)
{
    return sizeof(double) * ((size_t)K * QC + (size_t)QN * QCS + (size_t)QV * QM) + sizeof(float) * QM * QXS + sizeof(int) * QM;
}
static_assert(quality_lds(QUALITY_MAX_K) <= 160 * 1024, "the per-cluster sums of the largest K must fit a workgroup's LDS");

// the launch shape of k_quality, a function of (n, K, cus) alone: as many workgroups per CU as their LDS lets live there (4 at
// most), each taking the row tiles b, b + grid, ...
struct QualityPlan {
    int64_t ntiles;
    int grid;
    size_t lds;
    int per_cu;
};

QualityPlan quality_plan(int64_t n, int K, int cus)
{
    QualityPlan p;
    p.ntiles = (n + QM - 1) / QM;
    p.lds = quality_lds(K);
    p.per_cu = (int)std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / p.lds));
    p.grid = (int)std::min<int64_t>(p.ntiles, (int64_t)cus * p.per_cu);
    return p;
}

// labels outside [0, K): counted before anything indexes LDS with them
__global__ __launch_bounds__(256) void k_quality_labels(const int64_t *__restrict__ labels, int64_t n, int K, unsigned *__restrict__ bad)
{
    unsigned mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        mine += (labels[i] < 0 || labels[i] >= K) ? 1u : 0u;
    if (mine) atomicAdd(bad, mine);
}

// one wave per centre: cd[k] <- (double)c[k], cn[k] <- sum_j cd[k][j]^2 (lane l: columns l, l + 64, ...; then a fixed tree)
__global__ __launch_bounds__(64) void k_quality_centres(const float *__restrict__ c, int d, double *__restrict__ cd, double *__restrict__ cn)
{
    const size_t base = (size_t)blockIdx.x * d;
    double p = 0.0;
    for (int j = threadIdx.x; j < d; j += 64) {
        const double v = (double)c[base + j];
        cd[base + j] = v;
        p = fma(v, v, p);
    }
    for (int m = 32; m >= 1; m >>= 1) p = p + __shfl_xor(p, m);
    if (threadIdx.x == 0) cn[blockIdx.x] = p;
}

__global__ __launch_bounds__(256) void k_quality(const float *__restrict__ x, int64_t n, int d, const double *__restrict__ cd,
                                                 const double *__restrict__ cn, int K, const int64_t *__restrict__ labels,
                                                 double *__restrict__ row_stats, double *__restrict__ partials)
{
    extern __shared__ double q_smem[];
    double *sums = q_smem;                       // [K][QC]
    double *cs = sums + (size_t)K * QC;          // [QN][QCS]
    double *rv = cs + QN * QCS;                  // [QV][QM]
    float *xs = reinterpret_cast<float *>(rv + QV * QM);  // [QM][QXS]
    int *labs = reinterpret_cast<int *>(xs + QM * QXS);   // [QM]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;    // fragment row (A) / column (B) and k index of this lane
    const double inf = __builtin_inf();

    for (int i = t; i < K * QC; i += 256) sums[i] = 0.0;
    const int64_t ntiles = (n + QM - 1) / QM;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * QM;
        if (t < QM) labs[t] = row0 + t < n ? (int)labels[row0 + t] : -1;
        double a2[4], b2[4], xn[4] = {0.0, 0.0, 0.0, 0.0};
        int lab[4] = {-1, -1, -1, -1};
        for (int r = 0; r < 4; ++r) a2[r] = b2[r] = inf;
        double xn_part = 0.0;
        for (int k0 = 0; k0 < K; k0 += QN) {
            f64x4 acc[4];
            for (int ct = 0; ct < 4; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
            for (int j0 = 0; j0 < d; j0 += QD) {
                __syncthreads();  // the previous stage has been read
                for (int i = t; i < QM * QD; i += 256) {
                    const int r = i >> 5, c = i & 31;
                    const bool ok = row0 + r < n && j0 + c < d;
                    xs[r * QXS + c] = ok ? x[(size_t)(row0 + r) * d + j0 + c] : 0.f;
                }
                for (int i = t; i < QN * QD; i += 256) {
                    const int r = i >> 5, c = i & 31;
                    const bool ok = k0 + r < K && j0 + c < d;
                    cs[r * QCS + c] = ok ? cd[(size_t)(k0 + r) * d + j0 + c] : 0.0;
                }
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < QD / 4; ++kk) {
                    const double a = (double)xs[(wave * 16 + fr) * QXS + kk * 4 + fq];
                    if (k0 == 0) xn_part = fma(a, a, xn_part);
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const double b = cs[(ct * 16 + fr) * QCS + kk * 4 + fq];
                        acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[ct], 0, 0, 0);
                    }
                }
            }
            if (k0 == 0) {  // ||x||^2 of the wave's 16 rows: (p0 + p1) + (p2 + p3), then to the lanes that hold the rows' results
                double v = xn_part + __shfl_xor(xn_part, 16);
                v = v + __shfl_xor(v, 32);
                if (fq == 0) rv[wave * 16 + fr] = v;
                __syncthreads();
                for (int r = 0; r < 4; ++r) {  // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
                    xn[r] = rv[wave * 16 + fq + 4 * r];
                    lab[r] = labs[wave * 16 + fq + 4 * r];
                }
            }
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int k = k0 + ct * 16 + fr;
                if (k >= K) continue;
                const double ck = cn[k];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double dist = (xn[r] + ck) - 2.0 * acc[ct][r];
                    dist = dist < 0.0 ? 0.0 : dist;
                    if (k == lab[r])
                        a2[r] = dist;
                    else
                        b2[r] = dist < b2[r] ? dist : b2[r];
                }
            }
        }
        // the 16 lanes that share lane >> 4 hold one row's centres between them: exactly one has a2, the minimum is order-free
        for (int r = 0; r < 4; ++r)
            for (int m = 1; m < 16; m <<= 1) {
                const double oa = __shfl_xor(a2[r], m), ob = __shfl_xor(b2[r], m);
                a2[r] = oa < a2[r] ? oa : a2[r];
                b2[r] = ob < b2[r] ? ob : b2[r];
            }
        __syncthreads();  // every wave has taken its ||x||^2 out of rv
        if (fr == 0)
            for (int r = 0; r < 4; ++r) {
                rv[0 * QM + wave * 16 + fq + 4 * r] = a2[r];
                rv[1 * QM + wave * 16 + fq + 4 * r] = b2[r];
            }
        __syncthreads();
        if (t < QM && row0 + t < n) {
            const double a = rv[t], b = rv[QM + t];
            if (row_stats) {
                row_stats[(size_t)(row0 + t) * 2] = a;
                row_stats[(size_t)(row0 + t) * 2 + 1] = b;
            }
            const double sa = sqrt(a), sb = sqrt(b), m = sa > sb ? sa : sb;
            rv[2 * QM + t] = a;                                        // ACAV_QUALITY_SUM_A2
            rv[3 * QM + t] = sa;                                       // ACAV_QUALITY_SUM_SQRT_A2
            rv[4 * QM + t] = (K == 1 || !(m > 0.0)) ? 0.0 : (sb - sa) / m;  // ACAV_QUALITY_SUM_S
            rv[5 * QM + t] = b < a ? 1.0 : 0.0;                        // ACAV_QUALITY_DISPLACED
            rv[6 * QM + t] = b < a ? b : a;                            // ACAV_QUALITY_SUM_MIN
        }
        __syncthreads();
        if (t < QC) {  // lane t owns column t of every cluster's sums: the tile's rows in row order
            const int rows = n - row0 < QM ? (int)(n - row0) : QM;
            for (int i = 0; i < rows; ++i) {
                double *s = sums + (size_t)labs[i] * QC + t;
                *s = *s + (t == 0 ? 1.0 : rv[(t + 1) * QM + i]);
            }
        }
        __syncthreads();  // labs and rv are free for the next tile
    }
    __syncthreads();
    for (int i = t; i < K * QC; i += 256) partials[(size_t)blockIdx.x * K * QC + i] = sums[i];
}

__global__ __launch_bounds__(256) void k_quality_fold(const double *__restrict__ partials, int nparts, int len, double *__restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    double s = 0.0;
    for (int p = 0; p < nparts; ++p) s = s + partials[(size_t)p * len + i];
    out[i] = s;
}

// ---- acav_kmeans_probes: the m nearest centres of a row (KMeans.probe_centers; the multi-probe dedup of clustering/dedup.py)
//
// k_quality's stages, operands, accumulators and distance expression -- D_ik has the bytes of k_quality's -- but what leaves a
// pass of 64 centres is the whole [64 rows][64 centres] tile of distances, into LDS, where one thread per row walks its
// centres in ascending index and keeps the m - 1 smallest among the centres other than the row's label in a sorted list
// (insertion with a strict <: of two equal distances the lower index stays in front).  The list is a function of the row's
// distances alone, the distances of the row and the centres alone: not of the tile, the launch or the call.
constexpr int PM = ACAV_PROBES_MAX;
constexpr int QDS = QN + 1;  // f64 distance tile, row stride: the walk's lanes (one row each) fall into different bank pairs

constexpr size_t probes_lds()
{
    // the centre stage, the distance tile, the lists' distances, ||x||^2; the row stage; the lists' centres
    return sizeof(double) * ((size_t)QN * QCS + (size_t)QM * QDS + (size_t)PM * QM + QM) + sizeof(float) * QM * QXS +
           sizeof(int) * PM * QM;
}
static_assert(2 * probes_lds() <= 160 * 1024, "two workgroups share a compute unit's LDS");

// the launch shape of k_probes, a function of (n, cus) alone: two workgroups per CU, each taking the row tiles b, b + grid, ...
QualityPlan probes_plan(int64_t n, int cus)
{
    QualityPlan p;
    p.ntiles = (n + QM - 1) / QM;
    p.lds = probes_lds();
    p.per_cu = 2;
    p.grid = (int)std::min<int64_t>(p.ntiles, (int64_t)cus * p.per_cu);
    return p;
}

__global__ __launch_bounds__(256, 2) void k_probes(const float *__restrict__ x, int64_t n, int d, const double *__restrict__ cd,
                                                   const double *__restrict__ cn, int K, const int64_t *__restrict__ labels, int m,
                                                   int64_t *__restrict__ probes, double *__restrict__ dist)
{
    extern __shared__ double q_smem[];
    double *cs = q_smem;                          // [QN][QCS]
    double *dt = cs + QN * QCS;                   // [QM][QDS]
    double *lv = dt + QM * QDS;                   // [PM][QM]: slot s of row t at s * QM + t
    double *rv = lv + PM * QM;                    // [QM]
    float *xs = reinterpret_cast<float *>(rv + QM);      // [QM][QXS]
    int *li = reinterpret_cast<int *>(xs + QM * QXS);    // [PM][QM]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;    // fragment row (A) / column (B) and k index of this lane
    const double inf = __builtin_inf();
    const int others = m - 1;                    // the list holds the others; slot 0 of the output is the label

    const int64_t ntiles = (n + QM - 1) / QM;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * QM;
        const bool walker = t < QM && row0 + t < n;
        const int my_lab = walker ? (int)labels[row0 + t] : -1;
        double own = inf;  // D(row, its label)
        int cnt = 0;       // entries of this row's list
        double xn[4] = {0.0, 0.0, 0.0, 0.0};
        double xn_part = 0.0;
        for (int k0 = 0; k0 < K; k0 += QN) {
            f64x4 acc[4];
            for (int ct = 0; ct < 4; ++ct) acc[ct] = f64x4{0.0, 0.0, 0.0, 0.0};
            for (int j0 = 0; j0 < d; j0 += QD) {
                __syncthreads();  // the previous stage has been read, the previous pass's distance tile walked
                for (int i = t; i < QM * QD; i += 256) {
                    const int r = i >> 5, c = i & 31;
                    const bool ok = row0 + r < n && j0 + c < d;
                    xs[r * QXS + c] = ok ? x[(size_t)(row0 + r) * d + j0 + c] : 0.f;
                }
                for (int i = t; i < QN * QD; i += 256) {
                    const int r = i >> 5, c = i & 31;
                    const bool ok = k0 + r < K && j0 + c < d;
                    cs[r * QCS + c] = ok ? cd[(size_t)(k0 + r) * d + j0 + c] : 0.0;
                }
                __syncthreads();
#pragma unroll
                for (int kk = 0; kk < QD / 4; ++kk) {
                    const double a = (double)xs[(wave * 16 + fr) * QXS + kk * 4 + fq];
                    if (k0 == 0) xn_part = fma(a, a, xn_part);
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) {
                        const double b = cs[(ct * 16 + fr) * QCS + kk * 4 + fq];
                        acc[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[ct], 0, 0, 0);
                    }
                }
            }
            if (k0 == 0) {  // ||x||^2 of the wave's 16 rows, k_quality's: (p0 + p1) + (p2 + p3)
                double v = xn_part + __shfl_xor(xn_part, 16);
                v = v + __shfl_xor(v, 32);
                if (fq == 0) rv[wave * 16 + fr] = v;
                __syncthreads();
                for (int r = 0; r < 4; ++r) xn[r] = rv[wave * 16 + fq + 4 * r];
            }
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int k = k0 + ct * 16 + fr;
                const double ck = cn[k < K ? k : K - 1];
#pragma unroll
                for (int r = 0; r < 4; ++r) {  // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
                    double v = (xn[r] + ck) - 2.0 * acc[ct][r];
                    v = v < 0.0 ? 0.0 : v;
                    dt[(wave * 16 + fq + 4 * r) * QDS + ct * 16 + fr] = v;
                }
            }
            __syncthreads();
            if (walker) {
                const int cols = K - k0 < QN ? K - k0 : QN;
                const double *mine = dt + t * QDS;
                for (int c = 0; c < cols; ++c) {
                    const double v = mine[c];
                    if (k0 + c == my_lab) {
                        own = v;
                        continue;
                    }
                    if (others == 0 || (cnt == others && !(v < lv[(others - 1) * QM + t]))) continue;
                    int s = cnt < others ? cnt : others - 1;  // a full list drops its last entry
                    for (; s > 0 && v < lv[(s - 1) * QM + t]; --s) {
                        lv[s * QM + t] = lv[(s - 1) * QM + t];
                        li[s * QM + t] = li[(s - 1) * QM + t];
                    }
                    lv[s * QM + t] = v;
                    li[s * QM + t] = k0 + c;
                    cnt += cnt < others ? 1 : 0;
                }
            }
        }
        if (walker) {
            const size_t o = (size_t)(row0 + t) * m;
            probes[o] = my_lab;
            if (dist) dist[o] = own;
            for (int s = 0; s < others; ++s) {
                probes[o + 1 + s] = s < cnt ? (int64_t)li[s * QM + t] : (int64_t)-1;
                if (dist) dist[o + 1 + s] = s < cnt ? lv[s * QM + t] : inf;
            }
        }
    }
}

}  // namespace

ACAV_EXPORT int acav_kmeans_quality_plan(int64_t n, int k, int cus, int64_t *out)
{
    ACAV_REQUIRE(out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < ((int64_t)1 << 37) && k > 0 && k <= QUALITY_MAX_K && cus > 0, ACAV_EINVAL, "bad sizes");
    const QualityPlan p = quality_plan(n, k, cus);
    out[0] = p.ntiles, out[1] = p.grid, out[2] = (int64_t)p.lds, out[3] = p.per_cu;
    return ACAV_OK;
}

ACAV_EXPORT int acav_kmeans_quality(acav_kmeans *km, const float *x, int64_t n, const int64_t *labels, double *cluster_stats,
                                    double *row_stats)
{
    ACAV_REQUIRE(km, ACAV_EINVAL, "handle is NULL");
    ACAV_REQUIRE(n >= 0 && n < ((int64_t)1 << 37), ACAV_EINVAL, "n must be in [0, 2^37)");
    ACAV_REQUIRE(cluster_stats && (n == 0 || (x && labels)), ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(!is_device_ptr(cluster_stats), ACAV_EINVAL, "cluster_stats is a host array");
    ACAV_REQUIRE(km->K <= QUALITY_MAX_K, ACAV_EUNSUPPORTED, "k=%d: the per-cluster sums of acav_kmeans_quality are kept for k <= %d",
                 km->K, QUALITY_MAX_K);
    ACAV_REQUIRE(!km->warm(), ACAV_ESTATE,
                 "count=%lld < initial_rounds*k=%lld: the labels of the warm-up are random draws, their distances say nothing",
                 (long long)km->count, (long long)km->initial_rounds * km->K);
    const int K = km->K, d = km->d, len = K * QC;
    memset(cluster_stats, 0, sizeof(double) * (size_t)len);
    if (n == 0) return ACAV_OK;
    ACAV_HIP_TRY(hipSetDevice(km->ctx.device));
    hipStream_t st = km->ctx.stream;
    int cus = 0;
    ACAV_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, km->ctx.device));

    // scratch of this call only (parked blocks of the library's pool): the handle keeps nothing of it
    DevBuf stage_x, stage_lab, bad, cd, cn, parts, out, rows;
    StreamDrain drain = {st};
    const void *dx = nullptr, *dl = nullptr;
    ACAV_TRY(to_device(x, sizeof(float) * (size_t)n * d, stage_x, st, &dx));
    ACAV_TRY(to_device(labels, sizeof(int64_t) * (size_t)n, stage_lab, st, &dl));
    ACAV_TRY(bad.ensure(sizeof(unsigned)));
    ACAV_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_quality_labels, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                       static_cast<const int64_t *>(dl), n, K, bad.as<unsigned>());
    ACAV_HIP_TRY(hipGetLastError());
    unsigned nbad = 0;
    ACAV_HIP_TRY(hipMemcpyAsync(&nbad, bad.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(nbad == 0, ACAV_EINVAL, "%u of %lld labels are outside [0, %d)", nbad, (long long)n, K);

    const QualityPlan plan = quality_plan(n, K, cus);
    const int grid = plan.grid;
    const bool rows_dev = row_stats && is_device_ptr(row_stats);
    ACAV_TRY(cd.ensure(sizeof(double) * (size_t)K * d));
    ACAV_TRY(cn.ensure(sizeof(double) * (size_t)K));
    ACAV_TRY(parts.ensure(sizeof(double) * (size_t)grid * len));
    ACAV_TRY(out.ensure(sizeof(double) * (size_t)len));
    if (row_stats && !rows_dev) ACAV_TRY(rows.ensure(sizeof(double) * (size_t)n * 2));
    double *drows = !row_stats ? (double *)nullptr : rows_dev ? row_stats : rows.as<double>();
    // the largest K's size, whatever this call's: a second handle's call on another thread never lowers it under a pending launch
    ACAV_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_quality), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)quality_lds(QUALITY_MAX_K)));

    hipLaunchKernelGGL(k_quality_centres, dim3((unsigned)K), dim3(64), 0, st, km->centers.as<float>(), d, cd.as<double>(), cn.as<double>());
    hipLaunchKernelGGL(k_quality, dim3((unsigned)grid), dim3(256), plan.lds, st, static_cast<const float *>(dx), n, d, cd.as<double>(),
                       cn.as<double>(), K, static_cast<const int64_t *>(dl), drows, parts.as<double>());
    hipLaunchKernelGGL(k_quality_fold, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, st, parts.as<double>(), grid, len, out.as<double>());
    ACAV_HIP_TRY(hipGetLastError());
    ACAV_HIP_TRY(hipMemcpyAsync(cluster_stats, out.p, sizeof(double) * (size_t)len, hipMemcpyDeviceToHost, st));
    if (row_stats && !rows_dev)
        ACAV_HIP_TRY(hipMemcpyAsync(row_stats, rows.p, sizeof(double) * (size_t)n * 2, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}

ACAV_EXPORT int acav_kmeans_probes_plan(int64_t n, int k, int cus, int64_t *out)
{
    ACAV_REQUIRE(out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < ((int64_t)1 << 37) && k > 0 && k <= QUALITY_MAX_K && cus > 0, ACAV_EINVAL, "bad sizes");
    const QualityPlan p = probes_plan(n, cus);
    out[0] = p.ntiles, out[1] = p.grid, out[2] = (int64_t)p.lds, out[3] = p.per_cu;
    return ACAV_OK;
}

ACAV_EXPORT int acav_kmeans_probes(acav_kmeans *km, const float *x, int64_t n, const int64_t *labels, int m, int64_t *probes,
                                   double *dist)
{
    ACAV_REQUIRE(km, ACAV_EINVAL, "handle is NULL");
    ACAV_REQUIRE(n >= 0 && n < ((int64_t)1 << 37), ACAV_EINVAL, "n must be in [0, 2^37)");
    ACAV_REQUIRE(m >= 1 && m <= PM, ACAV_EINVAL, "m=%d must be in [1, %d]", m, PM);
    ACAV_REQUIRE(n == 0 || (x && labels && probes), ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(km->K <= QUALITY_MAX_K, ACAV_EUNSUPPORTED, "k=%d: acav_kmeans_probes keeps acav_kmeans_quality's limit, k <= %d", km->K,
                 QUALITY_MAX_K);
    ACAV_REQUIRE(!km->warm(), ACAV_ESTATE,
                 "count=%lld < initial_rounds*k=%lld: the labels of the warm-up are random draws, their distances say nothing",
                 (long long)km->count, (long long)km->initial_rounds * km->K);
    if (n == 0) return ACAV_OK;
    const int K = km->K, d = km->d;
    ACAV_HIP_TRY(hipSetDevice(km->ctx.device));
    hipStream_t st = km->ctx.stream;
    int cus = 0;
    ACAV_HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, km->ctx.device));

    DevBuf stage_x, stage_lab, bad, cd, cn, oprobes, odist;
    StreamDrain drain = {st};
    const void *dx = nullptr, *dl = nullptr;
    ACAV_TRY(to_device(x, sizeof(float) * (size_t)n * d, stage_x, st, &dx));
    ACAV_TRY(to_device(labels, sizeof(int64_t) * (size_t)n, stage_lab, st, &dl));
    ACAV_TRY(bad.ensure(sizeof(unsigned)));
    ACAV_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_quality_labels, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                       static_cast<const int64_t *>(dl), n, K, bad.as<unsigned>());
    ACAV_HIP_TRY(hipGetLastError());
    unsigned nbad = 0;
    ACAV_HIP_TRY(hipMemcpyAsync(&nbad, bad.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(nbad == 0, ACAV_EINVAL, "%u of %lld labels are outside [0, %d)", nbad, (long long)n, K);

    const QualityPlan plan = probes_plan(n, cus);
    const size_t cells = (size_t)n * m;
    const bool probes_dev = is_device_ptr(probes), dist_dev = dist && is_device_ptr(dist);
    ACAV_TRY(cd.ensure(sizeof(double) * (size_t)K * d));
    ACAV_TRY(cn.ensure(sizeof(double) * (size_t)K));
    if (!probes_dev) ACAV_TRY(oprobes.ensure(sizeof(int64_t) * cells));
    if (dist && !dist_dev) ACAV_TRY(odist.ensure(sizeof(double) * cells));
    int64_t *dprobes = probes_dev ? probes : oprobes.as<int64_t>();
    double *ddist = !dist ? (double *)nullptr : dist_dev ? dist : odist.as<double>();
    ACAV_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_probes), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)probes_lds()));

    hipLaunchKernelGGL(k_quality_centres, dim3((unsigned)K), dim3(64), 0, st, km->centers.as<float>(), d, cd.as<double>(), cn.as<double>());
    hipLaunchKernelGGL(k_probes, dim3((unsigned)plan.grid), dim3(256), plan.lds, st, static_cast<const float *>(dx), n, d, cd.as<double>(),
                       cn.as<double>(), K, static_cast<const int64_t *>(dl), m, dprobes, ddist);
    ACAV_HIP_TRY(hipGetLastError());
    if (!probes_dev) ACAV_HIP_TRY(hipMemcpyAsync(probes, oprobes.p, sizeof(int64_t) * cells, hipMemcpyDeviceToHost, st));
    if (dist && !dist_dev) ACAV_HIP_TRY(hipMemcpyAsync(dist, odist.p, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}
