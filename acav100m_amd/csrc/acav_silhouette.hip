// acav_silhouette.hip -- the exact silhouette of labelled rows (acav_rows_silhouette; clustering/silhouette.py, `evaluate
// --evaluate.silhouette_sample`): sklearn.metrics.silhouette_samples on a sample, every pairwise distance of it in float64.
// No counterpart in the reference.  acav_kmeans_quality is rows against K centres; this is rows against rows.
//
// Arithmetic.  Everything is float64 on the stored fp32 values: dist(i, j) = sqrt(max(0, (||x_i||^2 + ||x_j||^2) - 2 x_i.x_j)),
// x_i.x_j one chain of v_mfma_f64_16x16x4_f64 over the columns 0, 4, 8, ... from a zero accumulator (tails in d are zero-filled
// when a stage is loaded: they add exactly 0), ||x||^2 one wave per row: lane l chains fma(v, v, .) over its columns l, l + 64,
// ... from +0, the 64 lane values are summed by an xor-butterfly, v[l] + v[l ^ o] for o = 32 ... 1.  The rows are widened in
// registers on their way from the fp32 LDS stages into the operands.
//
// Label-sorted columns.  The entry sorts the sample positions by label, stably (the permutation of a stable counting sort: inside
// a cluster the rows keep ascending sample position; built on the host by a stable merge sort of the positions, M log M against
// the M^2 d of the sweep, and with no table of k entries: k is not limited).  The columns j are swept in that order, so a
// cluster is one contiguous RUN.  A query row keeps one running sum: it starts at +0 with a run's first column, takes
// sum <- sum + dist(i, j) for the run's columns in ascending sorted position -- ONE chain, carried across column blocks -- and
// is flushed at the run's end: into A_i = sum / (n - 1) if the run is the row's own cluster (0 when n = 1), otherwise
// B_i <- min(B_i, sum / n).  The column j == i is skipped by its position: its value is never added.  No [M][K] table, no
// floating-point atomics.
//
// Tiling.  One workgroup (4 waves) owns a tile of SIL_QM = 64 RT query rows (RT = 1 or 2 by the plan) and walks all column
// blocks of SIL_CN = 64 columns itself.  Query tile and column block are both staged through LDS as fp32 in chunks of
// SIL_DK = 32 columns of d (the next chunk is in flight in registers while the current one is multiplied); a wave holds the
// 4 RT accumulators of its 16 RT rows x 64 columns.  After the last chunk the block's distances go to LDS (over the stages) and
// one thread per query row walks its 64 columns in order.
//
// Invariance.  (A_i, B_i) is a pure function of the sample and the labels: the dot of a pair is the same chain wherever the pair
// sits in a tile, a run's sum is the chain above whatever the tile size, the workgroup, the query rows of the call
// (acav_rows_silhouette_range) or host / device / unaligned input (the guarded load path feeds the same values into the same
// chain).  The same call gives the same bytes every time.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "acav_common.h"

using namespace acav;

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int64_t SIL_MAX_M = ((int64_t)1 << 31) - 1;  // positions are 32-bit
constexpr int SIL_MAX_D = 16384;
constexpr int SIL_QM = 64;         // query rows of a tile per RT: 16 per wave
constexpr int SIL_CN = 64;         // columns of a block: four 16 x 16 accumulators per wave and RT
constexpr int SIL_DK = 32;         // columns of d of a stage
constexpr int SIL_ST = SIL_DK + 4; // fp32 stage, row stride: the 16 rows x 4 columns of a fragment fall into 64 different banks
constexpr int SIL_DS = SIL_CN + 1; // float64 distance tile, row stride: the walk's lanes (one row each) fall into different bank pairs

constexpr size_t silhouette_lds(int rt)
{
    // the distance tile lies over the two stages (which are dead by then); the block's run ids and run sizes follow it
    return std::max(sizeof(double) * (size_t)SIL_QM * rt * SIL_DS, sizeof(float) * (size_t)(SIL_QM * rt + SIL_CN) * SIL_ST) +
           sizeof(int) * 2 * SIL_CN;
}
static_assert(2 * silhouette_lds(2) <= 160 * 1024, "two workgroups of the larger tile share a compute unit's LDS");

// the launch shape, a function of (query rows, m, d, cus) alone: one workgroup per query tile.  128-row tiles (less operand
// traffic per multiply-add) once they alone give every compute unit a workgroup, 64-row tiles otherwise
struct SilPlan {
    int rt;
    int64_t tiles, blocks;
    int chunks;
    size_t lds, scratch;
};

SilPlan silhouette_plan(int64_t nq, int64_t m, int d, int cus)
{
    SilPlan p;
    p.rt = (nq + 2 * SIL_QM - 1) / (2 * SIL_QM) >= cus ? 2 : 1;
    p.tiles = (nq + (int64_t)SIL_QM * p.rt - 1) / ((int64_t)SIL_QM * p.rt);
    p.blocks = (m + SIL_CN - 1) / SIL_CN;
    p.chunks = (d + SIL_DK - 1) / SIL_DK;
    p.lds = silhouette_lds(p.rt);
    // the sorted positions, run ids and run sizes of the columns, the query positions and their output rows, the norms, (A, B)
    p.scratch = sizeof(int) * 3 * (size_t)m + sizeof(int) * 2 * (size_t)nq + sizeof(double) * (size_t)m + sizeof(double) * 2 * (size_t)nq;
    return p;
}

// labels outside [0, k): counted before anything is indexed with a label
__global__ __launch_bounds__(256) void k_sil_labels(const int64_t *__restrict__ labels, int64_t m, int k, unsigned *__restrict__ bad)
{
    unsigned mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256)
        mine += (labels[i] < 0 || labels[i] >= k) ? 1u : 0u;
    if (mine) atomicAdd(bad, mine);
}

// one wave per sorted position c: nrm[c] = ||x[perm[c]]||^2 (lane l: columns l, l + 64, ...; then a fixed tree)
__global__ __launch_bounds__(64) void k_sil_norms(const float *__restrict__ x, int d, const int *__restrict__ perm, double *__restrict__ nrm)
{
    const size_t base = (size_t)perm[blockIdx.x] * d;
    double p = 0.0;
    for (int j = threadIdx.x; j < d; j += 64) {
        const double v = (double)x[base + j];
        p = fma(v, v, p);
    }
    for (int o = 32; o >= 1; o >>= 1) p = p + __shfl_xor(p, o);
    if (threadIdx.x == 0) nrm[blockIdx.x] = p;
}

// columns j .. j + 3 of a row as they are stored; no branch: the load goes to a clamped address inside the row, sil_mask
// zeroes what was clamped
template <bool VEC>
__device__ __forceinline__ float4 sil_fetch(const float *__restrict__ r, int d, int j)
{
    if (VEC) return *reinterpret_cast<const float4 *>(r + min(j, d - 4));  // d % 4 == 0: j < d means j + 3 < d
    return make_float4(r[min(j, d - 1)], r[min(j + 1, d - 1)], r[min(j + 2, d - 1)], r[min(j + 3, d - 1)]);
}

__device__ __forceinline__ float4 sil_mask(float4 a, bool row_ok, int d, int j)
{
    float4 v;
    v.x = (row_ok && j < d) ? a.x : 0.f;
    v.y = (row_ok && j + 1 < d) ? a.y : 0.f;
    v.z = (row_ok && j + 2 < d) ? a.z : 0.f;
    v.w = (row_ok && j + 3 < d) ? a.w : 0.f;
    return v;
}

// perm[c]: the sample position of sorted position c; crun[c] / ccnt[c]: the run (0, 1, ... in sorted order) of column c and
// that run's size; nrm[c]: ||x||^2.  qpos[q]: the sorted position of query q, qout[q]: its row of `out` [nq][2] = (A, B)
template <int RT, bool VEC>
__global__ __launch_bounds__(256, 2) void k_silhouette(const float *__restrict__ x, int d, int m, const int *__restrict__ perm,
                                                       const int *__restrict__ crun, const int *__restrict__ ccnt,
                                                       const double *__restrict__ nrm, const int *__restrict__ qpos,
                                                       const int *__restrict__ qout, int nq, double *__restrict__ out)
{
    constexpr int QM = SIL_QM * RT;
    extern __shared__ double sil_smem[];
    double *dist = sil_smem;                                  // [QM][SIL_DS], after the last chunk of a block
    float *qs = reinterpret_cast<float *>(sil_smem);          // [QM][SIL_ST]
    float *cs = qs + QM * SIL_ST;                             // [SIL_CN][SIL_ST]
    constexpr size_t tile_bytes = sizeof(double) * QM * SIL_DS > sizeof(float) * (QM + SIL_CN) * SIL_ST
                                      ? sizeof(double) * QM * SIL_DS
                                      : sizeof(float) * (QM + SIL_CN) * SIL_ST;
    int *brun = reinterpret_cast<int *>(reinterpret_cast<char *>(sil_smem) + tile_bytes);  // [SIL_CN]
    int *bcnt = brun + SIL_CN;                                                             // [SIL_CN]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;  // fragment row (A) / column (B) and k index of this lane
    const int lq = t & 7, lr = t >> 3;         // this thread stages columns 4 lq .. 4 lq + 3 of the rows lr + 32 u
    const int q0 = blockIdx.x * QM;
    const double inf = __builtin_inf();

    // the query rows this thread stages, and the ones whose results it holds
    const float *qrow[2 * RT];
    bool qok[2 * RT];
#pragma unroll
    for (int u = 0; u < 2 * RT; ++u) {
        const int q = q0 + lr + 32 * u;
        qok[u] = q < nq;
        qrow[u] = x + (size_t)perm[qpos[qok[u] ? q : q0]] * d;
    }
    double qn[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
            const int q = q0 + wave * 16 * RT + rt * 16 + fq + 4 * r;
            qn[rt][r] = nrm[qpos[q < nq ? q : q0]];
        }
    // the walk: thread t < QM owns query row t of the tile
    const bool walker = t < QM && q0 + t < nq;
    const int my_pos = walker ? qpos[q0 + t] : -1;
    const int my_run = walker ? crun[my_pos] : -1;
    int cur_run = -1, cur_n = 0;
    double sum = 0.0, A = 0.0, B = inf;

    const int nblocks = (m + SIL_CN - 1) / SIL_CN;
    for (int cb = 0; cb < nblocks; ++cb) {
        const int c0 = cb * SIL_CN;
        const float *crow[2];
        bool cok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = c0 + lr + 32 * u;
            cok[u] = c < m;
            crow[u] = x + (size_t)perm[cok[u] ? c : c0] * d;
        }
        f64x4 acc[RT][4];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f64x4{0.0, 0.0, 0.0, 0.0};
        float4 pq[2 * RT], pc[2];  // the next chunk, in flight while the current one is multiplied
#pragma unroll
        for (int u = 0; u < 2 * RT; ++u) pq[u] = sil_fetch<VEC>(qrow[u], d, 4 * lq);
#pragma unroll
        for (int u = 0; u < 2; ++u) pc[u] = sil_fetch<VEC>(crow[u], d, 4 * lq);
        for (int j0 = 0; j0 < d; j0 += SIL_DK) {
            __syncthreads();  // the previous stage has been read (and the previous block's distance tile walked)
#pragma unroll
            for (int u = 0; u < 2 * RT; ++u)
                *reinterpret_cast<float4 *>(&qs[(lr + 32 * u) * SIL_ST + 4 * lq]) = sil_mask(pq[u], qok[u], d, j0 + 4 * lq);
#pragma unroll
            for (int u = 0; u < 2; ++u)
                *reinterpret_cast<float4 *>(&cs[(lr + 32 * u) * SIL_ST + 4 * lq]) = sil_mask(pc[u], cok[u], d, j0 + 4 * lq);
            if (j0 == 0 && t < SIL_CN) {
                const int c = c0 + t < m ? c0 + t : m - 1;
                brun[t] = crun[c];
                bcnt[t] = ccnt[c];
            }
            __syncthreads();
            if (j0 + SIL_DK < d) {
#pragma unroll
                for (int u = 0; u < 2 * RT; ++u) pq[u] = sil_fetch<VEC>(qrow[u], d, j0 + SIL_DK + 4 * lq);
#pragma unroll
                for (int u = 0; u < 2; ++u) pc[u] = sil_fetch<VEC>(crow[u], d, j0 + SIL_DK + 4 * lq);
            }
#pragma unroll
            for (int kk = 0; kk < SIL_DK / 4; ++kk) {
                double a[RT], b[4];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = (double)qs[(wave * 16 * RT + rt * 16 + fr) * SIL_ST + kk * 4 + fq];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) b[ct] = (double)cs[(ct * 16 + fr) * SIL_ST + kk * 4 + fq];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt], b[ct], acc[rt][ct], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave has read the last stage: the distance tile goes over it
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int c = c0 + ct * 16 + fr;
            const double cn = nrm[c < m ? c : m - 1];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double d2 = (qn[rt][r] + cn) - 2.0 * acc[rt][ct][r];
                    d2 = d2 < 0.0 ? 0.0 : d2;
                    dist[(wave * 16 * RT + rt * 16 + fq + 4 * r) * SIL_DS + ct * 16 + fr] = sqrt(d2);
                }
        }
        __syncthreads();
        if (walker) {
            const int cols = m - c0 < SIL_CN ? m - c0 : SIL_CN;
            const double *mine = dist + t * SIL_DS;
            for (int c = 0; c < cols; ++c) {
                const int run = brun[c];
                if (run != cur_run) {  // the previous run has ended: flush it
                    if (cur_run >= 0) {
                        if (cur_run == my_run) {
                            A = cur_n > 1 ? sum / (double)(cur_n - 1) : 0.0;
                        } else {
                            const double v = sum / (double)cur_n;
                            B = v < B ? v : B;
                        }
                    }
                    cur_run = run, cur_n = bcnt[c], sum = 0.0;
                }
                if (c0 + c != my_pos) sum = sum + mine[c];  // j == i is skipped by position
            }
        }
    }
    if (walker) {
        if (cur_run == my_run) {
            A = cur_n > 1 ? sum / (double)(cur_n - 1) : 0.0;
        } else {
            const double v = sum / (double)cur_n;
            B = v < B ? v : B;
        }
        const size_t o = (size_t)qout[q0 + t] * 2;
        out[o] = A;
        out[o + 1] = B;
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

template <int RT>
int launch(const SilPlan &plan, bool vec, hipStream_t st, const float *x, int d, int m, const int *perm, const int *crun,
           const int *ccnt, const double *nrm, const int *qpos, const int *qout, int nq, double *out)
{
    // the larger tile's size, whatever this call's: another thread's call never lowers it under a pending launch
    const void *fn = vec ? reinterpret_cast<const void *>(k_silhouette<RT, true>) : reinterpret_cast<const void *>(k_silhouette<RT, false>);
    ACAV_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)silhouette_lds(RT)));
    if (vec)
        hipLaunchKernelGGL((k_silhouette<RT, true>), dim3((unsigned)plan.tiles), dim3(256), plan.lds, st, x, d, m, perm, crun, ccnt,
                           nrm, qpos, qout, nq, out);
    else
        hipLaunchKernelGGL((k_silhouette<RT, false>), dim3((unsigned)plan.tiles), dim3(256), plan.lds, st, x, d, m, perm, crun, ccnt,
                           nrm, qpos, qout, nq, out);
    ACAV_HIP_TRY(hipGetLastError());
    return ACAV_OK;
}

}  // namespace

ACAV_EXPORT int acav_rows_silhouette_plan(int64_t m, int d, int k, int cus, int64_t *out)
{
    ACAV_REQUIRE(out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(m >= 2 && m <= SIL_MAX_M && d >= 1 && d <= SIL_MAX_D && k >= 1 && cus > 0, ACAV_EINVAL, "bad sizes");
    const SilPlan p = silhouette_plan(m, m, d, cus);
    out[0] = (int64_t)SIL_QM * p.rt, out[1] = SIL_CN, out[2] = SIL_DK, out[3] = p.tiles, out[4] = p.blocks, out[5] = p.chunks;
    out[6] = 4 * p.rt, out[7] = (int64_t)p.lds, out[8] = (int64_t)p.scratch;
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_silhouette_range(int device, const float *x, int64_t m, int d, const int64_t *labels, int k, int64_t q0,
                                           int64_t q1, double *row_stats, void *stream)
{
    ACAV_REQUIRE(x && labels && row_stats, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(m >= 2 && m <= SIL_MAX_M, ACAV_EINVAL, "m=%lld must be in [2, 2^31): a silhouette needs two rows, positions are 32-bit",
                 (long long)m);
    ACAV_REQUIRE(d >= 1 && d <= SIL_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, SIL_MAX_D);
    ACAV_REQUIRE(k >= 1, ACAV_EINVAL, "k=%d must be at least 1", k);
    ACAV_REQUIRE(q0 >= 0 && q0 < q1 && q1 <= m, ACAV_EINVAL, "query rows [%lld, %lld) must be a non-empty part of [0, %lld)",
                 (long long)q0, (long long)q1, (long long)m);
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);

    DevBuf stage_x, stage_lab, bad, ints, nrm, rows;
    StreamDrain drain = {st};
    const void *dx = nullptr, *dl = nullptr;
    ACAV_TRY(to_device(x, sizeof(float) * (size_t)m * d, stage_x, st, &dx));
    ACAV_TRY(to_device(labels, sizeof(int64_t) * (size_t)m, stage_lab, st, &dl));
    ACAV_TRY(bad.ensure(sizeof(unsigned)));
    ACAV_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL(k_sil_labels, dim3((unsigned)std::min<int64_t>((m + 255) / 256, 4096)), dim3(256), 0, st,
                       static_cast<const int64_t *>(dl), m, k, bad.as<unsigned>());
    ACAV_HIP_TRY(hipGetLastError());
    unsigned nbad = 0;
    std::vector<int64_t> lab((size_t)m);
    ACAV_HIP_TRY(hipMemcpyAsync(&nbad, bad.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipMemcpyAsync(lab.data(), dl, sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(nbad == 0, ACAV_EINVAL, "%u of %lld labels are outside [0, %d)", nbad, (long long)m, k);

    // the sample positions by label, stably; then per sorted position its run and the run's size, and the queries of the call
    const int64_t nq = q1 - q0;
    std::vector<int> host((size_t)(3 * m + 2 * nq));
    int *perm = host.data(), *crun = perm + m, *ccnt = crun + m, *qpos = ccnt + m, *qout = qpos + nq;
    std::iota(perm, perm + m, 0);
    std::stable_sort(perm, perm + m, [&](int a, int b) { return lab[(size_t)a] < lab[(size_t)b]; });
    int run = -1;
    for (int64_t c = 0, first = 0; c < m; ++c) {
        if (c == 0 || lab[(size_t)perm[c]] != lab[(size_t)perm[c - 1]]) ++run, first = c;
        crun[c] = run;
        if (c + 1 == m || lab[(size_t)perm[c + 1]] != lab[(size_t)perm[c]])
            for (int64_t e = first; e <= c; ++e) ccnt[e] = (int)(c - first + 1);
    }
    int64_t q = 0;
    for (int64_t c = 0; c < m; ++c)
        if (perm[c] >= q0 && perm[c] < q1) qpos[q] = (int)c, qout[q] = (int)(perm[c] - q0), ++q;

    const SilPlan plan = silhouette_plan(nq, m, d, cus);
    const bool rows_dev = is_device_ptr(row_stats);
    ACAV_TRY(upload(ints, host.data(), sizeof(int) * host.size(), st));
    ACAV_TRY(nrm.ensure(sizeof(double) * (size_t)m));
    if (!rows_dev) ACAV_TRY(rows.ensure(sizeof(double) * 2 * (size_t)nq));
    double *drows = rows_dev ? row_stats : rows.as<double>();
    const float *xd = static_cast<const float *>(dx);
    const int *dperm = ints.as<int>(), *dcrun = dperm + m, *dccnt = dcrun + m, *dqpos = dccnt + m, *dqout = dqpos + nq;
    const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(xd) & 15) == 0;
    hipLaunchKernelGGL(k_sil_norms, dim3((unsigned)m), dim3(64), 0, st, xd, d, dperm, nrm.as<double>());
    if (plan.rt == 2)
        ACAV_TRY(launch<2>(plan, vec, st, xd, d, (int)m, dperm, dcrun, dccnt, nrm.as<double>(), dqpos, dqout, (int)nq, drows));
    else
        ACAV_TRY(launch<1>(plan, vec, st, xd, d, (int)m, dperm, dcrun, dccnt, nrm.as<double>(), dqpos, dqout, (int)nq, drows));
    if (!rows_dev) ACAV_HIP_TRY(hipMemcpyAsync(row_stats, rows.p, sizeof(double) * 2 * (size_t)nq, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_silhouette(int device, const float *x, int64_t m, int d, const int64_t *labels, int k, double *row_stats,
                                     void *stream)
{
    return acav_rows_silhouette_range(device, x, m, d, labels, k, 0, m, row_stats, stream);
}
