// acav_score.hip -- how well the clusterings agree on a GIVEN subset: sklearn's mutual_info / normalized_mutual_info /
// adjusted_mutual_info / adjusted_rand / fowlkes_mallows / rand scores of every clustering pair's two label columns
// restricted to an id list (MutualInformation.get_measure, correspondence_retrieval/code/measures/mutual_information.py:
// 11-17,74-85).  The definition is written out in include/acav_hip.h ("subset scoring").
//
// Pipeline of one prefix of the id list, all on the handle's stream, no host round trip in between:
//   k_score_build_lds / _global   ids of the new slice -> += the call's own int32 tables N[P][C][C]   (integer atomics)
//   k_score_rows, k_score_cols    marginals b (rows) and a (columns) from the finished table
//   k_score_cells                 per workgroup of CELL_CHUNK cells: partial MI sum and partial sum C(N,2)
//   k_score_emi                   (adjusted_mutual_info only) per (row, pair, slice): partial exact EMI
//   k_score_finish                per pair: partials in fixed order, entropies, sum C(a,2), sum C(b,2) -> PairRaw
// Determinism: the tables are integer counts (any order of the ids gives the same cells); every double is a sum whose shape
// depends on (C, P, n) alone -- a thread adds its items in ascending order, a workgroup adds its threads by a fixed tree, the
// last pass adds the workgroups' partials the same way.  No float atomics anywhere.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>

#include "acav_score.h"

using namespace acav;

namespace {

constexpr int CELL_CHUNK = 4096;             // cells of one k_score_cells workgroup
constexpr size_t LDS_TABLE_MAX = 80 * 1024;  // half of a CU's 160 KB: two table-building workgroups per CU
constexpr int BUILD_IDS_PER_WG = 8192;       // ids one LDS-counting workgroup takes at least (amortises zero + flush of the table)

struct PairRaw {  // one pair's raw values as the device leaves them
    double mi, h_row, h_col, emi;
    long long tab, ta, tb;  // sum C(N,2), sum C(a,2), sum C(b,2)
    int n_rows, n_cols;
};

// sum over the workgroup's 256 threads by a fixed tree; every thread gets the result
template <class T>
__device__ __forceinline__ T block_sum(T v, T *sh)
{
    const int t = threadIdx.x;
    __syncthreads();  // sh may still be read from a previous sum
    sh[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sh[t] += sh[t + s];
        __syncthreads();
    }
    return sh[0];
}

// ---- tables ---------------------------------------------------------------------------------------------------------------------
// workgroup (slice x, pair y): counts its ids [i0 + x per, ...) in an LDS table, then adds the non-zero cells to the global one
__global__ __launch_bounds__(256) void k_score_build_lds(const int *__restrict__ asg, int D, int C, const int *__restrict__ pairs,
                                                         const int *__restrict__ ids, long long i0, long long i1, long long per,
                                                         int *__restrict__ N)
{
    extern __shared__ int tab[];
    const int p = blockIdx.y, cc = C * C;
    for (int c = threadIdx.x; c < cc; c += 256) tab[c] = 0;
    __syncthreads();
    const int d1 = pairs[2 * p], d2 = pairs[2 * p + 1];
    const long long lo = i0 + (long long)blockIdx.x * per;
    const long long hi = lo + per < i1 ? lo + per : i1;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const size_t row = (size_t)ids[i] * (size_t)D;
        atomicAdd(&tab[asg[row + d1] * C + asg[row + d2]], 1);
    }
    __syncthreads();
    int *Np = N + (size_t)p * cc;
    for (int c = threadIdx.x; c < cc; c += 256) {
        const int v = tab[c];
        if (v) atomicAdd(&Np[c], v);
    }
}

// a table beyond the LDS share: one id per thread, straight into the global table
__global__ __launch_bounds__(256) void k_score_build_global(const int *__restrict__ asg, int D, int C, const int *__restrict__ pairs,
                                                            const int *__restrict__ ids, long long i0, long long i1,
                                                            int *__restrict__ N)
{
    const int p = blockIdx.y;
    const long long i = i0 + (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= i1) return;
    const size_t row = (size_t)ids[i] * (size_t)D;
    const int r = asg[row + pairs[2 * p]], c = asg[row + pairs[2 * p + 1]];
    atomicAdd(&N[((size_t)p * C + r) * C + c], 1);
}

// b[p][i] = sum_j N[p][i][j]: workgroup (row i, pair p)
__global__ __launch_bounds__(256) void k_score_rows(int C, const int *__restrict__ N, int *__restrict__ b)
{
    __shared__ int sh[256];
    const int i = blockIdx.x, p = blockIdx.y;
    const int *row = N + ((size_t)p * C + i) * C;
    int s = 0;
    for (int j = threadIdx.x; j < C; j += 256) s += row[j];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) b[(size_t)p * C + i] = s;
}

// a[p][j] = sum_i N[p][i][j]: one thread per column
__global__ __launch_bounds__(256) void k_score_cols(int C, const int *__restrict__ N, int *__restrict__ a)
{
    const int j = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
    if (j >= C) return;
    const int *Np = N + (size_t)p * C * C;
    int s = 0;
    for (int i = 0; i < C; ++i) s += Np[(size_t)i * C + j];
    a[(size_t)p * C + j] = s;
}

// ---- per-pair sums --------------------------------------------------------------------------------------------------------------
// workgroup (chunk x, pair y): the MI terms and C(N,2) of cells [x CELL_CHUNK, (x+1) CELL_CHUNK) -> one partial each
__global__ __launch_bounds__(256) void k_score_cells(int C, long long n, const int *__restrict__ N, const int *__restrict__ a,
                                                     const int *__restrict__ b, const double *__restrict__ lnk,
                                                     double *__restrict__ part_mi, long long *__restrict__ part_tab)
{
    __shared__ double shd[256];
    __shared__ long long shl[256];
    const int p = blockIdx.y, nb = gridDim.x;
    const long long cc = (long long)C * C, base = (long long)blockIdx.x * CELL_CHUNK;
    const int *Np = N + (size_t)p * cc, *ap = a + (size_t)p * C, *bp = b + (size_t)p * C;
    const double ln_n = lnk[n], dn = (double)n;
    double s = 0.0;
    long long t = 0;
    for (int k = threadIdx.x; k < CELL_CHUNK; k += 256) {
        const long long c = base + k;
        if (c >= cc) break;
        const int v = Np[c];
        if (v > 0) {
            const int i = (int)(c / C), j = (int)(c - (long long)i * C);
            const double x = (double)v / dn;
            double term = x * (lnk[v] - ln_n) + x * ((-lnk[bp[i]] - lnk[ap[j]]) + 2.0 * ln_n);
            if (fabs(term) < DBL_EPSILON) term = 0.0;
            s += term;
            t += (long long)v * (v - 1) / 2;
        }
    }
    s = block_sum(s, shd);
    t = block_sum(t, shl);
    if (threadIdx.x == 0) {
        part_mi[(size_t)p * nb + blockIdx.x] = s;
        part_tab[(size_t)p * nb + blockIdx.x] = t;
    }
}

// exact expected mutual information: workgroup (row i, pair p, slice z of every cell's n_ij range).  `lpc` lanes share a column
// (256 / lpc columns at a time); lane l of them takes n_ij = lo + l, lo + l + lpc, ...  G is added up in sklearn's order
// (_expected_mutual_info_fast.pyx: rows first), so that on the same lf table it is the same number.
__global__ __launch_bounds__(256) void k_score_emi(int C, long long n, int lpc, const int *__restrict__ a, const int *__restrict__ b,
                                                   const double *__restrict__ lnk, const double *__restrict__ lf,
                                                   double *__restrict__ part)
{
    __shared__ double sh[256];
    const int i = blockIdx.x, p = blockIdx.y, z = blockIdx.z, Z = gridDim.z;
    const long long bi = b[(size_t)p * C + i];
    double s = 0.0;
    if (bi > 0) {  // (uniform over the workgroup)
        const int *ap = a + (size_t)p * C;
        const int group = threadIdx.x / lpc, lane = threadIdx.x % lpc, groups = 256 / lpc;
        const double ln_n = lnk[n], dn = (double)n, lfn = lf[n], lfb = lf[bi], lfnb = lf[n - bi], lnb = lnk[bi];
        for (int j = group; j < C; j += groups) {
            const long long aj = ap[j];
            if (aj == 0) continue;
            const long long start = aj + bi - n > 1 ? aj + bi - n : 1, end = aj < bi ? aj : bi;
            const long long chunk = (end - start + 1 + Z - 1) / Z;
            const long long lo = start + (long long)z * chunk;
            const long long hi = lo + chunk - 1 < end ? lo + chunk - 1 : end;
            const double g0 = (((lfb + lf[aj]) + lfnb) + lf[n - aj]) - lfn;
            const double lna = lnk[aj];
            for (long long nij = lo + lane; nij <= hi; nij += lpc) {
                const double G = (((g0 - lf[nij]) - lf[bi - nij]) - lf[aj - nij]) - lf[n - bi - aj + nij];
                const double t2 = ((ln_n + lnk[nij]) - lnb) - lna;
                s += (((double)nij / dn) * t2) * exp(G);
            }
        }
    }
    s = block_sum(s, sh);
    if (threadIdx.x == 0) part[((size_t)p * C + i) * Z + z] = s;
}

// workgroup p: the pair's partials and marginal sums -> out[p]
__global__ __launch_bounds__(256) void k_score_finish(int C, long long n, int nb, int emi_parts, const int *__restrict__ a,
                                                      const int *__restrict__ b, const double *__restrict__ lnk,
                                                      const double *__restrict__ part_mi, const long long *__restrict__ part_tab,
                                                      const double *__restrict__ part_emi, PairRaw *__restrict__ out)
{
    __shared__ double shd[256];
    __shared__ long long shl[256];
    const int p = blockIdx.x, t = threadIdx.x;
    const double ln_n = lnk[n], dn = (double)n;
    double mi = 0.0, emi = 0.0, hr = 0.0, hc = 0.0;
    long long tab = 0, ta = 0, tb = 0, nr = 0, nc = 0;
    for (int k = t; k < nb; k += 256) mi += part_mi[(size_t)p * nb + k], tab += part_tab[(size_t)p * nb + k];
    for (int k = t; k < emi_parts; k += 256) emi += part_emi[(size_t)p * emi_parts + k];
    for (int k = t; k < C; k += 256) {
        const long long m = b[(size_t)p * C + k];
        if (m > 0) hr += ((double)m / dn) * (lnk[m] - ln_n), tb += m * (m - 1) / 2, ++nr;
        const long long q = a[(size_t)p * C + k];
        if (q > 0) hc += ((double)q / dn) * (lnk[q] - ln_n), ta += q * (q - 1) / 2, ++nc;
    }
    mi = block_sum(mi, shd);
    emi = block_sum(emi, shd);
    hr = block_sum(hr, shd);
    hc = block_sum(hc, shd);
    tab = block_sum(tab, shl);
    ta = block_sum(ta, shl);
    tb = block_sum(tb, shl);
    nr = block_sum(nr, shl);
    nc = block_sum(nc, shl);
    if (t == 0) {
        PairRaw r;
        r.mi = mi < 0.0 ? 0.0 : mi;  // np.clip(mi.sum(), 0, None)
        r.h_row = -hr;
        r.h_col = -hc;
        r.emi = emi_parts ? emi : (double)NAN;
        r.tab = tab, r.ta = ta, r.tb = tb;
        r.n_rows = (int)nr, r.n_cols = (int)nc;
        out[p] = r;
    }
}

int floor_pow2(int x)
{
    int p = 1;
    while (2 * p <= x) p *= 2;
    return p;
}

// launch shapes of one prefix: functions of (C, P, n, m) alone -- n ids scored, the last m of them new to the tables
struct ScorePlan {
    bool lds;            // the table of a pair fits the LDS share (k_score_build_lds), else k_score_build_global
    int64_t slices, per; // table-building workgroups per pair and the ids each takes
    int nb;              // k_score_cells workgroups per pair
    int lpc;             // k_score_emi: lanes per column
    int64_t Z;           //              slices of every cell's n_ij range
    int emi_parts;       //              partials per pair (0: no EMI)
};

ScorePlan score_plan(int C, int P, int64_t n, int64_t m, bool want_emi)
{
    const size_t cc = (size_t)C * C;
    ScorePlan s = {};
    s.nb = (int)((cc + CELL_CHUNK - 1) / CELL_CHUNK);
    s.lds = cc * sizeof(int) <= LDS_TABLE_MAX;
    if (s.lds) {
        // enough slices to fill the device, none shorter than BUILD_IDS_PER_WG ids
        s.slices = (m + BUILD_IDS_PER_WG - 1) / BUILD_IDS_PER_WG;
        const int64_t cap = std::max<int64_t>(1, 2048 / P);
        s.slices = std::min(s.slices, cap);
        s.per = (m + s.slices - 1) / s.slices;
    } else {
        s.slices = (m + 255) / 256, s.per = 256;  // one id per thread
    }
    if (want_emi) {
        // lanes per column: 16 once there are 16 columns to spread a workgroup over, all 256 for a single column
        s.lpc = std::max(16, 256 / floor_pow2(C));
        // slices of every cell's n_ij range: few labels and many clips leave (row, pair) alone too coarse to fill the device
        s.Z = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(8192 / ((int64_t)P * C), n / (2 * s.lpc)), 1024));
        s.emi_parts = (int)(C * s.Z);
    }
    return s;
}

}  // namespace

// ---- host ------------------------------------------------------------------------------------------------------------------------
ACAV_EXPORT int acav_score_compose(const acav_score_stats *s, double *out)
{
    ACAV_REQUIRE(s && out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(s->n >= 1, ACAV_EINVAL, "a score needs at least one clip, got n = %lld", (long long)s->n);
    ACAV_REQUIRE(s->tp >= 0 && s->fp >= 0 && s->fn >= 0 && s->tn >= 0 && s->n_rows >= 0 && s->n_cols >= 0, ACAV_EINVAL,
                 "negative count in the pair's raw values");
    const double eps = DBL_EPSILON;  // 2^-52
    const bool one_label = s->n_rows == 1 && s->n_cols == 1;
    const double mean_h = (s->h_row + s->h_col) / 2.0;
    out[ACAV_SCORE_MUTUAL_INFO] = s->mi;
    out[ACAV_SCORE_NORMALIZED_MUTUAL_INFO] = one_label ? 1.0 : s->mi == 0.0 ? 0.0 : s->mi / (mean_h > eps ? mean_h : eps);
    if (one_label) {
        out[ACAV_SCORE_ADJUSTED_MUTUAL_INFO] = 1.0;
    } else if (s->n_rows == 1 || s->n_cols == 1) {
        out[ACAV_SCORE_ADJUSTED_MUTUAL_INFO] = std::isnan(s->emi) ? (double)NAN : 0.0;  // sklearn >= 1.6 returns 0 outright here (MI = EMI = 0)
    } else {
        double den = mean_h - s->emi, num = s->mi - s->emi;  // NaN stays NaN through both guards
        if (den < 0) den = den < -eps ? den : -eps;
        else if (den < eps) den = eps;
        if (num < 0) num = num < -eps ? num : -eps;          // sklearn guards the numerator the same way: a difference below 2^-52
        else if (num < eps) num = eps;                       // is rounding noise of two equal values
        out[ACAV_SCORE_ADJUSTED_MUTUAL_INFO] = num / den;
    }
    // sklearn's adjusted_rand_score works in Python ints: the products reach 2^122
    const __int128 tp = s->tp, fp = s->fp, fn = s->fn, tn = s->tn;
    if (s->fn == 0 && s->fp == 0) {
        out[ACAV_SCORE_ADJUSTED_RAND] = 1.0;
    } else {
        const __int128 num = tp * tn - fn * fp, den = (tp + fn) * (fn + tn) + (tp + fp) * (fp + tn);
        out[ACAV_SCORE_ADJUSTED_RAND] = 2.0 * (double)num / (double)den;
    }
    out[ACAV_SCORE_FOWLKES_MALLOWS] =
        s->tp == 0 ? 0.0 : sqrt((double)s->tp / (double)(s->tp + s->fp)) * sqrt((double)s->tp / (double)(s->tp + s->fn));
    const __int128 all = tp + fp + fn + tn;  // C(n,2)
    out[ACAV_SCORE_RAND] = all == 0 ? 1.0 : (double)(tp + tn) / (double)all;
    return ACAV_OK;
}

ACAV_EXPORT int acav_score_plan(int C, int P, int64_t n, int64_t m, int want_emi, int64_t *out)
{
    ACAV_REQUIRE(out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(C >= 1 && C <= 32768 && P >= 1 && P <= 65535 && n >= 1 && n < ((int64_t)1 << 31) && m >= 1 && m <= n, ACAV_EINVAL,
                 "bad sizes");
    const ScorePlan s = score_plan(C, P, n, m, want_emi != 0);
    const int64_t v[ACAV_SCORE_PLAN_LEN] = {s.lds ? 1 : 0, s.slices, s.per, s.nb, s.lpc, s.Z, s.emi_parts};
    for (int i = 0; i < ACAV_SCORE_PLAN_LEN; ++i) out[i] = v[i];
    return ACAV_OK;
}

int acav::score_subset_run(const ScoreJob &job)
{
    const int C = job.C, P = job.P;
    const size_t cc = (size_t)C * C, pc = (size_t)P * C;
    hipStream_t st = job.stream;
    const bool want_emi = (job.mask >> ACAV_SCORE_ADJUSTED_MUTUAL_INFO) & 1u;
    // launch shapes: functions of (C, P, n) alone; the path and the cell chunks are the same for every prefix
    const ScorePlan whole = score_plan(C, P, job.n, job.n, want_emi);
    const int nb = whole.nb;
    const bool lds = whole.lds;
    ACAV_REQUIRE(P <= 65535, ACAV_EINVAL, "subset scoring launches one workgroup row per pair: P = %d exceeds 65535", P);
    DevBuf N, a, b, part_mi, part_tab, part_emi, raw;
    std::vector<PairRaw> host((size_t)job.nprefix * P);
    // ACAV_SCORE_TIMING=1: the three phases of every prefix timed with events and printed to stderr (tools/bench_subset_scores.py)
    const bool timing = getenv("ACAV_SCORE_TIMING") != nullptr;
    hipEvent_t ev[4] = {};
    if (timing)
        for (auto &e : ev) ACAV_HIP_TRY(hipEventCreate(&e));
    auto enqueue = [&]() -> int {
    ACAV_TRY(N.ensure(sizeof(int) * cc * P));
    ACAV_TRY(a.ensure(sizeof(int) * pc));
    ACAV_TRY(b.ensure(sizeof(int) * pc));
    ACAV_TRY(part_mi.ensure(sizeof(double) * (size_t)nb * P));
    ACAV_TRY(part_tab.ensure(sizeof(long long) * (size_t)nb * P));
    ACAV_TRY(raw.ensure(sizeof(PairRaw) * (size_t)job.nprefix * P));
    ACAV_HIP_TRY(hipMemsetAsync(N.p, 0, sizeof(int) * cc * P, st));
    if (lds && cc * sizeof(int) > 48 * 1024)
        ACAV_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_score_build_lds), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(cc * sizeof(int))));
    int64_t done = 0;
    for (int q = 0; q < job.nprefix; ++q) {
        const int64_t n = job.prefix[q], m = n - done;
        if (timing) ACAV_HIP_TRY(hipEventRecord(ev[0], st));
        const ScorePlan plan = score_plan(C, P, n, m, want_emi);
        if (lds) {
            hipLaunchKernelGGL(k_score_build_lds, dim3((unsigned)plan.slices, (unsigned)P), dim3(256), cc * sizeof(int), st, job.asg, job.D, C,
                               job.pairs, job.ids, (long long)done, (long long)n, (long long)plan.per, N.as<int>());
        } else {
            hipLaunchKernelGGL(k_score_build_global, dim3((unsigned)plan.slices, (unsigned)P), dim3(256), 0, st, job.asg, job.D, C,
                               job.pairs, job.ids, (long long)done, (long long)n, N.as<int>());
        }
        ACAV_HIP_TRY(hipGetLastError());
        done = n;
        if (timing) ACAV_HIP_TRY(hipEventRecord(ev[1], st));
        hipLaunchKernelGGL(k_score_rows, dim3((unsigned)C, (unsigned)P), dim3(256), 0, st, C, N.as<int>(), b.as<int>());
        hipLaunchKernelGGL(k_score_cols, dim3((unsigned)((C + 255) / 256), (unsigned)P), dim3(256), 0, st, C, N.as<int>(), a.as<int>());
        hipLaunchKernelGGL(k_score_cells, dim3((unsigned)nb, (unsigned)P), dim3(256), 0, st, C, (long long)n, N.as<int>(), a.as<int>(),
                           b.as<int>(), job.lnk, part_mi.as<double>(), part_tab.as<long long>());
        ACAV_HIP_TRY(hipGetLastError());
        if (timing) ACAV_HIP_TRY(hipEventRecord(ev[2], st));
        const int emi_parts = plan.emi_parts;
        if (want_emi) {
            ACAV_TRY(part_emi.ensure(sizeof(double) * (size_t)emi_parts * P));
            hipLaunchKernelGGL(k_score_emi, dim3((unsigned)C, (unsigned)P, (unsigned)plan.Z), dim3(256), 0, st, C, (long long)n, plan.lpc, a.as<int>(),
                               b.as<int>(), job.lnk, job.lf, part_emi.as<double>());
            ACAV_HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(k_score_finish, dim3((unsigned)P), dim3(256), 0, st, C, (long long)n, nb, emi_parts, a.as<int>(), b.as<int>(),
                           job.lnk, part_mi.as<double>(), part_tab.as<long long>(), part_emi.as<double>(),
                           raw.as<PairRaw>() + (size_t)q * P);
        ACAV_HIP_TRY(hipGetLastError());
        if (timing) {  // (a synchronisation per prefix: measurements only)
            ACAV_HIP_TRY(hipEventRecord(ev[3], st));
            ACAV_HIP_TRY(hipEventSynchronize(ev[3]));
            float t_build = 0, t_sums = 0, t_emi = 0;
            ACAV_HIP_TRY(hipEventElapsedTime(&t_build, ev[0], ev[1]));
            ACAV_HIP_TRY(hipEventElapsedTime(&t_sums, ev[1], ev[2]));
            ACAV_HIP_TRY(hipEventElapsedTime(&t_emi, ev[2], ev[3]));
            fprintf(stderr, "acav_score: n=%lld C=%d P=%d ids=%lld table_%s_ms=%.3f marginals_cells_ms=%.3f emi_finish_ms=%.3f\n",
                    (long long)n, C, P, (long long)m, lds ? "lds" : "global", t_build, t_sums, t_emi);
        }
    }
    ACAV_HIP_TRY(hipMemcpyAsync(host.data(), raw.p, sizeof(PairRaw) * host.size(), hipMemcpyDeviceToHost, st));
    return ACAV_OK;
    };
    const int rc = enqueue();
    const hipError_t se = hipStreamSynchronize(st);  // the one synchronisation of the call; the scratch tables go after it, also when
    if (timing)
        for (auto &e : ev) (void)hipEventDestroy(e);
    ACAV_TRY(rc);                                    // enqueueing failed half-way
    ACAV_HIP_TRY(se);
    for (int q = 0; q < job.nprefix; ++q) {
        const int64_t n = job.prefix[q];
        double sum[ACAV_SCORE_COUNT] = {0, 0, 0, 0, 0, 0};
        for (int p = 0; p < P; ++p) {
            const PairRaw &r = host[(size_t)q * P + p];
            acav_score_stats s;
            s.mi = r.mi, s.h_row = r.h_row, s.h_col = r.h_col, s.emi = r.emi;
            s.tp = r.tab, s.fp = r.ta - r.tab, s.fn = r.tb - r.tab;
            s.tn = ((n * (n - 1) / 2 - r.ta) - r.tb) + r.tab;
            s.n_rows = r.n_rows, s.n_cols = r.n_cols, s.n = n;
            double sc[ACAV_SCORE_COUNT];
            ACAV_TRY(acav_score_compose(&s, sc));
            for (int k = 0; k < ACAV_SCORE_COUNT; ++k) {
                const bool on = (job.mask >> k) & 1u;
                if (!on) sc[k] = (double)NAN;
                sum[k] += sc[k];
                if (job.per_pair) job.per_pair[((size_t)q * ACAV_SCORE_COUNT + k) * P + p] = sc[k];
            }
            if (job.stats) job.stats[(size_t)q * P + p] = s;
        }
        for (int k = 0; k < ACAV_SCORE_COUNT; ++k) job.scores[(size_t)q * ACAV_SCORE_COUNT + k] = sum[k] / (double)P;
    }
    return ACAV_OK;
}
