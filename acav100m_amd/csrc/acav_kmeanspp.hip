// acav_kmeanspp.hip -- k-means++ (D^2) seeding for batch k-means (acav_kmeanspp_weights, acav_kmeanspp_seed;
// clustering/kmeanspp.py, clustering.init=kmeans++): K rows of a resident sample x [m, d], every next one drawn with a probability
// proportional to its squared distance to the nearest row chosen so far -- what scipy's kmeans2(minit='++') and sklearn's KMeans
// run; with T > 1 local trials per pick it is sklearn's greedy variant (the trial that lowers the potential most wins).
//
// Arithmetic.  The weight of row i against the sample row c with shift t:
//     e_j = double(x_ij) - double(x_cj),  p_j = e_j * e_j,  D = sum_j p_j,  W(i, c) = (int64) rint(D * 2^t)
// every operation one rounded float64 operation (no fma), rint = round half to even, the scaling exact.
// THE ORDER OF THE SUM, a function of d alone: with g(j) = j / 4 (the 16-byte group of column j), lane l = g(j) % 64 of a wave
// owns column j.  A lane chains the p_j of its columns from +0.0 in ascending j; the 64 lane values are then summed by an
// xor-butterfly, v[l] <- v[l] + v[l ^ o] for o = 32, 16, 8, 4, 2, 1 (IEEE addition commutes: all lanes end with the same bits).
// Columns past d are zero on both sides and add +0.0, which changes no bit.  One wave computes one row whatever m, the grid, the
// row's place or the pointer's alignment (rows off 16 bytes, or d % 4 != 0, take scalar loads into the same arithmetic).
// tests/_kmeanspp_np.py restates this order in numpy.  W(c, c) = 0 exactly: a chosen row, or a duplicate of it, has weight 0
// from then on and is never drawn again.
// Everything past W is integer: w_i = min over the chosen rows of W, totals, prefix sums, potentials.  The caller's shift keeps
// every sum of m weights below 2^62 (kmeanspp.weight_shift).  rows and potential are therefore a pure function of (x, k, T, u):
// not of the device, the grid or where x lives.  No floating-point atomics; the atomics here add integers.
//
// Schedule of one pick s (all on the stream; ONE device->host synchronisation per acav_kmeanspp_seed call, at its end):
//   k_kpp_sample   one workgroup.  total = sum of the per-block sums of w (blocks of KPP_BLOCK = 1024 rows); the T targets
//                  min(total - 1, (int64)(u * (double)total)) from the uploaded uniforms; a scan of the block sums finds each
//                  target's block, a scan of the block its row r_tau (the least i with w_0 + ... + w_i > target).
//                  total == 0 (fewer than k distinct rows) records s in a flag; the call then fails at its end.
//   k_kpp_sweep    the T candidate rows in LDS (fp32, zero-filled to a multiple of 256 columns); one wave per row, runs of 16
//                  consecutive rows per wave, 16-byte loads, up to four in flight per lane, T chains per lane; writes
//                  min(w_i, W(i, r_tau)) to a [T][m] scratch (coalesced, one store per run and trial) and adds the run's sum
//                  to the trial's per-block sums (64 integer adds per word; the sample kernel zeroed them).  When T * d floats
//                  exceed 64 KB of LDS the trials are split over several sweeps of floor(16384 / dpad) trials each -- same bits,
//                  the rows are then read once per sweep.
//   k_kpp_best     one workgroup: pot_tau = the sum of the trial's block sums; the trial of least potential (lowest tau on
//                  ties) gives rows[s] and potential[s].  (One word per trial that every wave of the sweep adds to costs more
//                  than the sweep: 4096 adds to one cache line take ~50 us.)
//   k_kpp_select   the best trial's column becomes w, its block sums the block sums.
#include <algorithm>
#include <cmath>
#include <vector>

#include "acav_common.h"

using namespace acav;

namespace {

constexpr int KPP_BLOCK = ACAV_KMEANSPP_BLOCK;  // rows of a block of the block sums
constexpr int KPP_RUN = 16;            // consecutive rows a wave takes at a time (KPP_BLOCK is a multiple)
constexpr int KPP_MAX_T = 16;
constexpr int KPP_MAX_D = 16384;
constexpr int KPP_LDS_FLOATS = 16384;  // 64 KB of candidate columns per sweep
constexpr int64_t KPP_MAX_M = (int64_t)1 << 31;
constexpr int KPP_MAX_SHIFT = 1000;    // |t|: 2^t stays a normal double
constexpr int KPP_PER_CU = 8;          // workgroups per compute unit the sweep's grid is capped at

static_assert(KPP_BLOCK % KPP_RUN == 0 && KPP_BLOCK == 4 * 256, "a run lies in one block; the sample kernel scans a block 4 rows per thread");

// inclusive scan of v over the 256 threads of the workgroup; *total = the sum.  sm: 4 words of LDS
__device__ __forceinline__ long long kpp_block_scan(long long v, long long *sm, long long *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const long long n = __shfl_up(v, o);
        if (lane >= o) v += n;
    }
    __syncthreads();  // (the previous call's readers of sm are done)
    if (lane == 63) sm[wave] = v;
    __syncthreads();
    long long before = 0;
    for (int q = 0; q < wave; ++q) before += sm[q];
    *total = sm[0] + sm[1] + sm[2] + sm[3];
    return v + before;
}

// One workgroup: the T candidate rows of pick s (s == 0: the one row min(m - 1, (int64)(u[0] * m))).
__global__ __launch_bounds__(256) void k_kpp_sample(const long long *__restrict__ w, const long long *__restrict__ bs, long long m, int nb,
                                                    const double *__restrict__ u, int s, int T, long long *__restrict__ cand_rows,
                                                    long long *__restrict__ flag, long long *__restrict__ cand_bs)
{
    __shared__ long long sm[4], tgt[KPP_MAX_T], blk[KPP_MAX_T], pre[KPP_MAX_T];
    const int t = threadIdx.x;
    for (long long b = t; b < (long long)T * nb; b += 256) cand_bs[b] = 0;  // the sums the sweep of this pick adds to
    if (s == 0) {
        if (t == 0) cand_rows[0] = min(m - 1, max(0ll, (long long)__dmul_rn(u[0], __ll2double_rn(m))));
        return;
    }
    long long a = 0, total = 0;
    for (int b = t; b < nb; b += 256) a += bs[b];
    (void)kpp_block_scan(a, sm, &total);
    if (total <= 0) {  // every row coincides with a chosen one: s distinct rows, no further centre
        if (t == 0 && *flag == 0) *flag = s;
        if (t < T) cand_rows[t] = 0;
        return;
    }
    if (t < T) {
        const double ut = u[1 + (size_t)(s - 1) * T + t];
        tgt[t] = min(total - 1, max(0ll, (long long)__dmul_rn(ut, __ll2double_rn(total))));
        blk[t] = nb - 1, pre[t] = total;  // (overwritten below: the block sums are the sums of w)
    }
    __syncthreads();
    long long base = 0;
    for (int c0 = 0; c0 < nb; c0 += 256) {
        const long long v = c0 + t < nb ? bs[c0 + t] : 0;
        long long chunk = 0;
        const long long excl = base + kpp_block_scan(v, sm, &chunk) - v;
        for (int q = 0; q < T; ++q) {
            const long long tg = tgt[q];
            if (excl <= tg && tg < excl + v) blk[q] = c0 + t, pre[q] = excl;  // exactly one thread of one chunk
        }
        base += chunk;
    }
    __syncthreads();
    for (int q = 0; q < T; ++q) {
        const long long i0 = blk[q] * KPP_BLOCK + 4 * t, tg = tgt[q];
        long long wv[4], v = 0, unused = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            wv[c] = i0 + c < m ? w[i0 + c] : 0;
            v += wv[c];
        }
        long long run = pre[q] + kpp_block_scan(v, sm, &unused) - v;
        if (run <= tg && tg < run + v) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool before = run <= tg;
                run += wv[c];
                if (before && run > tg) cand_rows[q] = i0 + c;
            }
        }
    }
}

// out[tau][i] = FIRST ? W(i, cand_rows[tau]) : min(w[i], W(i, cand_rows[tau])) for the trials tau0 <= tau < tau0 + ntau <= tau0 + NT;
// bs [T][nb] (NULL: skipped) += the sums of what was written.  Dynamic LDS: ntau * dpad floats.
template <int NT, bool VEC, bool FIRST>
__global__ __launch_bounds__(256) void k_kpp_sweep(const float *__restrict__ x, long long m, int d, int dpad,
                                                   const long long *__restrict__ cand_rows, int tau0, int ntau, double scale,
                                                   const long long *__restrict__ w, long long *__restrict__ out,
                                                   unsigned long long *__restrict__ bs, int nb)
{
    extern __shared__ __attribute__((aligned(16))) float cand[];  // [ntau][dpad]
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int q = 0; q < ntau; ++q) {
        const long long r = min(m - 1, max(0ll, cand_rows[tau0 + q]));
        const float *xr = x + (size_t)r * d;
        for (int j = threadIdx.x; j < dpad; j += 256) cand[(size_t)q * dpad + j] = j < d ? xr[j] : 0.f;
    }
    __syncthreads();
    const int groups = dpad / 256;  // 16-byte groups a lane owns
    const long long runs = (m + KPP_RUN - 1) / KPP_RUN;
    for (long long run = (long long)blockIdx.x * 4 + wave; run < runs; run += (long long)gridDim.x * 4) {
        const long long i0 = run * KPP_RUN;
        const int rows = (int)min((long long)KPP_RUN, m - i0);
        long long wmine = 0;
        if (!FIRST && lane < rows) wmine = w[i0 + lane];
        long long keep[NT], run_sum[NT];
#pragma unroll
        for (int q = 0; q < NT; ++q) keep[q] = 0, run_sum[q] = 0;
        for (int r = 0; r < rows; ++r) {
            const float *xi = x + (size_t)(i0 + r) * d;
            double acc[NT];
#pragma unroll
            for (int q = 0; q < NT; ++q) acc[q] = 0.0;
            for (int g0 = 0; g0 < groups; g0 += 4) {
                float4 v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {  // up to four loads in flight
                    const int col = 4 * (lane + 64 * (g0 + k));
                    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (VEC) {
                        if (col < d) v[k] = *reinterpret_cast<const float4 *>(xi + col);
                    } else {
                        if (col < d) v[k].x = xi[col];
                        if (col + 1 < d) v[k].y = xi[col + 1];
                        if (col + 2 < d) v[k].z = xi[col + 2];
                        if (col + 3 < d) v[k].w = xi[col + 3];
                    }
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (g0 + k >= groups) continue;
                    const int col = 4 * (lane + 64 * (g0 + k));
                    const double x0 = (double)v[k].x, x1 = (double)v[k].y, x2 = (double)v[k].z, x3 = (double)v[k].w;
#pragma unroll
                    for (int q = 0; q < NT; ++q) {
                        if (q >= ntau) continue;
                        const float4 c = *reinterpret_cast<const float4 *>(&cand[(size_t)q * dpad + col]);
                        const double e0 = __dsub_rn(x0, (double)c.x), e1 = __dsub_rn(x1, (double)c.y);
                        const double e2 = __dsub_rn(x2, (double)c.z), e3 = __dsub_rn(x3, (double)c.w);
                        double a = acc[q];
                        a = __dadd_rn(a, __dmul_rn(e0, e0));
                        a = __dadd_rn(a, __dmul_rn(e1, e1));
                        a = __dadd_rn(a, __dmul_rn(e2, e2));
                        a = __dadd_rn(a, __dmul_rn(e3, e3));
                        acc[q] = a;
                    }
                }
            }
            const long long wr = FIRST ? 0 : __shfl(wmine, r);
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                if (q >= ntau) continue;
                double a = acc[q];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) a = __dadd_rn(a, __shfl_xor(a, o));
                long long wq = __double2ll_rn(__dmul_rn(a, scale));
                if (!FIRST) wq = min(wq, wr);
                if (lane == r) keep[q] = wq;
                run_sum[q] += wq;
            }
        }
#pragma unroll
        for (int q = 0; q < NT; ++q) {
            if (q >= ntau) continue;
            if (lane < rows) out[(size_t)(tau0 + q) * m + i0 + lane] = keep[q];
            if (bs && lane == 0 && run_sum[q]) atomicAdd(&bs[(size_t)(tau0 + q) * nb + i0 / KPP_BLOCK], (unsigned long long)run_sum[q]);
        }
    }
}

// One workgroup: pot[tau] = the sum of the trial's block sums; *best = the trial of least potential, the lowest on ties;
// rows[s] = its row, potential[s] = its potential
__global__ __launch_bounds__(256) void k_kpp_best(int T, int nb, const long long *__restrict__ cand_bs, const long long *__restrict__ cand_rows,
                                                  int s, int *__restrict__ best_out, long long *__restrict__ rows_out,
                                                  long long *__restrict__ pot_out)
{
    __shared__ long long sm[4];
    int best = 0;
    long long least = 0;
    for (int q = 0; q < T; ++q) {
        long long a = 0, p = 0;
        for (int b = threadIdx.x; b < nb; b += 256) a += cand_bs[(size_t)q * nb + b];
        (void)kpp_block_scan(a, sm, &p);
        if (q == 0 || p < least) least = p, best = q;
    }
    if (threadIdx.x == 0) *best_out = best, rows_out[s] = cand_rows[best], pot_out[s] = least;
}

// w <- the column of the best trial, bs <- its block sums
__global__ __launch_bounds__(256) void k_kpp_select(int T, long long m, int nb, const long long *__restrict__ cand_w,
                                                    const long long *__restrict__ cand_bs, const int *__restrict__ best_in,
                                                    long long *__restrict__ w, long long *__restrict__ bs)
{
    const int best = min(max(*best_in, 0), T - 1);
    const long long stride = (long long)gridDim.x * 256, first = (long long)blockIdx.x * 256 + threadIdx.x;
    for (long long i = first; i < m; i += stride) w[i] = cand_w[(size_t)best * m + i];
    for (long long b = first; b < nb; b += stride) bs[b] = cand_bs[(size_t)best * nb + b];
}

int kpp_use_device(int device, int *cus)
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

struct KppSweep {
    const float *x;
    int64_t m;
    int d, dpad, per_sweep, nb, grid;
    bool vec;
    double scale;
};

int kpp_sweep_shape(KppSweep *sw, const float *x, int64_t m, int d, int t, int cus)
{
    sw->x = x, sw->m = m, sw->d = d;
    sw->dpad = (d + 255) / 256 * 256;
    sw->per_sweep = std::min(KPP_MAX_T, KPP_LDS_FLOATS / sw->dpad);  // >= 1: dpad <= 16384
    sw->nb = (int)((m + KPP_BLOCK - 1) / KPP_BLOCK);
    const int64_t runs = (m + KPP_RUN - 1) / KPP_RUN;
    sw->grid = (int)std::max<int64_t>(1, std::min<int64_t>((runs + 3) / 4, (int64_t)cus * KPP_PER_CU));
    sw->vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && d % 4 == 0;
    sw->scale = ldexp(1.0, t);
    return ACAV_OK;
}

template <int NT, bool FIRST>
void kpp_launch_nt(const KppSweep &sw, hipStream_t st, const long long *cand_rows, int tau0, int ntau, const long long *w, long long *out,
                   unsigned long long *bs)
{
    const size_t lds = sizeof(float) * (size_t)ntau * sw.dpad;
    if (sw.vec)
        hipLaunchKernelGGL((k_kpp_sweep<NT, true, FIRST>), dim3((unsigned)sw.grid), dim3(256), lds, st, sw.x, (long long)sw.m, sw.d, sw.dpad,
                           cand_rows, tau0, ntau, sw.scale, w, out, bs, sw.nb);
    else
        hipLaunchKernelGGL((k_kpp_sweep<NT, false, FIRST>), dim3((unsigned)sw.grid), dim3(256), lds, st, sw.x, (long long)sw.m, sw.d, sw.dpad,
                           cand_rows, tau0, ntau, sw.scale, w, out, bs, sw.nb);
}

// the sweeps of T trials: floor(16384 / dpad) trials at a time
template <bool FIRST>
void kpp_sweeps(const KppSweep &sw, hipStream_t st, const long long *cand_rows, int T, const long long *w, long long *out,
                unsigned long long *bs)
{
    for (int tau0 = 0; tau0 < T; tau0 += sw.per_sweep) {
        const int ntau = std::min(sw.per_sweep, T - tau0);
        if (ntau == 1) kpp_launch_nt<1, FIRST>(sw, st, cand_rows, tau0, ntau, w, out, bs);
        else if (ntau == 2) kpp_launch_nt<2, FIRST>(sw, st, cand_rows, tau0, ntau, w, out, bs);
        else if (ntau <= 4) kpp_launch_nt<4, FIRST>(sw, st, cand_rows, tau0, ntau, w, out, bs);
        else if (ntau <= 8) kpp_launch_nt<8, FIRST>(sw, st, cand_rows, tau0, ntau, w, out, bs);
        else kpp_launch_nt<16, FIRST>(sw, st, cand_rows, tau0, ntau, w, out, bs);
    }
}

int kpp_check_sizes(int64_t m, int d, int T, int t)
{
    ACAV_REQUIRE(m >= 1 && m < KPP_MAX_M, ACAV_EINVAL, "m=%lld must be in [1, 2^31)", (long long)m);
    ACAV_REQUIRE(d >= 1 && d <= KPP_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, KPP_MAX_D);
    ACAV_REQUIRE(T >= 1 && T <= KPP_MAX_T, ACAV_EINVAL, "T=%d trials must be in [1, %d]", T, KPP_MAX_T);
    ACAV_REQUIRE(t >= -KPP_MAX_SHIFT && t <= KPP_MAX_SHIFT, ACAV_EINVAL, "t=%d must be in [-%d, %d]", t, KPP_MAX_SHIFT, KPP_MAX_SHIFT);
    return ACAV_OK;
}

}  // namespace

ACAV_EXPORT int acav_kmeanspp_weights(int device, const float *x, int64_t m, int d, const int64_t *cand_rows, int T, int t, int64_t *out,
                                      void *stream)
{
    ACAV_REQUIRE(x && cand_rows && out, ACAV_EINVAL, "NULL argument");
    ACAV_TRY(kpp_check_sizes(m, d, T, t));
    ACAV_REQUIRE(!is_device_ptr(cand_rows), ACAV_EINVAL, "cand_rows is a host array");
    for (int q = 0; q < T; ++q)
        ACAV_REQUIRE(cand_rows[q] >= 0 && cand_rows[q] < m, ACAV_EINVAL, "cand_rows[%d] = %lld lies outside [0, %lld)", q,
                     (long long)cand_rows[q], (long long)m);
    int cus = 0;
    ACAV_TRY(kpp_use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf stage_x, dcand, dout;
    StreamDrain drain = {st};
    const void *dx = nullptr;
    ACAV_TRY(to_device(x, sizeof(float) * (size_t)m * d, stage_x, st, &dx));
    ACAV_TRY(upload(dcand, cand_rows, sizeof(int64_t) * (size_t)T, st));
    const size_t out_bytes = sizeof(int64_t) * (size_t)T * (size_t)m;
    long long *o = reinterpret_cast<long long *>(out);
    const bool out_dev = is_device_ptr(out);
    if (!out_dev) {
        ACAV_TRY(dout.ensure(out_bytes));
        o = dout.as<long long>();
    }
    KppSweep sw;
    ACAV_TRY(kpp_sweep_shape(&sw, static_cast<const float *>(dx), m, d, t, cus));
    kpp_sweeps<true>(sw, st, dcand.as<long long>(), T, nullptr, o, nullptr);
    ACAV_HIP_TRY(hipGetLastError());
    if (!out_dev) ACAV_HIP_TRY(hipMemcpyAsync(out, o, out_bytes, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}

ACAV_EXPORT int acav_kmeanspp_seed(int device, const float *x, int64_t m, int d, int k, int T, const double *u, int t, int64_t *rows_out,
                                   int64_t *potential_out, void *stream)
{
    ACAV_REQUIRE(x && u && rows_out && potential_out, ACAV_EINVAL, "NULL argument");
    ACAV_TRY(kpp_check_sizes(m, d, T, t));
    ACAV_REQUIRE(k >= 1 && k <= m, ACAV_EINVAL, "k=%d centres from m=%lld rows: k must be in [1, m]", k, (long long)m);
    ACAV_REQUIRE(!is_device_ptr(u) && !is_device_ptr(rows_out) && !is_device_ptr(potential_out), ACAV_EINVAL,
                 "u, rows_out and potential_out are host arrays");
    const size_t nu = 1 + (size_t)(k - 1) * T;
    for (size_t q = 0; q < nu; ++q)
        ACAV_REQUIRE(u[q] >= 0.0 && u[q] < 1.0, ACAV_EINVAL, "u[%lld] = %.17g lies outside [0, 1)", (long long)q, u[q]);
    int cus = 0;
    ACAV_TRY(kpp_use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf stage_x, du, w, bs, cand_w, cand_sums, cand_rows, results, flag, best;
    StreamDrain drain = {st};
    const void *dx = nullptr;
    ACAV_TRY(to_device(x, sizeof(float) * (size_t)m * d, stage_x, st, &dx));
    ACAV_TRY(upload(du, u, sizeof(double) * nu, st));
    KppSweep sw;
    ACAV_TRY(kpp_sweep_shape(&sw, static_cast<const float *>(dx), m, d, t, cus));
    const int nb = sw.nb;
    const size_t sums_bytes = sizeof(int64_t) * (size_t)T * nb;  // the trials' block sums
    ACAV_TRY(w.ensure(sizeof(int64_t) * (size_t)m));
    ACAV_TRY(bs.ensure(sizeof(int64_t) * (size_t)nb));
    ACAV_TRY(cand_w.ensure(sizeof(int64_t) * (size_t)T * (size_t)m));
    ACAV_TRY(cand_sums.ensure(sums_bytes));
    ACAV_TRY(cand_rows.ensure(sizeof(int64_t) * KPP_MAX_T));
    ACAV_TRY(results.ensure(sizeof(int64_t) * 2 * (size_t)k));
    ACAV_TRY(flag.ensure(sizeof(int64_t)));
    ACAV_TRY(best.ensure(sizeof(int)));
    ACAV_HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(int64_t), st));
    ACAV_HIP_TRY(hipMemsetAsync(cand_rows.p, 0, sizeof(int64_t) * KPP_MAX_T, st));
    unsigned long long *cbs = cand_sums.as<unsigned long long>();
    long long *drows = results.as<long long>(), *dpot = drows + k;
    const unsigned sel_grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>((m + 255) / 256, (int64_t)cus * 4));
    for (int s = 0; s < k; ++s) {
        const int trials = s == 0 ? 1 : T;
        hipLaunchKernelGGL(k_kpp_sample, dim3(1), dim3(256), 0, st, w.as<long long>(), bs.as<long long>(), (long long)m, nb,
                           du.as<double>(), s, T, cand_rows.as<long long>(), flag.as<long long>(), cand_sums.as<long long>());
        if (s == 0)
            kpp_sweeps<true>(sw, st, cand_rows.as<long long>(), trials, nullptr, cand_w.as<long long>(), cbs);
        else
            kpp_sweeps<false>(sw, st, cand_rows.as<long long>(), trials, w.as<long long>(), cand_w.as<long long>(), cbs);
        hipLaunchKernelGGL(k_kpp_best, dim3(1), dim3(256), 0, st, trials, nb, cand_sums.as<long long>(), cand_rows.as<long long>(), s,
                           best.as<int>(), drows, dpot);
        hipLaunchKernelGGL(k_kpp_select, dim3(sel_grid), dim3(256), 0, st, trials, (long long)m, nb, cand_w.as<long long>(),
                           cand_sums.as<long long>(), best.as<int>(), w.as<long long>(), bs.as<long long>());
        ACAV_HIP_TRY(hipGetLastError());
    }
    std::vector<int64_t> host(2 * (size_t)k);
    int64_t bad = 0;
    ACAV_HIP_TRY(hipMemcpyAsync(host.data(), results.p, sizeof(int64_t) * 2 * (size_t)k, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipMemcpyAsync(&bad, flag.p, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(bad == 0, ACAV_EINVAL, "the sample holds only %lld distinct rows: %d centres cannot be seeded from it", (long long)bad, k);
    memcpy(rows_out, host.data(), sizeof(int64_t) * (size_t)k);
    memcpy(potential_out, host.data() + k, sizeof(int64_t) * (size_t)k);
    return ACAV_OK;
}
