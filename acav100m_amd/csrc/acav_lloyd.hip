// acav_lloyd.hip -- the update half of batch (Lloyd) k-means: per-cluster column sums and counts of labelled feature rows in
// 64-bit fixed point (acav_rows_absmax, acav_lloyd_accumulate; clustering/lloyd.py).  The reference's clusterers
// (correspondence_retrieval/code/clustering.py, clustering_func_type = 'faiss' / 'scipy') move every centre to the mean of its rows
// once per pass; the assignment half is the existing acav_kmeans_assign sweep.
//
// Arithmetic.  q = rint((double)x * 2^s) as int64 (round half to even; the product is exact: a power of two times an fp32 value
// inside the double range), sums[label][j] += q, counts[label] += 1, all in integers.  The caller picks s from the largest |x| of
// ALL rows (acav_rows_absmax) and their number N such that |q| < 2^62 / N: no sum of N terms leaves int64.  Integer addition is
// associative, so the tables are a pure function of the rows and their labels -- not of the summation order, the grid, the
// device, the row groups or how the rows reached the device.  No floating-point atomics; the atomics here add integers.
//
// Schedule of one acav_lloyd_accumulate call (the scatter-add recipe: inverted index + chunked per-destination sums):
//   k_lloyd_bin<.., false>  histogram of the labels (a workgroup bins a contiguous run of rows in LDS, then adds its non-zero
//                           bins to the global histogram); a label outside [0, k) raises a flag and the call fails
//   host                    exclusive scan of the histogram -> list starts; every list is cut into CHUNKS of at most 512 rows
//                           (lloyd_chunks, the function acav_lloyd_accumulate_plan exposes)
//   k_lloyd_bin<.., true>   the inverted index: a workgroup reserves, per non-zero bin, a run of positions of the bin's list with
//                           one global add, then hands them to its rows with LDS adds.  The order inside a list is free.
//   k_lloyd_sum             one wave = one (chunk, strip of 64 columns): the chunk's rows through the index, one coalesced 256-B
//                           read per row, summed in registers; the partial goes into sums with one 64-bit integer add per column.
//                           A cluster is never one wave's job: a cluster holding half the rows is n / 1024 chunks like any other.
// Every feature byte is read once.
//
// acav_lloyd_centers: the centre update that follows, on the device.  centers[c][j] = (float)(((double)sums[c][j] * 2^-s) /
// (double)counts[c]) -- an int64 -> double conversion (round to nearest even), an exact scaling by a power of two, one IEEE double
// division and one rounding to fp32, each its own operation (the build has -ffp-contract=off and no fast-math): what
// clustering/lloyd.py:centers_from_sums computes in numpy, bit for bit.  One streaming kernel (k_lloyd_centers) over the
// [k][d] table as one flat array: 8 bytes read and 4 written per element, no LDS, one integer atomic per empty cluster.
#include <algorithm>
#include <cmath>
#include <vector>

#include "acav_common.h"

using namespace acav;

namespace {

constexpr int LL_CHUNK = 512;        // rows of a chunk at most
constexpr int LL_STRIP = 64;         // columns of a strip: one per lane
constexpr int LL_PER_CU = 8;         // workgroups per compute unit the grids are capped at
constexpr int LL_BIN_ROWS = 4096;    // rows a binning workgroup takes at least
constexpr int LL_LDS_BINS = 8192;    // k up to which a binning workgroup keeps its histogram in LDS (32 KB)
constexpr int LL_MAX_D = 16384;
constexpr int64_t LL_MAX_N = (int64_t)1 << 31;       // rows of ONE call: positions in the index are 32-bit
constexpr int64_t LL_MAX_TOTAL = (int64_t)1 << 37;   // rows of one acav_rows_absmax call
constexpr int LL_MAX_K = 1 << 30;
constexpr int LL_MAX_SHIFT = 1000;   // |s|: 2^s stays a normal double

struct LloydChunk {
    int label, start, rows;  // rows index[start .. start + rows) carry `label`
};

// the launch shapes of one accumulate call, a function of (n, k, d, cus) and the chunk count alone
struct LloydPlan {
    int64_t chunks;
    int strips;
    int64_t items;      // (chunk, strip) pairs, chunk-major: the strips of a chunk are neighbours in dispatch order
    int grid;           // k_lloyd_sum: four items per workgroup at a time
    int bin_grid;       // k_lloyd_bin: workgroup b bins the rows [b * bin_rows, (b + 1) * bin_rows)
    int64_t bin_rows;
    int lds_bins;       // 1: the binning workgroups keep their histogram in LDS
    size_t scratch;     // histogram + cursors + index + chunk list
};

// hist[k] -> the chunk list in label order (NULL: count only); returns the number of chunks
int64_t lloyd_chunks(const int64_t *hist, int k, std::vector<LloydChunk> *out)
{
    int64_t chunks = 0, start = 0;
    for (int b = 0; b < k; ++b) {
        for (int64_t r = 0; r < hist[b]; r += LL_CHUNK) {
            if (out) out->push_back({b, (int)(start + r), (int)std::min<int64_t>(LL_CHUNK, hist[b] - r)});
            ++chunks;
        }
        start += hist[b];
    }
    return chunks;
}

LloydPlan lloyd_plan(int64_t n, int k, int d, int cus, int64_t chunks)
{
    LloydPlan p;
    p.chunks = chunks;
    p.strips = (d + LL_STRIP - 1) / LL_STRIP;
    p.items = chunks * p.strips;
    p.grid = (int)std::max<int64_t>(1, std::min<int64_t>((p.items + 3) / 4, (int64_t)cus * LL_PER_CU));
    p.bin_grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + LL_BIN_ROWS - 1) / LL_BIN_ROWS, (int64_t)cus * 4));
    p.bin_rows = (n + p.bin_grid - 1) / p.bin_grid;
    p.lds_bins = k <= LL_LDS_BINS;
    p.scratch = sizeof(unsigned) * (2 * (size_t)k + (size_t)n) + sizeof(LloydChunk) * (size_t)chunks;
    return p;
}

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }

// out_bits = max over the elements of the bits of |x|: non-negative floats order like unsigned integers, and every inf / NaN
// pattern lies above every finite one -- the host sees a non-finite value as bits >= 0x7f800000
template <bool VEC>
__global__ __launch_bounds__(256) void k_rows_absmax(const float *__restrict__ x, size_t total, unsigned *__restrict__ out_bits)
{
    __shared__ unsigned sm[4];
    const size_t stride = (size_t)gridDim.x * 256;
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    unsigned m = 0;
    if (VEC) {
        const float4 *p = reinterpret_cast<const float4 *>(x);
        const size_t quads = total / 4;
        for (; i + 3 * stride < quads; i += 4 * stride) {  // four loads in flight
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = p[i + u * stride];
#pragma unroll
            for (int u = 0; u < 4; ++u) m = max(max(m, max(abs_bits(v[u].x), abs_bits(v[u].y))), max(abs_bits(v[u].z), abs_bits(v[u].w)));
        }
        for (; i < quads; i += stride) {
            const float4 v = p[i];
            m = max(max(m, max(abs_bits(v.x), abs_bits(v.y))), max(abs_bits(v.z), abs_bits(v.w)));
        }
        if (blockIdx.x == 0 && quads * 4 + threadIdx.x < total) m = max(m, abs_bits(x[quads * 4 + threadIdx.x]));  // 0..3 tail elements
    } else {
        for (; i < total; i += stride) m = max(m, abs_bits(x[i]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(out_bits, max(max(sm[0], sm[1]), max(sm[2], sm[3])));
}

// SCATTER = false: hist[label] += 1 for the n labels; a label outside [0, k) sets *bad and is skipped.
// SCATTER = true:  index[position] = row, the positions of a label's list handed out from cursor[label] (which starts at the
//                  list's first position).  Every position is below n when the labels are the ones the histogram counted; the
//                  store is guarded all the same.
// LDS: the workgroup bins its rows in LDS first and touches the global table once per non-zero bin.
template <bool LDS, bool SCATTER>
__global__ __launch_bounds__(256) void k_lloyd_bin(const int64_t *__restrict__ labels, int64_t n, int k, int64_t bin_rows,
                                                   unsigned *__restrict__ table, unsigned *__restrict__ index, unsigned *__restrict__ bad)
{
    __shared__ unsigned sh[LDS ? LL_LDS_BINS : 1];
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * bin_rows, r1 = min(n, r0 + bin_rows);
    if (!LDS) {
        for (int64_t r = r0 + t; r < r1; r += 256) {
            const int64_t l = labels[r];
            if (l < 0 || l >= k) {
                if (!SCATTER) atomicOr(bad, 1u);
                continue;
            }
            const unsigned pos = atomicAdd(&table[l], 1u);
            if (SCATTER && pos < (unsigned long long)n) index[pos] = (unsigned)r;
        }
        return;
    }
    for (int b = t; b < k; b += 256) sh[b] = 0u;
    __syncthreads();
    for (int64_t r = r0 + t; r < r1; r += 256) {
        const int64_t l = labels[r];
        if (l < 0 || l >= k) {
            if (!SCATTER) atomicOr(bad, 1u);
            continue;
        }
        atomicAdd(&sh[l], 1u);
    }
    __syncthreads();
    for (int b = t; b < k; b += 256) {
        const unsigned c = sh[b];
        if (c) {
            const unsigned base = atomicAdd(&table[b], c);
            if (SCATTER) sh[b] = base;  // the workgroup's run of positions in the list of b
        }
    }
    if (!SCATTER) return;
    __syncthreads();
    for (int64_t r = r0 + t; r < r1; r += 256) {
        const int64_t l = labels[r];
        if (l < 0 || l >= k) continue;
        const unsigned pos = atomicAdd(&sh[l], 1u);
        if (pos < (unsigned long long)n) index[pos] = (unsigned)r;
    }
}

__global__ __launch_bounds__(256) void k_lloyd_counts(const unsigned *__restrict__ hist, int k, unsigned long long *__restrict__ counts)
{
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b < k && hist[b]) atomicAdd(&counts[b], (unsigned long long)hist[b]);
}

__device__ __forceinline__ long long ll_quant(float v, double scale) { return __double2ll_rn((double)v * scale); }

// One wave per (chunk, strip): lane l owns column strip * 64 + l.  The row numbers of up to 64 rows sit one per lane and are
// broadcast one at a time; eight row reads are in flight per wave.
__global__ __launch_bounds__(256) void k_lloyd_sum(const float *__restrict__ x, int64_t n, int d, const unsigned *__restrict__ index,
                                                   const LloydChunk *__restrict__ chunks, int64_t items, int strips, double scale,
                                                   unsigned long long *__restrict__ sums)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int64_t item = (int64_t)blockIdx.x * 4 + wave; item < items; item += (int64_t)gridDim.x * 4) {
        const int64_t chunk = item / strips;
        const int strip = (int)(item - chunk * strips);
        const int label = chunks[chunk].label, start = chunks[chunk].start, rows = chunks[chunk].rows;
        const int col = strip * LL_STRIP + lane;
        const bool valid = col < d;
        const float *xc = x + (valid ? col : 0);
        long long acc = 0;
        for (int r0 = 0; r0 < rows; r0 += 64) {
            const int m = min(64, rows - r0);
            const int mine = lane < m ? (int)min(index[start + r0 + lane], (unsigned)(n - 1)) : 0;  // (never beyond the rows)
            int i = 0;
            for (; i + 8 <= m; i += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const size_t row = (size_t)(unsigned)__builtin_amdgcn_readlane(mine, i + u);
                    v[u] = valid ? xc[row * d] : 0.f;
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += ll_quant(v[u], scale);
            }
            for (; i < m; ++i) {
                const size_t row = (size_t)(unsigned)__builtin_amdgcn_readlane(mine, i);
                acc += ll_quant(valid ? xc[row * d] : 0.f, scale);
            }
        }
        if (valid) atomicAdd(&sums[(size_t)label * d + col], (unsigned long long)acc);
    }
}

// The flat table of k * d elements in quads: a thread loads two 16-byte pairs of sums and stores one 16-byte quad of centres
// (vec: both tables start on a 16-byte boundary; a quad's place in the flat array is then aligned whatever the row pitch d).
// A quad may cross rows: the row c and column r of its first element come from one division, the others by stepping.  The last
// total % 4 elements, and every element when !vec, go one by one through the same arithmetic (ll_center).  The thread that
// holds column 0 of row c writes sizes[c] and counts the row when it is empty.
__device__ __forceinline__ float ll_center(long long sum, long long count, double inv_scale)
{
    if (count == 0) return 0.f;
    const double scaled = (double)sum * inv_scale;  // exact: a power of two
    return (float)(scaled / (double)count);
}

__global__ __launch_bounds__(256) void k_lloyd_centers(const long long *__restrict__ sums, const long long *__restrict__ counts,
                                                       unsigned total, unsigned d, double inv_scale, int vec,
                                                       float *__restrict__ centers, float *__restrict__ sizes, unsigned *__restrict__ empty)
{
    const unsigned quads = vec ? total / 4 : 0;
    const unsigned stride = gridDim.x * 256;
    for (unsigned q = blockIdx.x * 256 + threadIdx.x; q < quads; q += stride) {
        const unsigned e = 4 * q;
        const longlong2 a = reinterpret_cast<const longlong2 *>(sums)[2 * q], b = reinterpret_cast<const longlong2 *>(sums)[2 * q + 1];
        const long long v[4] = {a.x, a.y, b.x, b.y};
        unsigned c = e / d, r = e - c * d;
        long long n = counts[c];
        float out[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (r == 0) {
                sizes[c] = (float)n;
                if (n == 0) atomicAdd(empty, 1u);
            }
            out[u] = ll_center(v[u], n, inv_scale);
            if (++r == d && u < 3 && e + u + 1 < total) {
                r = 0;
                n = counts[++c];
            }
        }
        reinterpret_cast<float4 *>(centers)[q] = make_float4(out[0], out[1], out[2], out[3]);
    }
    for (unsigned e = 4 * quads + blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
        const unsigned c = e / d, r = e - c * d;
        const long long n = counts[c];
        if (r == 0) {
            sizes[c] = (float)n;
            if (n == 0) atomicAdd(empty, 1u);
        }
        centers[e] = ll_center(sums[e], n, inv_scale);
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

ACAV_EXPORT int acav_rows_absmax(int device, const float *x, int64_t n, int d, float *out, void *stream)
{
    ACAV_REQUIRE(out && (n == 0 || x), ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < LL_MAX_TOTAL, ACAV_EINVAL, "n must be in [0, 2^37)");
    ACAV_REQUIRE(d >= 1 && d <= LL_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, LL_MAX_D);
    *out = 0.f;
    if (n == 0) return ACAV_OK;
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf stage_x, bits;
    StreamDrain drain = {st};
    const void *dx = nullptr;
    const size_t total = (size_t)n * d;
    ACAV_TRY(to_device(x, sizeof(float) * total, stage_x, st, &dx));
    ACAV_TRY(bits.ensure(sizeof(unsigned)));
    ACAV_HIP_TRY(hipMemsetAsync(bits.p, 0, sizeof(unsigned), st));
    const float *xd = static_cast<const float *>(dx);
    const bool vec = (reinterpret_cast<uintptr_t>(xd) & 15) == 0;
    const size_t per = vec ? 4 : 1;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((total / per + 255) / 256, (size_t)cus * LL_PER_CU));
    if (vec)
        hipLaunchKernelGGL(k_rows_absmax<true>, dim3(grid), dim3(256), 0, st, xd, total, bits.as<unsigned>());
    else
        hipLaunchKernelGGL(k_rows_absmax<false>, dim3(grid), dim3(256), 0, st, xd, total, bits.as<unsigned>());
    ACAV_HIP_TRY(hipGetLastError());
    unsigned h = 0;
    ACAV_HIP_TRY(hipMemcpyAsync(&h, bits.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(h < 0x7f800000u, ACAV_EINVAL, "the rows hold a value that is not finite (inf or NaN)");
    memcpy(out, &h, sizeof(float));
    return ACAV_OK;
}

ACAV_EXPORT int acav_lloyd_accumulate_plan(const int64_t *hist, int k, int d, int cus, int64_t *out, int64_t *chunks, int64_t cap)
{
    ACAV_REQUIRE(hist && out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(k >= 1 && k <= LL_MAX_K && d >= 1 && d <= LL_MAX_D && cus > 0, ACAV_EINVAL, "bad sizes");
    int64_t n = 0;
    for (int b = 0; b < k; ++b) {
        ACAV_REQUIRE(hist[b] >= 0 && hist[b] < LL_MAX_N, ACAV_EINVAL, "hist[%d] = %lld must be in [0, 2^31)", b, (long long)hist[b]);
        n += hist[b];
        ACAV_REQUIRE(n < LL_MAX_N, ACAV_EINVAL, "the lists hold 2^31 rows or more: one call takes fewer");
    }
    std::vector<LloydChunk> list;
    const int64_t count = lloyd_chunks(hist, k, chunks ? &list : nullptr);
    ACAV_REQUIRE(!chunks || cap >= count, ACAV_EINVAL, "room for %lld chunks, the lists are cut into %lld", (long long)cap, (long long)count);
    const LloydPlan p = lloyd_plan(n, k, d, cus, count);
    out[0] = LL_CHUNK, out[1] = p.chunks, out[2] = p.strips, out[3] = p.items, out[4] = p.grid, out[5] = p.bin_grid;
    out[6] = p.bin_rows, out[7] = p.lds_bins, out[8] = (int64_t)p.scratch;
    if (chunks)
        for (int64_t c = 0; c < count; ++c)
            chunks[3 * c] = list[(size_t)c].label, chunks[3 * c + 1] = list[(size_t)c].start, chunks[3 * c + 2] = list[(size_t)c].rows;
    return ACAV_OK;
}

ACAV_EXPORT int acav_lloyd_accumulate(int device, const float *x, int64_t n, int d, const int64_t *labels, int k, int s,
                                      int64_t *sums, int64_t *counts, void *stream)
{
    ACAV_REQUIRE(sums && counts && (n == 0 || (x && labels)), ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 0 && n < LL_MAX_N, ACAV_EINVAL, "n must be in [0, 2^31): split the rows into several calls");
    ACAV_REQUIRE(d >= 1 && d <= LL_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, LL_MAX_D);
    ACAV_REQUIRE(k >= 1 && (int64_t)k * d <= ((int64_t)1 << 30), ACAV_EINVAL, "k=%d: k * d must be in [1, 2^30]", k);
    ACAV_REQUIRE(s >= -LL_MAX_SHIFT && s <= LL_MAX_SHIFT, ACAV_EINVAL, "s=%d must be in [-%d, %d]", s, LL_MAX_SHIFT, LL_MAX_SHIFT);
    if (n == 0) return ACAV_OK;
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool tables_dev = is_device_ptr(sums);
    ACAV_REQUIRE(tables_dev == is_device_ptr(counts), ACAV_EINVAL, "sums and counts live on the same side: both host or both device");
    std::vector<unsigned> hhist((size_t)k), starts((size_t)k);
    std::vector<int64_t> h64((size_t)k);
    std::vector<LloydChunk> list;
    unsigned bad = 0;
    // scratch of this call only (parked blocks of the library's pool)
    DevBuf stage_x, stage_lab, stage_sums, stage_counts, hist, cursor, index, dchunks, flag;
    StreamDrain drain = {st};
    const void *dx = nullptr, *dl = nullptr;
    ACAV_TRY(to_device(x, sizeof(float) * (size_t)n * d, stage_x, st, &dx));
    ACAV_TRY(to_device(labels, sizeof(int64_t) * (size_t)n, stage_lab, st, &dl));
    unsigned long long *dsums = reinterpret_cast<unsigned long long *>(sums), *dcounts = reinterpret_cast<unsigned long long *>(counts);
    if (!tables_dev) {
        ACAV_TRY(upload(stage_sums, sums, sizeof(int64_t) * (size_t)k * d, st));
        ACAV_TRY(upload(stage_counts, counts, sizeof(int64_t) * (size_t)k, st));
        dsums = stage_sums.as<unsigned long long>(), dcounts = stage_counts.as<unsigned long long>();
    }
    ACAV_TRY(hist.ensure(sizeof(unsigned) * (size_t)k));
    ACAV_TRY(flag.ensure(sizeof(unsigned)));
    ACAV_TRY(index.ensure(sizeof(unsigned) * (size_t)n));
    ACAV_HIP_TRY(hipMemsetAsync(hist.p, 0, sizeof(unsigned) * (size_t)k, st));
    ACAV_HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(unsigned), st));
    const int64_t *lab = static_cast<const int64_t *>(dl);
    LloydPlan plan = lloyd_plan(n, k, d, cus, 0);

    // ---- histogram
    if (plan.lds_bins)
        hipLaunchKernelGGL((k_lloyd_bin<true, false>), dim3((unsigned)plan.bin_grid), dim3(256), 0, st, lab, n, k, plan.bin_rows,
                           hist.as<unsigned>(), (unsigned *)nullptr, flag.as<unsigned>());
    else
        hipLaunchKernelGGL((k_lloyd_bin<false, false>), dim3((unsigned)plan.bin_grid), dim3(256), 0, st, lab, n, k, plan.bin_rows,
                           hist.as<unsigned>(), (unsigned *)nullptr, flag.as<unsigned>());
    ACAV_HIP_TRY(hipGetLastError());
    ACAV_HIP_TRY(hipMemcpyAsync(hhist.data(), hist.p, sizeof(unsigned) * (size_t)k, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipMemcpyAsync(&bad, flag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(bad == 0, ACAV_EINVAL, "a label lies outside [0, %d): nothing was added", k);

    // ---- scan and chunk list (host), inverted index
    int64_t run = 0;
    for (int b = 0; b < k; ++b) {
        h64[(size_t)b] = hhist[(size_t)b];
        starts[(size_t)b] = (unsigned)run;
        run += hhist[(size_t)b];
    }
    ACAV_REQUIRE(run == n, ACAV_ESTATE, "internal: the histogram holds %lld of %lld rows", (long long)run, (long long)n);
    plan = lloyd_plan(n, k, d, cus, lloyd_chunks(h64.data(), k, &list));
    ACAV_TRY(upload(cursor, starts.data(), sizeof(unsigned) * (size_t)k, st));
    ACAV_TRY(upload(dchunks, list.data(), sizeof(LloydChunk) * list.size(), st));
    if (plan.lds_bins)
        hipLaunchKernelGGL((k_lloyd_bin<true, true>), dim3((unsigned)plan.bin_grid), dim3(256), 0, st, lab, n, k, plan.bin_rows,
                           cursor.as<unsigned>(), index.as<unsigned>(), flag.as<unsigned>());
    else
        hipLaunchKernelGGL((k_lloyd_bin<false, true>), dim3((unsigned)plan.bin_grid), dim3(256), 0, st, lab, n, k, plan.bin_rows,
                           cursor.as<unsigned>(), index.as<unsigned>(), flag.as<unsigned>());

    // ---- sums and counts
    hipLaunchKernelGGL(k_lloyd_sum, dim3((unsigned)plan.grid), dim3(256), 0, st, static_cast<const float *>(dx), n, d, index.as<unsigned>(),
                       dchunks.as<LloydChunk>(), plan.items, plan.strips, ldexp(1.0, s), dsums);
    hipLaunchKernelGGL(k_lloyd_counts, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, hist.as<unsigned>(), k, dcounts);
    ACAV_HIP_TRY(hipGetLastError());
    if (!tables_dev) {
        ACAV_HIP_TRY(hipMemcpyAsync(sums, dsums, sizeof(int64_t) * (size_t)k * d, hipMemcpyDeviceToHost, st));
        ACAV_HIP_TRY(hipMemcpyAsync(counts, dcounts, sizeof(int64_t) * (size_t)k, hipMemcpyDeviceToHost, st));
    }
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}

ACAV_EXPORT int acav_lloyd_centers(int device, const int64_t *sums_dev, const int64_t *counts_dev, int k, int d, int s,
                                   float *centers_dev, float *sizes_dev, int64_t *empty_host, void *stream)
{
    ACAV_REQUIRE(sums_dev && counts_dev && centers_dev && sizes_dev && empty_host, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(d >= 1 && d <= LL_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, LL_MAX_D);
    ACAV_REQUIRE(k >= 1 && (int64_t)k * d <= ((int64_t)1 << 30), ACAV_EINVAL, "k=%d: k * d must be in [1, 2^30]", k);
    ACAV_REQUIRE(s >= -LL_MAX_SHIFT && s <= LL_MAX_SHIFT, ACAV_EINVAL, "s=%d must be in [-%d, %d]", s, LL_MAX_SHIFT, LL_MAX_SHIFT);
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    ACAV_REQUIRE(is_device_ptr(sums_dev) && is_device_ptr(counts_dev) && is_device_ptr(centers_dev) && is_device_ptr(sizes_dev),
                 ACAV_EINVAL, "sums, counts, centers and sizes are device tables: a host table takes the host path of the caller");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevBuf flag;
    StreamDrain drain = {st};
    ACAV_TRY(flag.ensure(sizeof(unsigned)));
    ACAV_HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(unsigned), st));
    const unsigned total = (unsigned)((int64_t)k * d);
    const int vec = ((reinterpret_cast<uintptr_t>(sums_dev) | reinterpret_cast<uintptr_t>(centers_dev)) & 15) == 0;
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(((int64_t)total / (vec ? 4 : 1) + 255) / 256, (int64_t)cus * LL_PER_CU));
    hipLaunchKernelGGL(k_lloyd_centers, dim3(grid), dim3(256), 0, st, reinterpret_cast<const long long *>(sums_dev),
                       reinterpret_cast<const long long *>(counts_dev), total, (unsigned)d, ldexp(1.0, -s), vec, centers_dev, sizes_dev,
                       flag.as<unsigned>());
    ACAV_HIP_TRY(hipGetLastError());
    unsigned h = 0;
    ACAV_HIP_TRY(hipMemcpyAsync(&h, flag.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    *empty_host = (int64_t)h;
    return ACAV_OK;
}
