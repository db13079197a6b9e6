// acav_neardup.hip -- near-duplicates inside clusters (acav_rows_neardup; clustering/dedup.py, the `dedup` verb): for every row
// the largest cosine to an EARLIER row of its own cluster and that row, every such pair in float64.  SemDeDup's rule with the
// clusterings as the blocking structure; the reference removes duplicates only upstream, inside one video.
//
// Arithmetic.  Everything is float64 on the stored fp32 values, as in acav_silhouette.hip: nrm_i = ||x_i||^2 one wave per row
// (lane l chains fma(v, v, .) over its columns l, l + 64, ... from +0, then v[l] + v[l ^ o] for o = 32 ... 1), dot(i, j) one chain
// of v_mfma_f64_16x16x4_f64 over the columns 0, 4, 8, ... from a zero accumulator (tails in d are zero-filled when a stage is
// loaded: they add exactly 0), cos(i, j) = dot(i, j) / sqrt(nrm_i * nrm_j): one product, one sqrt, one division.
//
// Label-sorted positions.  The entry sorts the positions by label, stably, so a cluster is one contiguous RUN in which ascending
// sorted position is ascending input position.  The earlier rows of row p's cluster are then the sorted positions
// [start of p's run, p): one pair of bounds per row, no run ids.  A column whose norm is 0 is stored as -inf and never wins.
//
// Tiling.  One workgroup (4 waves) owns a tile of ND_QM = 64 RT consecutive sorted positions (RT = 1 or 2 by the plan) and walks
// the column blocks of ND_CN = 64 sorted positions from the block that holds the start of its FIRST row's run up to the block
// that holds its own LAST row: the work is triangular.  Stages, operands and accumulators are acav_silhouette.hip's.  After the
// last stage of a block the tile's cosines go to LDS (over the stages) and one thread per query row walks its columns
// max(block start, run start) ... min(block end, p) - 1 in ascending position with a strict `>`: the lowest position wins a tie,
// within a block and -- the blocks being walked in ascending order -- across them.
//
// Tile list.  Tiles late in a large cluster walk more blocks than early ones, so the host orders the tiles by descending number
// of blocks (ties: ascending tile index) and workgroup b takes entry b of that list: the long tiles start first.  neardup_tiles
// builds the list from the label histogram alone; acav_rows_neardup_plan exposes it, the entry point launches from it.
//
// Invariance.  (best_i, partner_i) is a pure function of the rows of cluster labels[i] up to row i: the dot of a pair is the same
// chain wherever the pair sits in a tile, the maximum is taken in ascending position whatever the tile size, the workgroup, the
// other clusters or host / device / unaligned input (the guarded load path feeds the same values into the same chain).  No
// floating-point atomics; the same call gives the same bytes every time.
//
// Against a held-out set (acav_rows_crossdup; dedup.nearest_in, `dedup --dedup.against_path`): the same arithmetic over TWO
// arrays.  For every row of a pool piece x the largest cosine to a row of the held-out set y with its label and that row.  Both
// arrays are label-sorted; per sorted pool position the run [ylo, yhi) of its label in y's sorted order replaces the triangle's
// bounds, and a tile walks the column blocks of y that cover [ylo of its first row, yhi of its last row): a rectangle per
// label, one contiguous range per tile, possibly empty.  k_crossdup is k_neardup's stage loop with the columns taken from y;
// crossdup_tiles builds its tile list from the two histograms.  A pool row's result depends on no other pool row, so the pool
// may come in pieces of any length: only y has to be resident.
//
// Multi-probe (acav_rows_probedup; dedup.nearest_earlier / nearest_in with probes, `dedup --dedup.probes=m`): a pair that a
// cluster border splits is missed by both sweeps above.  Here a row is compared with the rows of y in the m clusters its probe
// list names (acav_kmeans_probes: its own and the m - 1 centres next nearest).  The queries are (probed cluster, row) ENTRIES,
// sorted by cluster and then by row; an entry's columns are a prefix [ystart[c], ystart[c] + r) of the cluster's run in y's
// sorted order (r: the rows of the cluster below before[i]; all without a cut), which is k_crossdup's pair of bounds per
// position -- the sweep is k_crossdup over entries (its ENTRY instantiation keeps the results by entry), and k_pd_fold merges
// a row's at most m entry results in slot order, the larger cosine first, then the lower position.  In the in-set use a tile
// of entries late in a cluster walks a prefix of the run: the triangle, m times.  probedup_entries and probedup_tiles build
// entries and tile list on the host; acav_rows_probedup_plan exposes them, the entry point launches from them.
//
// Every pair over a threshold (acav_rows_neardup_pairs; dedup.pairs_earlier, `dedup --dedup.groups=True`): the graph of which
// (best, partner) is the nearest-earlier forest, in two sweeps of k_neardup's stage loop (k_neardup_pairs, a sibling kernel:
// k_neardup is the text it was).  COUNT: the walker of a row also counts the columns of its range at cosine >= threshold; the
// host sums the counts over input positions into offsets.  EMIT, over the tiles that hold a row with pairs (pairs_tiles filters
// the count sweep's list, order kept): the walker stores those columns in ascending position from offsets[i] on, never at or
// beyond offsets[i + 1]; a count that differs from the first raises a flag (ACAV_ESTATE).  No atomics, no sort; a pair's
// cosine is the value the count sweep compared, the same chain.  acav_pairs_components: union-find on the host, no device.
//
// A list of pairs (acav_pairs_cosine; dedup.pair_cosines, `dedup --dedup.confirm_view=`): the cosines of given pairs (i, j) of
// another array -- no labels, no runs, no walk.  k_paircos puts 16 pair_i rows and 16 pair_j rows of a wave through k_neardup's
// stage loop and keeps the diagonal of the one accumulator: the kernel is bound by the gather, and the same instruction over
// the same stages makes a pair's cosine the bytes the sweeps above give for it.
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

#include "acav_common.h"

using namespace acav;

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int64_t ND_MAX_N = ((int64_t)1 << 31) - 1;  // positions are 32-bit
constexpr int ND_MAX_D = 16384;
constexpr int ND_QM = 64;        // query rows of a tile per RT: 16 per wave
constexpr int ND_CN = 64;        // columns of a block: four 16 x 16 accumulators per wave and RT
constexpr int ND_DK = 32;        // columns of d of a stage
constexpr int ND_ST = ND_DK + 4; // fp32 stage, row stride: the 16 rows x 4 columns of a fragment fall into 64 different banks
constexpr int ND_CS = ND_CN + 1; // float64 cosine tile, row stride: the walk's lanes (one row each) fall into different bank pairs

constexpr size_t neardup_lds(int rt)
{
    // the cosine tile lies over the two stages (which are dead by then)
    return std::max(sizeof(double) * (size_t)ND_QM * rt * ND_CS, sizeof(float) * (size_t)(ND_QM * rt + ND_CN) * ND_ST);
}
static_assert(2 * neardup_lds(2) <= 160 * 1024, "two workgroups of the larger tile share a compute unit's LDS");

struct NdTile {
    int q0, rows, cb0, blocks;  // first sorted position, rows, first column block, column blocks
};

struct NdPlan {
    int rt;
    int64_t tiles, blocks;  // blocks: column blocks walked by all tiles together
    size_t lds, scratch;
};

// 128-row tiles (less operand traffic per multiply-add) once they alone give every compute unit a workgroup, 64-row tiles
// otherwise: acav_rows_silhouette_plan's rule
int neardup_rt(int64_t n, int cus) { return (n + 2 * ND_QM - 1) / (2 * ND_QM) >= cus ? 2 : 1; }

// the tiles of a label histogram: tile t holds the sorted positions [t QM, min(n, (t + 1) QM)) and walks the column blocks from
// the one that holds the start of the run of its first row up to the one that holds its last row.  list (NULL: skipped): the
// tiles by descending blocks, ties by ascending t.  Returns the plan.
NdPlan neardup_tiles(const int64_t *hist, int k, int d, int cus, std::vector<NdTile> *list)
{
    (void)d;
    int64_t n = 0;
    for (int b = 0; b < k; ++b) n += hist[b];
    NdPlan p;
    p.rt = neardup_rt(n, cus);
    const int64_t qm = (int64_t)ND_QM * p.rt;
    p.tiles = (n + qm - 1) / qm;
    p.blocks = 0;
    if (list) list->clear(), list->reserve((size_t)p.tiles);
    int b = 0;
    int64_t start = 0;  // of the run that holds the tile's first row
    for (int64_t t = 0; t < p.tiles; ++t) {
        const int64_t q0 = t * qm, q1 = std::min(n, q0 + qm);
        while (start + hist[b] <= q0) start += hist[b], ++b;  // empty labels have no run
        const int64_t cb0 = start / ND_CN, cb1 = (q1 - 1) / ND_CN;
        p.blocks += cb1 - cb0 + 1;
        if (list) list->push_back(NdTile{(int)q0, (int)(q1 - q0), (int)cb0, (int)(cb1 - cb0 + 1)});
    }
    if (list) std::stable_sort(list->begin(), list->end(), [](const NdTile &a, const NdTile &c) { return a.blocks > c.blocks; });
    p.lds = neardup_lds(p.rt);
    // the sorted positions and run starts, the norms, the tile list, (best, partner)
    p.scratch = sizeof(int) * 2 * (size_t)n + sizeof(double) * (size_t)n + sizeof(NdTile) * (size_t)p.tiles +
                (sizeof(double) + sizeof(int64_t)) * (size_t)n;
    return p;
}

// labels outside [0, k): counted before anything is indexed with a label
__global__ __launch_bounds__(256) void k_nd_labels(const int64_t *__restrict__ labels, int64_t n, int k, unsigned *__restrict__ bad)
{
    unsigned mine = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        mine += (labels[i] < 0 || labels[i] >= k) ? 1u : 0u;
    if (mine) atomicAdd(bad, mine);
}

// values that are not finite (an all-ones exponent), counted likewise
__global__ __launch_bounds__(256) void k_nd_finite(const float *__restrict__ x, size_t total, unsigned long long *__restrict__ bad)
{
    unsigned long long mine = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256)
        mine += (__float_as_uint(x[i]) & 0x7f800000u) == 0x7f800000u ? 1ull : 0ull;
    if (mine) atomicAdd(bad, mine);
}

// one wave per sorted position c: nrm[c] = ||x[perm[c]]||^2 (lane l: columns l, l + 64, ...; then a fixed tree)
__global__ __launch_bounds__(64) void k_nd_norms(const float *__restrict__ x, int d, const int *__restrict__ perm, double *__restrict__ nrm)
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

// columns j .. j + 3 of a row as they are stored; no branch: the load goes to a clamped address inside the row, nd_mask zeroes
// what was clamped
template <bool VEC>
__device__ __forceinline__ float4 nd_fetch(const float *__restrict__ r, int d, int j)
{
    if (VEC) return *reinterpret_cast<const float4 *>(r + min(j, d - 4));  // d % 4 == 0: j < d means j + 3 < d
    return make_float4(r[min(j, d - 1)], r[min(j + 1, d - 1)], r[min(j + 2, d - 1)], r[min(j + 3, d - 1)]);
}

__device__ __forceinline__ float4 nd_mask(float4 a, bool row_ok, int d, int j)
{
    float4 v;
    v.x = (row_ok && j < d) ? a.x : 0.f;
    v.y = (row_ok && j + 1 < d) ? a.y : 0.f;
    v.z = (row_ok && j + 2 < d) ? a.z : 0.f;
    v.w = (row_ok && j + 3 < d) ? a.w : 0.f;
    return v;
}

// perm[c]: the input position of sorted position c; rstart[c]: the sorted position its run starts at; nrm[c]: ||x||^2.
// tiles[b]: the tile workgroup b takes.  best / partner: by INPUT position
template <int RT, bool VEC>
__global__ __launch_bounds__(256, 2) void k_neardup(const float *__restrict__ x, int d, int n, const int *__restrict__ perm,
                                                    const int *__restrict__ rstart, const double *__restrict__ nrm,
                                                    const NdTile *__restrict__ tiles, double *__restrict__ best,
                                                    int64_t *__restrict__ partner)
{
    constexpr int QM = ND_QM * RT;
    extern __shared__ double nd_smem[];
    double *cosv = nd_smem;                          // [QM][ND_CS], after the last chunk of a block
    float *qs = reinterpret_cast<float *>(nd_smem);  // [QM][ND_ST]
    float *cs = qs + QM * ND_ST;                     // [ND_CN][ND_ST]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;  // fragment row (A) / column (B) and k index of this lane
    const int lq = t & 7, lr = t >> 3;         // this thread stages columns 4 lq .. 4 lq + 3 of the rows lr + 32 u
    const NdTile tile = tiles[blockIdx.x];
    const int q0 = tile.q0, q1 = tile.q0 + tile.rows;  // q1 <= n
    const double inf = __builtin_inf();

    // the query rows this thread stages, and the ones whose results it holds
    const float *qrow[2 * RT];
    bool qok[2 * RT];
#pragma unroll
    for (int u = 0; u < 2 * RT; ++u) {
        const int q = q0 + lr + 32 * u;
        qok[u] = q < q1;
        qrow[u] = x + (size_t)perm[qok[u] ? q : q0] * d;
    }
    double qn[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
            const int q = q0 + wave * 16 * RT + rt * 16 + fq + 4 * r;
            qn[rt][r] = nrm[q < q1 ? q : q0];
        }
    // the walk: thread t < QM owns query row t of the tile; a zero row has no partner and is none
    const int my_pos = q0 + t;
    const bool walker = t < QM && my_pos < q1;
    const int my_lo = walker && nrm[my_pos] > 0.0 ? rstart[my_pos] : n;  // its columns: the sorted positions [my_lo, my_pos)
    double top = -inf;
    int arg = -1;

    for (int cb = tile.cb0; cb < tile.cb0 + tile.blocks; ++cb) {
        const int c0 = cb * ND_CN;  // c0 <= q1 - 1 < n
        const float *crow[2];
        bool cok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = c0 + lr + 32 * u;
            cok[u] = c < n;
            crow[u] = x + (size_t)perm[cok[u] ? c : c0] * d;
        }
        f64x4 acc[RT][4];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f64x4{0.0, 0.0, 0.0, 0.0};
        float4 pq[2 * RT], pc[2];  // the next chunk, in flight while the current one is multiplied
#pragma unroll
        for (int u = 0; u < 2 * RT; ++u) pq[u] = nd_fetch<VEC>(qrow[u], d, 4 * lq);
#pragma unroll
        for (int u = 0; u < 2; ++u) pc[u] = nd_fetch<VEC>(crow[u], d, 4 * lq);
        for (int j0 = 0; j0 < d; j0 += ND_DK) {
            __syncthreads();  // the previous stage has been read (and the previous block's cosine tile walked)
#pragma unroll
            for (int u = 0; u < 2 * RT; ++u)
                *reinterpret_cast<float4 *>(&qs[(lr + 32 * u) * ND_ST + 4 * lq]) = nd_mask(pq[u], qok[u], d, j0 + 4 * lq);
#pragma unroll
            for (int u = 0; u < 2; ++u)
                *reinterpret_cast<float4 *>(&cs[(lr + 32 * u) * ND_ST + 4 * lq]) = nd_mask(pc[u], cok[u], d, j0 + 4 * lq);
            __syncthreads();
            if (j0 + ND_DK < d) {
#pragma unroll
                for (int u = 0; u < 2 * RT; ++u) pq[u] = nd_fetch<VEC>(qrow[u], d, j0 + ND_DK + 4 * lq);
#pragma unroll
                for (int u = 0; u < 2; ++u) pc[u] = nd_fetch<VEC>(crow[u], d, j0 + ND_DK + 4 * lq);
            }
#pragma unroll
            for (int kk = 0; kk < ND_DK / 4; ++kk) {
                double a[RT], b[4];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = (double)qs[(wave * 16 * RT + rt * 16 + fr) * ND_ST + kk * 4 + fq];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) b[ct] = (double)cs[(ct * 16 + fr) * ND_ST + kk * 4 + fq];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt], b[ct], acc[rt][ct], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave has read the last stage: the cosine tile goes over it
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int c = c0 + ct * 16 + fr;
            const double cn = nrm[c < n ? c : n - 1];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    cosv[(wave * 16 * RT + rt * 16 + fq + 4 * r) * ND_CS + ct * 16 + fr] =
                        cn > 0.0 ? acc[rt][ct][r] / sqrt(qn[rt][r] * cn) : -inf;  // a zero row is never a partner
        }
        __syncthreads();
        if (walker) {
            const int lo = my_lo > c0 ? my_lo : c0, hi = my_pos < c0 + ND_CN ? my_pos : c0 + ND_CN;
            const double *mine = cosv + t * ND_CS;
            for (int c = lo; c < hi; ++c) {
                const double v = mine[c - c0];
                if (v > top) top = v, arg = c;  // strict: the lowest position keeps a tie
            }
        }
    }
    if (walker) {
        const size_t o = (size_t)perm[my_pos];
        best[o] = top;
        partner[o] = arg >= 0 ? (int64_t)perm[arg] : (int64_t)-1;
    }
}

// what the pair sweeps (acav_rows_neardup_pairs) carry beside k_neardup's arguments.  deg / offsets: by INPUT position
struct NdPairs {
    double threshold;
    int *deg;                // count sweep: the columns of a row's range at cosine >= threshold
    const int64_t *offsets;  // emit sweep [n + 1]: row i's pairs go to [offsets[i], offsets[i + 1])
    int64_t *pair_j;         // emit sweep: the input position of the column
    double *pair_cos;        // emit sweep: its cosine (NULL: not wanted)
    int *mismatch;           // emit sweep: set when a row's count differs from offsets[i + 1] - offsets[i]
};

enum { ND_COUNT = 1, ND_EMIT = 2 };

// the count sweep (MODE ND_COUNT) and the emit sweep (ND_EMIT) of acav_rows_neardup_pairs: k_neardup's arguments, stage loop,
// operands and cosine tile -- a cosine is the same chain in all three.  Count: the walker of a row keeps (top, arg) as k_neardup
// does and counts the columns of its range at cosine >= threshold into pr.deg.  Emit, over the tiles that hold a row with
// pairs: the walker writes those columns in ascending position from offsets[i] on; best and partner are not touched
template <int RT, bool VEC, int MODE>
__global__ __launch_bounds__(256, 2) void k_neardup_pairs(const float *__restrict__ x, int d, int n, const int *__restrict__ perm,
                                                          const int *__restrict__ rstart, const double *__restrict__ nrm,
                                                          const NdTile *__restrict__ tiles, double *__restrict__ best,
                                                          int64_t *__restrict__ partner, const NdPairs pr)
{
    constexpr int QM = ND_QM * RT;
    extern __shared__ double nd_smem[];
    double *cosv = nd_smem;                          // [QM][ND_CS], after the last chunk of a block
    float *qs = reinterpret_cast<float *>(nd_smem);  // [QM][ND_ST]
    float *cs = qs + QM * ND_ST;                     // [ND_CN][ND_ST]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;  // fragment row (A) / column (B) and k index of this lane
    const int lq = t & 7, lr = t >> 3;         // this thread stages columns 4 lq .. 4 lq + 3 of the rows lr + 32 u
    const NdTile tile = tiles[blockIdx.x];
    const int q0 = tile.q0, q1 = tile.q0 + tile.rows;  // q1 <= n
    const double inf = __builtin_inf();

    // the query rows this thread stages, and the ones whose results it holds
    const float *qrow[2 * RT];
    bool qok[2 * RT];
#pragma unroll
    for (int u = 0; u < 2 * RT; ++u) {
        const int q = q0 + lr + 32 * u;
        qok[u] = q < q1;
        qrow[u] = x + (size_t)perm[qok[u] ? q : q0] * d;
    }
    double qn[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
            const int q = q0 + wave * 16 * RT + rt * 16 + fq + 4 * r;
            qn[rt][r] = nrm[q < q1 ? q : q0];
        }
    // the walk: thread t < QM owns query row t of the tile; a zero row has no partner and is none
    const int my_pos = q0 + t;
    const bool walker = t < QM && my_pos < q1;
    const int my_lo = walker && nrm[my_pos] > 0.0 ? rstart[my_pos] : n;  // its columns: the sorted positions [my_lo, my_pos)
    double top = -inf;
    int arg = -1;
    int cnt = 0;              // the columns met so far at cosine >= threshold
    int64_t at = 0, end = 0;  // ND_EMIT: where the next pair goes, and where the row's room ends
    if (MODE == ND_EMIT && walker) {
        const size_t o = (size_t)perm[my_pos];
        at = pr.offsets[o], end = pr.offsets[o + 1];
    }

    for (int cb = tile.cb0; cb < tile.cb0 + tile.blocks; ++cb) {
        const int c0 = cb * ND_CN;  // c0 <= q1 - 1 < n
        const float *crow[2];
        bool cok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int c = c0 + lr + 32 * u;
            cok[u] = c < n;
            crow[u] = x + (size_t)perm[cok[u] ? c : c0] * d;
        }
        f64x4 acc[RT][4];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f64x4{0.0, 0.0, 0.0, 0.0};
        float4 pq[2 * RT], pc[2];  // the next chunk, in flight while the current one is multiplied
#pragma unroll
        for (int u = 0; u < 2 * RT; ++u) pq[u] = nd_fetch<VEC>(qrow[u], d, 4 * lq);
#pragma unroll
        for (int u = 0; u < 2; ++u) pc[u] = nd_fetch<VEC>(crow[u], d, 4 * lq);
        for (int j0 = 0; j0 < d; j0 += ND_DK) {
            __syncthreads();  // the previous stage has been read (and the previous block's cosine tile walked)
#pragma unroll
            for (int u = 0; u < 2 * RT; ++u)
                *reinterpret_cast<float4 *>(&qs[(lr + 32 * u) * ND_ST + 4 * lq]) = nd_mask(pq[u], qok[u], d, j0 + 4 * lq);
#pragma unroll
            for (int u = 0; u < 2; ++u)
                *reinterpret_cast<float4 *>(&cs[(lr + 32 * u) * ND_ST + 4 * lq]) = nd_mask(pc[u], cok[u], d, j0 + 4 * lq);
            __syncthreads();
            if (j0 + ND_DK < d) {
#pragma unroll
                for (int u = 0; u < 2 * RT; ++u) pq[u] = nd_fetch<VEC>(qrow[u], d, j0 + ND_DK + 4 * lq);
#pragma unroll
                for (int u = 0; u < 2; ++u) pc[u] = nd_fetch<VEC>(crow[u], d, j0 + ND_DK + 4 * lq);
            }
#pragma unroll
            for (int kk = 0; kk < ND_DK / 4; ++kk) {
                double a[RT], b[4];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = (double)qs[(wave * 16 * RT + rt * 16 + fr) * ND_ST + kk * 4 + fq];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) b[ct] = (double)cs[(ct * 16 + fr) * ND_ST + kk * 4 + fq];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt], b[ct], acc[rt][ct], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave has read the last stage: the cosine tile goes over it
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const int c = c0 + ct * 16 + fr;
            const double cn = nrm[c < n ? c : n - 1];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    cosv[(wave * 16 * RT + rt * 16 + fq + 4 * r) * ND_CS + ct * 16 + fr] =
                        cn > 0.0 ? acc[rt][ct][r] / sqrt(qn[rt][r] * cn) : -inf;  // a zero row is never a partner
        }
        __syncthreads();
        if (walker) {
            const int lo = my_lo > c0 ? my_lo : c0, hi = my_pos < c0 + ND_CN ? my_pos : c0 + ND_CN;
            const double *mine = cosv + t * ND_CS;
            for (int c = lo; c < hi; ++c) {
                const double v = mine[c - c0];
                if (MODE == ND_COUNT && v > top) top = v, arg = c;  // strict: the lowest position keeps a tie
                if (v >= pr.threshold) {
                    if (MODE == ND_EMIT && at + cnt < end) {  // never at or beyond offsets[i + 1], whatever the counts say
                        pr.pair_j[at + cnt] = (int64_t)perm[c];
                        if (pr.pair_cos) pr.pair_cos[at + cnt] = v;
                    }
                    ++cnt;
                }
            }
        }
    }
    if (walker) {
        const size_t o = (size_t)perm[my_pos];
        if (MODE == ND_COUNT) {
            best[o] = top;
            partner[o] = arg >= 0 ? (int64_t)perm[arg] : (int64_t)-1;
            pr.deg[o] = cnt;
        }
        if (MODE == ND_EMIT && (int64_t)cnt != end - at) *pr.mismatch = 1;  // inconsistent inputs: the entry returns ACAV_ESTATE
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

// perm [n]: the positions 0 ... n - 1 by label, stably
void sort_by_label(const std::vector<int64_t> &lab, int64_t n, int k, int *perm)
{
    if ((int64_t)k <= 4 * n + 1024) {  // a counting sort, n + k steps (a million rows: a few ms against the merge sort's 100)
        std::vector<int64_t> at((size_t)k + 1, 0);
        for (int64_t i = 0; i < n; ++i) ++at[(size_t)lab[(size_t)i] + 1];
        for (int b = 0; b < k; ++b) at[(size_t)b + 1] += at[(size_t)b];
        for (int64_t i = 0; i < n; ++i) perm[at[(size_t)lab[(size_t)i]]++] = (int)i;
    } else {  // the same permutation without a table of k entries: k is not limited
        std::iota(perm, perm + n, 0);
        std::stable_sort(perm, perm + n, [&](int a, int b) { return lab[(size_t)a] < lab[(size_t)b]; });
    }
}

template <int RT>
int launch(const NdPlan &plan, bool vec, hipStream_t st, const float *x, int d, int n, const int *perm, const int *rstart,
           const double *nrm, const NdTile *tiles, double *best, int64_t *partner)
{
    // the tile's size, whatever another thread's call asks for: it never lowers it under a pending launch
    const void *fn = vec ? reinterpret_cast<const void *>(k_neardup<RT, true>) : reinterpret_cast<const void *>(k_neardup<RT, false>);
    ACAV_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)neardup_lds(RT)));
    if (vec)
        hipLaunchKernelGGL((k_neardup<RT, true>), dim3((unsigned)plan.tiles), dim3(256), plan.lds, st, x, d, n, perm, rstart, nrm,
                           tiles, best, partner);
    else
        hipLaunchKernelGGL((k_neardup<RT, false>), dim3((unsigned)plan.tiles), dim3(256), plan.lds, st, x, d, n, perm, rstart, nrm,
                           tiles, best, partner);
    ACAV_HIP_TRY(hipGetLastError());
    return ACAV_OK;
}

// one of the two pair sweeps over `count` entries of `tiles`
template <int RT, int MODE>
int launch_pairs(int64_t count, bool vec, hipStream_t st, const float *x, int d, int n, const int *perm, const int *rstart,
                 const double *nrm, const NdTile *tiles, double *best, int64_t *partner, const NdPairs &pr)
{
    const void *fn = vec ? reinterpret_cast<const void *>(k_neardup_pairs<RT, true, MODE>)
                         : reinterpret_cast<const void *>(k_neardup_pairs<RT, false, MODE>);
    ACAV_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)neardup_lds(RT)));
    if (vec)
        hipLaunchKernelGGL((k_neardup_pairs<RT, true, MODE>), dim3((unsigned)count), dim3(256), neardup_lds(RT), st, x, d, n, perm,
                           rstart, nrm, tiles, best, partner, pr);
    else
        hipLaunchKernelGGL((k_neardup_pairs<RT, false, MODE>), dim3((unsigned)count), dim3(256), neardup_lds(RT), st, x, d, n, perm,
                           rstart, nrm, tiles, best, partner, pr);
    ACAV_HIP_TRY(hipGetLastError());
    return ACAV_OK;
}

// the emit sweep's tile list: the entries of the count sweep's list (descending blocks, ties by ascending tile) whose tile
// holds a row with pairs, in that order.  has_pairs [tiles]: by TILE INDEX q0 / H, nonzero when the tile holds such a row.
// Returns the column blocks the kept tiles walk together
int64_t pairs_tiles(const std::vector<NdTile> &list, int rt, const unsigned char *has_pairs, std::vector<NdTile> *kept)
{
    const int qm = ND_QM * rt;
    int64_t blocks = 0;
    kept->clear();
    for (const NdTile &e : list)
        if (has_pairs[e.q0 / qm]) kept->push_back(e), blocks += e.blocks;
    return blocks;
}

// ---- acav_rows_crossdup: the pool piece x [n] against the held-out set y [m]

// the tiles of two label histograms: tile t holds the sorted pool positions [t QM, min(n, (t + 1) QM)) and walks the column
// blocks of y's sorted order that cover [ystart[label of its first row], yend[label of its last row]) -- both arrays being
// label-sorted that is one contiguous range, which holds the run of every row of the tile; it is empty (0 blocks, first block
// floor(ystart / 64)) when none of the tile's labels has a held-out row.  list (NULL: skipped): the tiles by descending blocks,
// ties by ascending t.  Returns the plan.
NdPlan crossdup_tiles(const int64_t *hist_x, const int64_t *hist_y, int k, int d, int cus, std::vector<NdTile> *list)
{
    (void)d;
    int64_t n = 0, m = 0;
    for (int b = 0; b < k; ++b) n += hist_x[b], m += hist_y[b];
    NdPlan p;
    p.rt = neardup_rt(n, cus);
    const int64_t qm = (int64_t)ND_QM * p.rt;
    p.tiles = (n + qm - 1) / qm;
    p.blocks = 0;
    if (list) list->clear(), list->reserve((size_t)p.tiles);
    int b = 0;
    int64_t xs = 0, ys = 0;  // the starts of label b's runs in x and in y; b: the label of the tile's first row
    for (int64_t t = 0; t < p.tiles; ++t) {
        const int64_t q0 = t * qm, q1 = std::min(n, q0 + qm);
        while (xs + hist_x[b] <= q0) xs += hist_x[b], ys += hist_y[b], ++b;
        int e = b;  // the label of the tile's last row, xe and ye the ends of its runs
        int64_t xe = xs + hist_x[b], ye = ys + hist_y[b];
        while (xe < q1) ++e, xe += hist_x[e], ye += hist_y[e];
        const int64_t cb0 = ys / ND_CN, blocks = ye > ys ? (ye + ND_CN - 1) / ND_CN - cb0 : 0;
        p.blocks += blocks;
        if (list) list->push_back(NdTile{(int)q0, (int)(q1 - q0), (int)cb0, (int)blocks});
    }
    if (list) std::stable_sort(list->begin(), list->end(), [](const NdTile &a, const NdTile &c) { return a.blocks > c.blocks; });
    p.lds = neardup_lds(p.rt);
    // the sorted positions of both arrays and the two bounds per pool row, the norms, the tile list, (best, partner)
    p.scratch = sizeof(int) * (3 * (size_t)n + (size_t)m) + sizeof(double) * (size_t)(n + m) + sizeof(NdTile) * (size_t)p.tiles +
                (sizeof(double) + sizeof(int64_t)) * (size_t)n;
    return p;
}

// permx[q] / permy[c]: the input position of sorted position q of x / c of y; ylo[q], yhi[q]: the run of q's label in y's sorted
// order; nrmx / nrmy: ||.||^2 by sorted position.  tiles[b]: the tile workgroup b takes.  best / partner: by INPUT position of
// x, partner an input position of y.  k_neardup's stages, operands and accumulators; positions past 2^31 - 64 are compared
// unsigned.  ENTRY (acav_rows_probedup): the sorted positions are (probed cluster, row) entries, permx[q] the row of entry q,
// and best / partner are kept by ENTRY q for k_pd_fold
template <int RT, bool VEC, bool ENTRY = false>
__global__ __launch_bounds__(256, 2) void k_crossdup(const float *__restrict__ x, const float *__restrict__ y, int d, int m,
                                                     const int *__restrict__ permx, const int *__restrict__ permy,
                                                     const int *__restrict__ ylo, const int *__restrict__ yhi,
                                                     const double *__restrict__ nrmx, const double *__restrict__ nrmy,
                                                     const NdTile *__restrict__ tiles, double *__restrict__ best,
                                                     int64_t *__restrict__ partner)
{
    constexpr int QM = ND_QM * RT;
    extern __shared__ double nd_smem[];
    double *cosv = nd_smem;                          // [QM][ND_CS], after the last chunk of a block
    float *qs = reinterpret_cast<float *>(nd_smem);  // [QM][ND_ST]
    float *cs = qs + QM * ND_ST;                     // [ND_CN][ND_ST]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;  // fragment row (A) / column (B) and k index of this lane
    const int lq = t & 7, lr = t >> 3;         // this thread stages columns 4 lq .. 4 lq + 3 of the rows lr + 32 u
    const NdTile tile = tiles[blockIdx.x];
    const unsigned q0 = (unsigned)tile.q0, q1 = q0 + (unsigned)tile.rows, um = (unsigned)m;  // q1 <= n
    const double inf = __builtin_inf();

    // the pool rows this thread stages, and the ones whose results it holds
    const float *qrow[2 * RT];
    bool qok[2 * RT];
#pragma unroll
    for (int u = 0; u < 2 * RT; ++u) {
        const unsigned q = q0 + lr + 32 * u;
        qok[u] = q < q1;
        qrow[u] = x + (size_t)permx[qok[u] ? q : q0] * d;
    }
    double qn[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
            const unsigned q = q0 + wave * 16 * RT + rt * 16 + fq + 4 * r;
            qn[rt][r] = nrmx[q < q1 ? q : q0];
        }
    // the walk: thread t < QM owns pool row t of the tile; a zero row has no partner
    const unsigned my_pos = q0 + t;
    const bool walker = t < QM && my_pos < q1;
    const bool alive = walker && nrmx[my_pos] > 0.0;
    const unsigned my_lo = alive ? (unsigned)ylo[my_pos] : 0u, my_hi = alive ? (unsigned)yhi[my_pos] : 0u;  // its columns
    double top = -inf;
    int arg = -1;

    for (int cb = tile.cb0; cb < tile.cb0 + tile.blocks; ++cb) {
        const unsigned c0 = (unsigned)cb * ND_CN;  // c0 < yhi of the tile's last row <= m
        const float *crow[2];
        bool cok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const unsigned c = c0 + lr + 32 * u;
            cok[u] = c < um;
            crow[u] = y + (size_t)permy[cok[u] ? c : c0] * d;
        }
        f64x4 acc[RT][4];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = f64x4{0.0, 0.0, 0.0, 0.0};
        float4 pq[2 * RT], pc[2];  // the next chunk, in flight while the current one is multiplied
#pragma unroll
        for (int u = 0; u < 2 * RT; ++u) pq[u] = nd_fetch<VEC>(qrow[u], d, 4 * lq);
#pragma unroll
        for (int u = 0; u < 2; ++u) pc[u] = nd_fetch<VEC>(crow[u], d, 4 * lq);
        for (int j0 = 0; j0 < d; j0 += ND_DK) {
            __syncthreads();  // the previous stage has been read (and the previous block's cosine tile walked)
#pragma unroll
            for (int u = 0; u < 2 * RT; ++u)
                *reinterpret_cast<float4 *>(&qs[(lr + 32 * u) * ND_ST + 4 * lq]) = nd_mask(pq[u], qok[u], d, j0 + 4 * lq);
#pragma unroll
            for (int u = 0; u < 2; ++u)
                *reinterpret_cast<float4 *>(&cs[(lr + 32 * u) * ND_ST + 4 * lq]) = nd_mask(pc[u], cok[u], d, j0 + 4 * lq);
            __syncthreads();
            if (j0 + ND_DK < d) {
#pragma unroll
                for (int u = 0; u < 2 * RT; ++u) pq[u] = nd_fetch<VEC>(qrow[u], d, j0 + ND_DK + 4 * lq);
#pragma unroll
                for (int u = 0; u < 2; ++u) pc[u] = nd_fetch<VEC>(crow[u], d, j0 + ND_DK + 4 * lq);
            }
#pragma unroll
            for (int kk = 0; kk < ND_DK / 4; ++kk) {
                double a[RT], b[4];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = (double)qs[(wave * 16 * RT + rt * 16 + fr) * ND_ST + kk * 4 + fq];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) b[ct] = (double)cs[(ct * 16 + fr) * ND_ST + kk * 4 + fq];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[rt], b[ct], acc[rt][ct], 0, 0, 0);
            }
        }
        __syncthreads();  // every wave has read the last stage: the cosine tile goes over it
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            const unsigned c = c0 + ct * 16 + fr;
            const double cn = nrmy[c < um ? c : um - 1];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    cosv[(wave * 16 * RT + rt * 16 + fq + 4 * r) * ND_CS + ct * 16 + fr] =
                        cn > 0.0 ? acc[rt][ct][r] / sqrt(qn[rt][r] * cn) : -inf;  // a zero row is never a partner
        }
        __syncthreads();
        if (walker) {
            const unsigned lo = my_lo > c0 ? my_lo : c0, hi = my_hi < c0 + ND_CN ? my_hi : c0 + ND_CN;
            const double *mine = cosv + t * ND_CS;
            for (unsigned c = lo; c < hi; ++c) {
                const double v = mine[c - c0];
                if (v > top) top = v, arg = (int)c;  // strict: the lowest position keeps a tie
            }
        }
    }
    if (walker) {
        const size_t o = ENTRY ? (size_t)my_pos : (size_t)permx[my_pos];
        best[o] = top;
        partner[o] = arg >= 0 ? (int64_t)permy[arg] : (int64_t)-1;
    }
}

template <int RT, bool ENTRY = false>
int launch_cross(const NdPlan &plan, bool vec, hipStream_t st, const float *x, const float *y, int d, int m, const int *permx,
                 const int *permy, const int *ylo, const int *yhi, const double *nrmx, const double *nrmy, const NdTile *tiles,
                 double *best, int64_t *partner)
{
    const void *fn = vec ? reinterpret_cast<const void *>(k_crossdup<RT, true, ENTRY>)
                         : reinterpret_cast<const void *>(k_crossdup<RT, false, ENTRY>);
    ACAV_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)neardup_lds(RT)));
    if (vec)
        hipLaunchKernelGGL((k_crossdup<RT, true, ENTRY>), dim3((unsigned)plan.tiles), dim3(256), plan.lds, st, x, y, d, m, permx, permy,
                           ylo, yhi, nrmx, nrmy, tiles, best, partner);
    else
        hipLaunchKernelGGL((k_crossdup<RT, false, ENTRY>), dim3((unsigned)plan.tiles), dim3(256), plan.lds, st, x, y, d, m, permx, permy,
                           ylo, yhi, nrmx, nrmy, tiles, best, partner);
    ACAV_HIP_TRY(hipGetLastError());
    return ACAV_OK;
}

// ---- acav_rows_probedup: the rows of x [n] against the rows of y [my] in the m probed clusters of each

// the queries of a probe sweep.  An ENTRY is a (probed cluster c, row i) pair; the entries are sorted by c, then by i, so that
// -- y being label-sorted -- consecutive entries walk the same run of y.  Per entry: the row, and its column range [lo, hi) in
// y's sorted order, lo = ystart[c], hi = lo + (the rows of y labelled c at input positions below before[i]; all when before is
// NULL): ascending sorted position being ascending input position inside a run, that is a prefix of the run
struct PdEntries {
    std::vector<int> erow, elo, ehi;  // [entries]
    std::vector<int> eidx;            // [n][m]: the entry of slot p of row i; -1 for a -1 slot and for a label repeated in the list
    std::vector<int> permy;           // [my]: y's positions by label, stably
    int64_t pairs = 0;                // sum of hi - lo
};

// ACAV_EINVAL for a probe outside [-1, k) or a label of y outside [0, k): checked before anything is indexed with one
int probedup_entries(const int64_t *probes, int64_t n, int m, const std::vector<int64_t> &laby, int64_t my, const int64_t *before, int k,
                     PdEntries *E)
{
    int64_t bad = 0;
    for (int64_t j = 0; j < my; ++j) bad += (laby[(size_t)j] < 0 || laby[(size_t)j] >= k) ? 1 : 0;
    ACAV_REQUIRE(bad == 0, ACAV_EINVAL, "%lld of the %lld labels of y are outside [0, %d)", (long long)bad, (long long)my, k);
    for (int64_t c = 0; c < n * m; ++c) bad += (probes[c] < -1 || probes[c] >= k) ? 1 : 0;
    ACAV_REQUIRE(bad == 0, ACAV_EINVAL, "%lld of the %lld x %d probes of x are outside [-1, %d)", (long long)bad, (long long)n, m, k);
    E->permy.resize((size_t)my);
    sort_by_label(laby, my, k, E->permy.data());

    // the cells (i, p) that are entries, in (i, p) order, and their clusters; then the order by cluster, stably: by i inside one
    std::vector<int64_t> key;
    std::vector<int> cell;
    key.reserve((size_t)(n * m)), cell.reserve((size_t)(n * m));
    for (int64_t i = 0; i < n; ++i)
        for (int p = 0; p < m; ++p) {
            const int64_t c = probes[i * m + p];
            bool entry = c >= 0;
            for (int q = 0; entry && q < p; ++q) entry = probes[i * m + q] != c;  // a repeated label counts once, at its first slot
            if (entry) key.push_back(c), cell.push_back((int)(i * m + p));
        }
    const int64_t ne = (int64_t)key.size();
    std::vector<int> order((size_t)ne);
    sort_by_label(key, ne, k, order.data());
    E->erow.resize((size_t)ne), E->elo.resize((size_t)ne), E->ehi.resize((size_t)ne);
    E->eidx.assign((size_t)(n * m), -1);
    E->pairs = 0;
    const int *py = E->permy.data();
    int64_t ys = 0, ye = 0, cur = -1;  // the run of cluster `cur` in y's sorted order
    for (int64_t e = 0; e < ne; ++e) {
        const int at = order[(size_t)e], cl = cell[(size_t)at];
        const int64_t c = key[(size_t)at], i = cl / m;
        if (c != cur) {
            for (ys = ye; ys < my && laby[(size_t)py[ys]] < c; ++ys) {}
            for (ye = ys; ye < my && laby[(size_t)py[ye]] == c; ++ye) {}
            cur = c;
        }
        const int64_t r = before ? std::lower_bound(py + ys, py + ye, before[i], [](int a, int64_t b) { return (int64_t)a < b; }) - (py + ys)
                                 : ye - ys;
        E->erow[(size_t)e] = (int)i, E->elo[(size_t)e] = (int)ys, E->ehi[(size_t)e] = (int)(ys + r);
        E->eidx[(size_t)cl] = (int)e;
        E->pairs += r;
    }
    return ACAV_OK;
}

// the tiles of the entries: tile t holds the entries [t QM, min(entries, (t + 1) QM)) and walks the column blocks of y's sorted
// order from the first one any of its non-empty ranges touches to the last one (lo does not decrease along the entries: the
// first non-empty range has the lowest lo); 0 blocks, at first block floor(lo of its first entry / 64), when all its ranges are
// empty.  list (NULL: skipped): the tiles by descending blocks, ties by ascending t.  Returns the plan.
NdPlan probedup_tiles(const PdEntries &E, int64_t n, int m, int64_t my, int cus, std::vector<NdTile> *list)
{
    const int64_t ne = (int64_t)E.erow.size();
    NdPlan p;
    p.rt = neardup_rt(ne, cus);
    const int64_t qm = (int64_t)ND_QM * p.rt;
    p.tiles = (ne + qm - 1) / qm;
    p.blocks = 0;
    if (list) list->clear(), list->reserve((size_t)p.tiles);
    for (int64_t t = 0; t < p.tiles; ++t) {
        const int64_t q0 = t * qm, q1 = std::min(ne, q0 + qm);
        int64_t first = -1, end = 0;
        for (int64_t e = q0; e < q1; ++e)
            if (E.ehi[(size_t)e] > E.elo[(size_t)e]) {
                if (first < 0) first = E.elo[(size_t)e] / ND_CN;
                end = std::max<int64_t>(end, (E.ehi[(size_t)e] + ND_CN - 1) / ND_CN);
            }
        const int64_t cb0 = first < 0 ? E.elo[(size_t)q0] / ND_CN : first, blocks = first < 0 ? 0 : end - first;
        p.blocks += blocks;
        if (list) list->push_back(NdTile{(int)q0, (int)(q1 - q0), (int)cb0, (int)blocks});
    }
    if (list) std::stable_sort(list->begin(), list->end(), [](const NdTile &a, const NdTile &c) { return a.blocks > c.blocks; });
    p.lds = neardup_lds(p.rt);
    // per entry the row and two bounds, y's sorted positions, the entry of every (row, slot); the norms by entry and of y; the
    // tile list; (best, partner) per entry and per row; best_each
    p.scratch = sizeof(int) * (3 * (size_t)ne + (size_t)my + (size_t)(n * m)) + sizeof(double) * (size_t)(ne + my) +
                sizeof(NdTile) * (size_t)p.tiles + (sizeof(double) + sizeof(int64_t)) * (size_t)(ne + n) + sizeof(double) * (size_t)(n * m);
    return p;
}

// one thread per row: its at most m entry results in slot order, the larger cosine first, then the lower position of y
__global__ __launch_bounds__(256) void k_pd_fold(int n, int m, const int *__restrict__ eidx, const double *__restrict__ ebest,
                                                 const int64_t *__restrict__ epartner, double *__restrict__ best,
                                                 int64_t *__restrict__ partner, double *__restrict__ best_each)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double top = -__builtin_inf();
    int64_t arg = -1;
    for (int p = 0; p < m; ++p) {
        const int e = eidx[(size_t)i * m + p];
        const double v = e >= 0 ? ebest[e] : -__builtin_inf();
        const int64_t j = e >= 0 ? epartner[e] : (int64_t)-1;
        if (best_each) best_each[(size_t)i * m + p] = v;
        if (j >= 0 && (v > top || (v == top && j < arg))) top = v, arg = j;
    }
    best[i] = top;
    partner[i] = arg;
}

// count int64 values of p (host or device) on the host
int fetch_i64(const int64_t *p, int64_t count, std::vector<int64_t> *out, hipStream_t st)
{
    out->resize((size_t)count);
    if (is_device_ptr(p)) {
        ACAV_HIP_TRY(hipMemcpyAsync(out->data(), p, sizeof(int64_t) * (size_t)count, hipMemcpyDeviceToHost, st));
        ACAV_HIP_TRY(hipStreamSynchronize(st));
    } else {
        std::copy(p, p + count, out->begin());
    }
    return ACAV_OK;
}

int check_probedup_sizes(int64_t n, int64_t my, int d, int m, int k)
{
    ACAV_REQUIRE(n >= 1 && n <= ND_MAX_N, ACAV_EINVAL, "n=%lld must be in [1, 2^31): positions are 32-bit", (long long)n);
    ACAV_REQUIRE(my >= 1 && my <= ND_MAX_N, ACAV_EINVAL, "my=%lld must be in [1, 2^31): positions are 32-bit", (long long)my);
    ACAV_REQUIRE(d >= 1 && d <= ND_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, ND_MAX_D);
    ACAV_REQUIRE(k >= 1, ACAV_EINVAL, "k=%d must be at least 1", k);
    ACAV_REQUIRE(m >= 1 && m <= ACAV_PROBES_MAX, ACAV_EINVAL, "m=%d must be in [1, %d]", m, ACAV_PROBES_MAX);
    ACAV_REQUIRE(n * m <= ND_MAX_N, ACAV_EINVAL, "n m = %lld entries must be below 2^31: entries are 32-bit", (long long)(n * m));
    return ACAV_OK;
}

int check_hist(const int64_t *hist, int k, const char *what, int64_t *sum)
{
    int64_t n = 0;
    for (int b = 0; b < k; ++b) {
        ACAV_REQUIRE(hist[b] >= 0 && hist[b] <= ND_MAX_N, ACAV_EINVAL, "%s[%d] = %lld must be in [0, 2^31)", what, b, (long long)hist[b]);
        n += hist[b];
        ACAV_REQUIRE(n <= ND_MAX_N, ACAV_EINVAL, "%s holds 2^31 rows or more: positions are 32-bit", what);
    }
    ACAV_REQUIRE(n >= 1, ACAV_EINVAL, "%s holds no row", what);
    *sum = n;
    return ACAV_OK;
}

// what acav_rows_neardup and acav_rows_neardup_pairs do up to their sweep, and the way their (best, partner) come home: the rows
// and labels on the device, the checks of labels and values, the positions by label with their run starts, the tile list, the
// norms.  Declared AFTER the DevBufs an entry adds: its drain then idles the stream before any of them goes back to the pool
struct NdSetup {
    DevBuf stage_x, stage_lab, bad, ints, nrm, dtiles, obest, opartner;
    StreamDrain drain;      // after the buffers: destroyed before them
    std::vector<int> host;  // perm [n]: the positions by label, stably; rstart [n]: per sorted position the start of its run
    std::vector<NdTile> list;
    NdPlan plan;
    const float *xd = nullptr;
    const int *dperm = nullptr, *drstart = nullptr;
    double *dbest = nullptr;
    int64_t *dpartner = nullptr;
    bool vec = false, best_dev = false, partner_dev = false;

    explicit NdSetup(hipStream_t st) : drain{st} {}

    // ACAV_EINVAL for a label outside [0, k) or a value that is not finite, before anything is indexed with a label
    int prepare(const float *x, int64_t n, int d, const int64_t *labels, int k, int cus, double *best, int64_t *partner, hipStream_t st)
    {
        const void *dx = nullptr, *dl = nullptr;
        const size_t total = (size_t)n * d;
        ACAV_TRY(to_device(x, sizeof(float) * total, stage_x, st, &dx));
        ACAV_TRY(to_device(labels, sizeof(int64_t) * (size_t)n, stage_lab, st, &dl));
        xd = static_cast<const float *>(dx);
        ACAV_TRY(bad.ensure(sizeof(unsigned long long) * 2));  // [0] labels out of range (its low word), [1] values not finite
        ACAV_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(unsigned long long) * 2, st));
        hipLaunchKernelGGL(k_nd_labels, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                           static_cast<const int64_t *>(dl), n, k, bad.as<unsigned>());
        ACAV_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_nd_finite, dim3((unsigned)std::min<size_t>((total + 255) / 256, (size_t)cus * 8)), dim3(256), 0, st, xd,
                           total, bad.as<unsigned long long>() + 1);
        ACAV_HIP_TRY(hipGetLastError());
        unsigned long long nbad[2] = {0, 0};
        std::vector<int64_t> lab((size_t)n);
        ACAV_HIP_TRY(hipMemcpyAsync(nbad, bad.p, sizeof(nbad), hipMemcpyDeviceToHost, st));
        ACAV_HIP_TRY(hipMemcpyAsync(lab.data(), dl, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        ACAV_HIP_TRY(hipStreamSynchronize(st));
        ACAV_REQUIRE(nbad[0] == 0, ACAV_EINVAL, "%llu of %lld labels are outside [0, %d)", nbad[0], (long long)n, k);
        ACAV_REQUIRE(nbad[1] == 0, ACAV_EINVAL, "%llu of the %lld x %d values are not finite (inf or NaN)", nbad[1], (long long)n, d);

        // the positions by label, stably; per sorted position the start of its run; the label histogram for the tile list
        host.resize((size_t)(2 * n));
        int *perm = host.data(), *rstart = perm + n;
        sort_by_label(lab, n, k, perm);
        std::vector<int64_t> runs;  // the histogram without its empty labels: the same tiles
        for (int64_t c = 0, first = 0; c < n; ++c) {
            if (c == 0 || lab[(size_t)perm[c]] != lab[(size_t)perm[c - 1]]) first = c, runs.push_back(0);
            rstart[c] = (int)first;
            ++runs.back();
        }
        plan = neardup_tiles(runs.data(), (int)runs.size(), d, cus, &list);

        best_dev = is_device_ptr(best), partner_dev = is_device_ptr(partner);
        ACAV_TRY(upload(ints, host.data(), sizeof(int) * host.size(), st));
        ACAV_TRY(upload(dtiles, list.data(), sizeof(NdTile) * list.size(), st));
        ACAV_TRY(nrm.ensure(sizeof(double) * (size_t)n));
        if (!best_dev) ACAV_TRY(obest.ensure(sizeof(double) * (size_t)n));
        if (!partner_dev) ACAV_TRY(opartner.ensure(sizeof(int64_t) * (size_t)n));
        dbest = best_dev ? best : obest.as<double>();
        dpartner = partner_dev ? partner : opartner.as<int64_t>();
        dperm = ints.as<int>(), drstart = dperm + n;
        vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(xd) & 15) == 0;
        hipLaunchKernelGGL(k_nd_norms, dim3((unsigned)n), dim3(64), 0, st, xd, d, dperm, nrm.as<double>());
        ACAV_HIP_TRY(hipGetLastError());
        return ACAV_OK;
    }

    // (best, partner) to host pointers, async on st
    int fetch(double *best, int64_t *partner, int64_t n, hipStream_t st)
    {
        if (!best_dev) ACAV_HIP_TRY(hipMemcpyAsync(best, obest.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
        if (!partner_dev) ACAV_HIP_TRY(hipMemcpyAsync(partner, opartner.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        return ACAV_OK;
    }
};

// ---- acav_pairs_cosine: the cosines of a LIST of pairs (i, j) of x [n] -- the confirmation of a pair list in a second view

constexpr int PC_WAVE = 16;           // pairs of a wave per round: the diagonal of one 16 x 16 accumulator
constexpr int PC_WG = 4 * PC_WAVE;    // pairs of a workgroup per round
constexpr int PC_WG_PER_CU = 8;       // the grid stops growing there: 8 x 18 KB of LDS and 32 waves fill a compute unit
constexpr size_t PC_LDS = sizeof(float) * 2 * PC_WG * ND_ST;  // the pair_i rows and the pair_j rows of one stage

struct PcPlan {
    int64_t wgs, rounds;
    size_t scratch;
};

// workgroup b takes the rounds b, b + wgs, ...: round r holds the pairs [64 r, 64 r + 64), in the caller's order
PcPlan paircos_plan(int64_t pairs, int cus)
{
    PcPlan p;
    const int64_t rounds = (pairs + PC_WG - 1) / PC_WG;
    p.wgs = std::min<int64_t>(rounds, (int64_t)cus * PC_WG_PER_CU);
    p.rounds = p.wgs ? (rounds + p.wgs - 1) / p.wgs : 0;
    // host lists staged on the device (16 per pair), a norm per pair end at the most (16), host cosines (8), the two counters
    p.scratch = (size_t)pairs * 40 + 16;
    return p;
}

// indices outside [0, n): counted before anything is indexed with one
__global__ __launch_bounds__(256) void k_pc_indices(const int64_t *__restrict__ pi, const int64_t *__restrict__ pj, int64_t pairs,
                                                    int64_t n, unsigned long long *__restrict__ bad)
{
    unsigned long long mine = 0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < pairs; e += (int64_t)gridDim.x * 256)
        mine += (pi[e] < 0 || pi[e] >= n ? 1ull : 0ull) + (pj[e] < 0 || pj[e] >= n ? 1ull : 0ull);
    if (mine) atomicAdd(bad, mine);
}

// k_nd_norms' chain, one wave at a time over the entries c, c + waves, ...: nrm[c] = ||x[rows[c]]||^2 (rows NULL: row c itself)
__global__ __launch_bounds__(64) void k_pc_norms(const float *__restrict__ x, int d, const int64_t *__restrict__ rows, int64_t count,
                                                 double *__restrict__ nrm)
{
    for (int64_t c = blockIdx.x; c < count; c += gridDim.x) {
        const size_t base = (size_t)(rows ? rows[c] : c) * d;
        double p = 0.0;
        for (int j = threadIdx.x; j < d; j += 64) {
            const double v = (double)x[base + j];
            p = fma(v, v, p);
        }
        for (int o = 32; o >= 1; o >>= 1) p = p + __shfl_xor(p, o);
        if (threadIdx.x == 0) nrm[c] = p;
    }
}

// one wave: 16 pairs per round, the pair_i rows as the A operand and the pair_j rows as the B operand of k_neardup's MFMA chain
// (the same stages of ND_DK columns, zero-filled tails included); only the diagonal of the accumulator is a result: pair p of
// the wave is register p / 4 of the lane with lane & 15 == p and lane >> 4 == p % 4.  na / nb: the norms of the two ends, by
// ROW (by_row) or by pair.  Every index has been checked; the cosines leave by plain vector stores
template <bool VEC>
__global__ __launch_bounds__(256) void k_paircos(const float *__restrict__ x, int d, const int64_t *__restrict__ pi,
                                                 const int64_t *__restrict__ pj, int64_t pairs, const double *__restrict__ na,
                                                 const double *__restrict__ nb, int by_row, int64_t rounds, double *__restrict__ cos)
{
    __shared__ float as[PC_WG * ND_ST];  // [PC_WG][ND_ST]: a stage of the pair_i rows
    __shared__ float bs[PC_WG * ND_ST];  // of the pair_j rows

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int fr = lane & 15, fq = lane >> 4;  // fragment row (A) / column (B) and k index of this lane
    const int lq = t & 7, lr = t >> 3;         // this thread stages columns 4 lq .. 4 lq + 3 of the pairs lr + 32 u
    const double inf = __builtin_inf();

    for (int64_t r = 0; r < rounds; ++r) {
        const int64_t e0 = (r * gridDim.x + blockIdx.x) * PC_WG;
        if (e0 >= pairs) break;  // the same for every thread of the workgroup
        const float *arow[2], *brow[2];
        bool ok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int64_t e = e0 + lr + 32 * u;
            ok[u] = e < pairs;
            arow[u] = x + (size_t)pi[ok[u] ? e : e0] * d;
            brow[u] = x + (size_t)pj[ok[u] ? e : e0] * d;
        }
        f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
        float4 pa[2], pb[2];  // the next chunk, in flight while the current one is multiplied
#pragma unroll
        for (int u = 0; u < 2; ++u) pa[u] = nd_fetch<VEC>(arow[u], d, 4 * lq), pb[u] = nd_fetch<VEC>(brow[u], d, 4 * lq);
        for (int j0 = 0; j0 < d; j0 += ND_DK) {
            __syncthreads();  // the previous stage (of this round or the last) has been read
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                *reinterpret_cast<float4 *>(&as[(lr + 32 * u) * ND_ST + 4 * lq]) = nd_mask(pa[u], ok[u], d, j0 + 4 * lq);
                *reinterpret_cast<float4 *>(&bs[(lr + 32 * u) * ND_ST + 4 * lq]) = nd_mask(pb[u], ok[u], d, j0 + 4 * lq);
            }
            __syncthreads();
            if (j0 + ND_DK < d) {
#pragma unroll
                for (int u = 0; u < 2; ++u)
                    pa[u] = nd_fetch<VEC>(arow[u], d, j0 + ND_DK + 4 * lq), pb[u] = nd_fetch<VEC>(brow[u], d, j0 + ND_DK + 4 * lq);
            }
#pragma unroll
            for (int kk = 0; kk < ND_DK / 4; ++kk) {
                const double a = (double)as[(wave * PC_WAVE + fr) * ND_ST + kk * 4 + fq];
                const double b = (double)bs[(wave * PC_WAVE + fr) * ND_ST + kk * 4 + fq];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
        }
        // C/D of the f64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register; the diagonal element of pair fr
        const int64_t e = e0 + wave * PC_WAVE + fr;
        if (fq == (fr & 3) && e < pairs) {
            const int reg = fr >> 2;
            const double dot = reg == 0 ? acc[0] : reg == 1 ? acc[1] : reg == 2 ? acc[2] : acc[3];
            const double qn = na[by_row ? pi[e] : e], cn = nb[by_row ? pj[e] : e];
            cos[e] = (qn > 0.0 && cn > 0.0) ? dot / sqrt(qn * cn) : -inf;
        }
    }
}

}  // namespace

ACAV_EXPORT int acav_rows_neardup_plan(const int64_t *hist, int k, int d, int cus, int64_t *out, int64_t *tiles, int64_t cap)
{
    ACAV_REQUIRE(hist && out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(k >= 1 && d >= 1 && d <= ND_MAX_D && cus > 0, ACAV_EINVAL, "bad sizes");
    int64_t n = 0;
    for (int b = 0; b < k; ++b) {
        ACAV_REQUIRE(hist[b] >= 0 && hist[b] <= ND_MAX_N, ACAV_EINVAL, "hist[%d] = %lld must be in [0, 2^31)", b, (long long)hist[b]);
        n += hist[b];
        ACAV_REQUIRE(n <= ND_MAX_N, ACAV_EINVAL, "the histogram holds 2^31 rows or more: positions are 32-bit");
    }
    ACAV_REQUIRE(n >= 1, ACAV_EINVAL, "the histogram holds no row");
    std::vector<NdTile> list;
    const NdPlan p = neardup_tiles(hist, k, d, cus, tiles ? &list : nullptr);
    ACAV_REQUIRE(!tiles || cap >= p.tiles, ACAV_EINVAL, "room for %lld tiles, the rows are cut into %lld", (long long)cap, (long long)p.tiles);
    out[0] = (int64_t)ND_QM * p.rt, out[1] = p.tiles, out[2] = p.blocks, out[3] = p.tiles, out[4] = (int64_t)p.lds;
    out[5] = (int64_t)p.scratch;
    if (tiles)
        for (int64_t t = 0; t < p.tiles; ++t) {
            const NdTile &e = list[(size_t)t];
            tiles[4 * t] = e.q0, tiles[4 * t + 1] = e.rows, tiles[4 * t + 2] = e.cb0, tiles[4 * t + 3] = e.blocks;
        }
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_neardup(int device, const float *x, int64_t n, int d, const int64_t *labels, int k, double *best,
                                  int64_t *partner, void *stream)
{
    ACAV_REQUIRE(x && labels && best && partner, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 1 && n <= ND_MAX_N, ACAV_EINVAL, "n=%lld must be in [1, 2^31): positions are 32-bit", (long long)n);
    ACAV_REQUIRE(d >= 1 && d <= ND_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, ND_MAX_D);
    ACAV_REQUIRE(k >= 1, ACAV_EINVAL, "k=%d must be at least 1", k);
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);

    NdSetup S(st);
    ACAV_TRY(S.prepare(x, n, d, labels, k, cus, best, partner, st));
    if (S.plan.rt == 2)
        ACAV_TRY(launch<2>(S.plan, S.vec, st, S.xd, d, (int)n, S.dperm, S.drstart, S.nrm.as<double>(), S.dtiles.as<NdTile>(), S.dbest,
                           S.dpartner));
    else
        ACAV_TRY(launch<1>(S.plan, S.vec, st, S.xd, d, (int)n, S.dperm, S.drstart, S.nrm.as<double>(), S.dtiles.as<NdTile>(), S.dbest,
                           S.dpartner));
    ACAV_TRY(S.fetch(best, partner, n, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_neardup_pairs_plan(const int64_t *hist, int k, int d, int cus, const unsigned char *has_pairs, int64_t *out,
                                             int64_t *tiles, int64_t cap)
{
    ACAV_REQUIRE(hist && out && has_pairs, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(k >= 1 && d >= 1 && d <= ND_MAX_D && cus > 0, ACAV_EINVAL, "bad sizes");
    int64_t n = 0;
    ACAV_TRY(check_hist(hist, k, "hist", &n));
    std::vector<NdTile> list, kept;
    const NdPlan p = neardup_tiles(hist, k, d, cus, &list);
    const int64_t blocks = pairs_tiles(list, p.rt, has_pairs, &kept);
    const int64_t emit = (int64_t)kept.size();
    ACAV_REQUIRE(!tiles || cap >= emit, ACAV_EINVAL, "room for %lld tiles, the emit sweep launches %lld", (long long)cap, (long long)emit);
    out[0] = (int64_t)ND_QM * p.rt, out[1] = p.tiles, out[2] = p.blocks, out[3] = emit, out[4] = blocks, out[5] = (int64_t)p.lds;
    // the count sweep's scratch, a degree per row and the offsets; the pairs themselves are the caller's
    out[6] = (int64_t)(p.scratch + sizeof(int) * (size_t)n + sizeof(int64_t) * ((size_t)n + 1) + sizeof(NdTile) * (size_t)emit);
    if (tiles)
        for (int64_t t = 0; t < emit; ++t) {
            const NdTile &e = kept[(size_t)t];
            tiles[4 * t] = e.q0, tiles[4 * t + 1] = e.rows, tiles[4 * t + 2] = e.cb0, tiles[4 * t + 3] = e.blocks;
        }
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_neardup_pairs(int device, const float *x, int64_t n, int d, const int64_t *labels, int k, double threshold,
                                        double *best, int64_t *partner, int64_t *offsets, int64_t cap, int64_t *pair_j,
                                        double *pair_cos, void *stream)
{
    ACAV_REQUIRE(x && labels && best && partner && offsets, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 1 && n <= ND_MAX_N, ACAV_EINVAL, "n=%lld must be in [1, 2^31): positions are 32-bit", (long long)n);
    ACAV_REQUIRE(d >= 1 && d <= ND_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, ND_MAX_D);
    ACAV_REQUIRE(k >= 1, ACAV_EINVAL, "k=%d must be at least 1", k);
    ACAV_REQUIRE(threshold > 0.0 && threshold <= 1.0, ACAV_EINVAL, "threshold=%g must be in (0, 1]", threshold);  // a NaN fails too
    ACAV_REQUIRE(cap >= 0, ACAV_EINVAL, "cap=%lld must not be negative", (long long)cap);
    ACAV_REQUIRE(cap == 0 || pair_j, ACAV_EINVAL, "cap=%lld with a NULL pair_j: room for pairs needs a place for them", (long long)cap);
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);

    DevBuf ddeg, doff, dkept, opj, opc, dflag;
    NdSetup S(st);  // after them: its drain idles the stream first
    ACAV_TRY(S.prepare(x, n, d, labels, k, cus, best, partner, st));
    const NdPlan &plan = S.plan;
    const std::vector<NdTile> &list = S.list;
    const int *perm = S.host.data();
    const float *xd = S.xd;
    const int *dperm = S.dperm, *drstart = S.drstart;
    const bool vec = S.vec;
    DevBuf &nrm = S.nrm, &dtiles = S.dtiles;
    ACAV_TRY(ddeg.ensure(sizeof(int) * (size_t)n));
    NdPairs pr = {threshold, ddeg.as<int>(), nullptr, nullptr, nullptr, nullptr};
    if (plan.rt == 2)
        ACAV_TRY((launch_pairs<2, ND_COUNT>(plan.tiles, vec, st, xd, d, (int)n, dperm, drstart, nrm.as<double>(), dtiles.as<NdTile>(),
                                            S.dbest, S.dpartner, pr)));
    else
        ACAV_TRY((launch_pairs<1, ND_COUNT>(plan.tiles, vec, st, xd, d, (int)n, dperm, drstart, nrm.as<double>(), dtiles.as<NdTile>(),
                                            S.dbest, S.dpartner, pr)));
    std::vector<int> deg((size_t)n);
    ACAV_HIP_TRY(hipMemcpyAsync(deg.data(), ddeg.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    ACAV_TRY(S.fetch(best, partner, n, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));

    // the offsets: the exclusive prefix sum of the degrees over INPUT positions
    std::vector<int64_t> off((size_t)n + 1);
    off[0] = 0;
    for (int64_t i = 0; i < n; ++i) off[(size_t)i + 1] = off[(size_t)i] + deg[(size_t)i];
    const int64_t pairs = off[(size_t)n];
    const bool off_dev = is_device_ptr(offsets);
    if (off_dev)
        ACAV_HIP_TRY(hipMemcpyAsync(offsets, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice, st));
    else
        std::copy(off.begin(), off.end(), offsets);
    if (pairs == 0 || pairs > cap) {  // nothing to emit, or no room: the caller compares offsets[n] with cap
        ACAV_HIP_TRY(hipStreamSynchronize(st));
        return ACAV_OK;
    }

    // the emit sweep over the tiles that hold a row with pairs
    const int qm = ND_QM * plan.rt;
    std::vector<unsigned char> has_pairs((size_t)plan.tiles, 0);
    for (int64_t c = 0; c < n; ++c)
        if (deg[(size_t)perm[c]] > 0) has_pairs[(size_t)(c / qm)] = 1;
    std::vector<NdTile> kept;
    pairs_tiles(list, plan.rt, has_pairs.data(), &kept);
    const int64_t *doffsets = offsets;
    if (!off_dev) {
        ACAV_TRY(upload(doff, off.data(), sizeof(int64_t) * off.size(), st));
        doffsets = doff.as<int64_t>();
    }
    ACAV_TRY(upload(dkept, kept.data(), sizeof(NdTile) * kept.size(), st));
    const bool pj_dev = is_device_ptr(pair_j), pc_dev = pair_cos && is_device_ptr(pair_cos);
    if (!pj_dev) ACAV_TRY(opj.ensure(sizeof(int64_t) * (size_t)pairs));
    if (pair_cos && !pc_dev) ACAV_TRY(opc.ensure(sizeof(double) * (size_t)pairs));
    ACAV_TRY(dflag.ensure(sizeof(int)));
    ACAV_HIP_TRY(hipMemsetAsync(dflag.p, 0, sizeof(int), st));
    pr.deg = nullptr, pr.offsets = doffsets, pr.pair_j = pj_dev ? pair_j : opj.as<int64_t>();
    pr.pair_cos = !pair_cos ? nullptr : pc_dev ? pair_cos : opc.as<double>(), pr.mismatch = dflag.as<int>();
    if (plan.rt == 2)
        ACAV_TRY((launch_pairs<2, ND_EMIT>((int64_t)kept.size(), vec, st, xd, d, (int)n, dperm, drstart, nrm.as<double>(),
                                           dkept.as<NdTile>(), nullptr, nullptr, pr)));
    else
        ACAV_TRY((launch_pairs<1, ND_EMIT>((int64_t)kept.size(), vec, st, xd, d, (int)n, dperm, drstart, nrm.as<double>(),
                                           dkept.as<NdTile>(), nullptr, nullptr, pr)));
    int mismatch = 0;
    ACAV_HIP_TRY(hipMemcpyAsync(&mismatch, dflag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    if (!pj_dev) ACAV_HIP_TRY(hipMemcpyAsync(pair_j, opj.p, sizeof(int64_t) * (size_t)pairs, hipMemcpyDeviceToHost, st));
    if (pair_cos && !pc_dev) ACAV_HIP_TRY(hipMemcpyAsync(pair_cos, opc.p, sizeof(double) * (size_t)pairs, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(mismatch == 0, ACAV_ESTATE, "the emit sweep counted other pairs than the count sweep: the rows changed during the call");
    return ACAV_OK;
}

ACAV_EXPORT int acav_pairs_components(int64_t n, const int64_t *offsets, const int64_t *pair_j, int64_t *root)
{
    ACAV_REQUIRE(n >= 1 && offsets && root, ACAV_EINVAL, "n=%lld must be at least 1, offsets and root not NULL", (long long)n);
    ACAV_REQUIRE(offsets[0] == 0, ACAV_EINVAL, "offsets[0] = %lld must be 0", (long long)offsets[0]);
    for (int64_t i = 0; i < n; ++i)
        ACAV_REQUIRE(offsets[i + 1] >= offsets[i], ACAV_EINVAL, "offsets decrease at row %lld", (long long)i);
    const int64_t pairs = offsets[n];
    ACAV_REQUIRE(pairs == 0 || pair_j, ACAV_EINVAL, "%lld pairs and a NULL pair_j", (long long)pairs);
    for (int64_t e = 0; e < pairs; ++e)
        ACAV_REQUIRE(pair_j[e] >= 0 && pair_j[e] < n, ACAV_EINVAL, "pair_j[%lld] = %lld is outside [0, %lld)", (long long)e,
                     (long long)pair_j[e], (long long)n);
    // union-find in a table of its own (root stays untouched until nothing can be refused): path halving, no recursion; the
    // lower root becomes the parent, so a root is the lowest position of its set
    std::vector<int64_t> up((size_t)n);
    std::iota(up.begin(), up.end(), (int64_t)0);
    auto find = [&](int64_t a) {
        while (up[(size_t)a] != a) {
            up[(size_t)a] = up[(size_t)up[(size_t)a]];
            a = up[(size_t)a];
        }
        return a;
    };
    for (int64_t i = 0; i < n; ++i)
        for (int64_t e = offsets[i]; e < offsets[i + 1]; ++e) {
            const int64_t a = find(i), b = find(pair_j[e]);
            if (a != b) up[(size_t)std::max(a, b)] = std::min(a, b);
        }
    for (int64_t i = 0; i < n; ++i) root[i] = find(i);
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_crossdup_plan(const int64_t *hist_x, const int64_t *hist_y, int k, int d, int cus, int64_t *out,
                                        int64_t *tiles, int64_t cap)
{
    ACAV_REQUIRE(hist_x && hist_y && out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(k >= 1 && d >= 1 && d <= ND_MAX_D && cus > 0, ACAV_EINVAL, "bad sizes");
    int64_t n = 0, m = 0;
    ACAV_TRY(check_hist(hist_x, k, "hist_x", &n));
    ACAV_TRY(check_hist(hist_y, k, "hist_y", &m));
    std::vector<NdTile> list;
    const NdPlan p = crossdup_tiles(hist_x, hist_y, k, d, cus, tiles ? &list : nullptr);
    ACAV_REQUIRE(!tiles || cap >= p.tiles, ACAV_EINVAL, "room for %lld tiles, the rows are cut into %lld", (long long)cap, (long long)p.tiles);
    out[0] = (int64_t)ND_QM * p.rt, out[1] = p.tiles, out[2] = p.blocks, out[3] = p.tiles, out[4] = (int64_t)p.lds;
    out[5] = (int64_t)p.scratch;
    if (tiles)
        for (int64_t t = 0; t < p.tiles; ++t) {
            const NdTile &e = list[(size_t)t];
            tiles[4 * t] = e.q0, tiles[4 * t + 1] = e.rows, tiles[4 * t + 2] = e.cb0, tiles[4 * t + 3] = e.blocks;
        }
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_crossdup(int device, const float *x, int64_t n, const float *y, int64_t m, int d, const int64_t *labels_x,
                                   const int64_t *labels_y, int k, double *best, int64_t *partner, void *stream)
{
    ACAV_REQUIRE(x && y && best && partner, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 1 && n <= ND_MAX_N, ACAV_EINVAL, "n=%lld must be in [1, 2^31): positions are 32-bit", (long long)n);
    ACAV_REQUIRE(m >= 1 && m <= ND_MAX_N, ACAV_EINVAL, "m=%lld must be in [1, 2^31): positions are 32-bit", (long long)m);
    ACAV_REQUIRE(d >= 1 && d <= ND_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, ND_MAX_D);
    ACAV_REQUIRE(k >= 1, ACAV_EINVAL, "k=%d must be at least 1", k);
    const bool blocked = labels_x != nullptr;
    ACAV_REQUIRE(blocked == (labels_y != nullptr), ACAV_EINVAL, "labels_x and labels_y go together: both, or neither (no blocking)");
    ACAV_REQUIRE(blocked || k == 1, ACAV_EINVAL, "k=%d without labels: no blocking is k = 1", k);
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);

    DevBuf stage_x, stage_y, stage_lx, stage_ly, bad, ints, nrm, dtiles, obest, opartner;
    StreamDrain drain = {st};
    const void *dx = nullptr, *dy = nullptr, *dlx = nullptr, *dly = nullptr;
    const size_t total_x = (size_t)n * d, total_y = (size_t)m * d;
    ACAV_TRY(to_device(x, sizeof(float) * total_x, stage_x, st, &dx));
    ACAV_TRY(to_device(y, sizeof(float) * total_y, stage_y, st, &dy));
    const float *xd = static_cast<const float *>(dx), *yd = static_cast<const float *>(dy);
    // [0], [1] labels of x, of y out of range (the low words), [2], [3] values of x, of y that are not finite
    ACAV_TRY(bad.ensure(sizeof(unsigned long long) * 4));
    ACAV_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(unsigned long long) * 4, st));
    std::vector<int64_t> labx, laby;
    if (blocked) {
        ACAV_TRY(to_device(labels_x, sizeof(int64_t) * (size_t)n, stage_lx, st, &dlx));
        ACAV_TRY(to_device(labels_y, sizeof(int64_t) * (size_t)m, stage_ly, st, &dly));
        hipLaunchKernelGGL(k_nd_labels, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, st,
                           static_cast<const int64_t *>(dlx), n, k, bad.as<unsigned>());
        ACAV_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_nd_labels, dim3((unsigned)std::min<int64_t>((m + 255) / 256, 4096)), dim3(256), 0, st,
                           static_cast<const int64_t *>(dly), m, k, bad.as<unsigned>() + 2);
        ACAV_HIP_TRY(hipGetLastError());
        labx.resize((size_t)n), laby.resize((size_t)m);
        ACAV_HIP_TRY(hipMemcpyAsync(labx.data(), dlx, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, st));
        ACAV_HIP_TRY(hipMemcpyAsync(laby.data(), dly, sizeof(int64_t) * (size_t)m, hipMemcpyDeviceToHost, st));
    }
    hipLaunchKernelGGL(k_nd_finite, dim3((unsigned)std::min<size_t>((total_x + 255) / 256, (size_t)cus * 8)), dim3(256), 0, st, xd,
                       total_x, bad.as<unsigned long long>() + 2);
    ACAV_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_nd_finite, dim3((unsigned)std::min<size_t>((total_y + 255) / 256, (size_t)cus * 8)), dim3(256), 0, st, yd,
                       total_y, bad.as<unsigned long long>() + 3);
    ACAV_HIP_TRY(hipGetLastError());
    unsigned long long nbad[4] = {0, 0, 0, 0};
    ACAV_HIP_TRY(hipMemcpyAsync(nbad, bad.p, sizeof(nbad), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(nbad[0] == 0, ACAV_EINVAL, "%llu of the %lld labels of x are outside [0, %d)", nbad[0], (long long)n, k);
    ACAV_REQUIRE(nbad[1] == 0, ACAV_EINVAL, "%llu of the %lld labels of y are outside [0, %d)", nbad[1], (long long)m, k);
    ACAV_REQUIRE(nbad[2] == 0, ACAV_EINVAL, "%llu of the %lld x %d values of x are not finite (inf or NaN)", nbad[2], (long long)n, d);
    ACAV_REQUIRE(nbad[3] == 0, ACAV_EINVAL, "%llu of the %lld x %d values of y are not finite (inf or NaN)", nbad[3], (long long)m, d);

    // both arrays' positions by label, stably; per sorted pool position the run of its label in y's sorted order; the two
    // histograms over the labels that occur (in either array, ascending) for the tile list
    std::vector<int> host((size_t)(3 * n + m));
    int *permx = host.data(), *ylo = permx + n, *yhi = ylo + n, *permy = yhi + n;
    std::vector<int64_t> hx, hy;
    if (!blocked) {
        std::iota(permx, permx + n, 0);
        std::iota(permy, permy + m, 0);
        std::fill(ylo, ylo + n, 0);
        std::fill(yhi, yhi + n, (int)m);
        hx.push_back(n), hy.push_back(m);
    } else {
        sort_by_label(labx, n, k, permx);
        sort_by_label(laby, m, k, permy);
        for (int64_t i = 0, j = 0; i < n || j < m;) {
            const int64_t c = i < n && (j >= m || labx[(size_t)permx[i]] <= laby[(size_t)permy[j]]) ? labx[(size_t)permx[i]]
                                                                                                    : laby[(size_t)permy[j]];
            int64_t i1 = i, j1 = j;
            while (i1 < n && labx[(size_t)permx[i1]] == c) ++i1;
            while (j1 < m && laby[(size_t)permy[j1]] == c) ++j1;
            std::fill(ylo + i, ylo + i1, (int)j);
            std::fill(yhi + i, yhi + i1, (int)j1);
            hx.push_back(i1 - i), hy.push_back(j1 - j);
            i = i1, j = j1;
        }
    }
    std::vector<NdTile> list;
    const NdPlan plan = crossdup_tiles(hx.data(), hy.data(), (int)hx.size(), d, cus, &list);

    const bool best_dev = is_device_ptr(best), partner_dev = is_device_ptr(partner);
    ACAV_TRY(upload(ints, host.data(), sizeof(int) * host.size(), st));
    ACAV_TRY(upload(dtiles, list.data(), sizeof(NdTile) * list.size(), st));
    ACAV_TRY(nrm.ensure(sizeof(double) * (size_t)(n + m)));
    if (!best_dev) ACAV_TRY(obest.ensure(sizeof(double) * (size_t)n));
    if (!partner_dev) ACAV_TRY(opartner.ensure(sizeof(int64_t) * (size_t)n));
    double *dbest = best_dev ? best : obest.as<double>();
    int64_t *dpartner = partner_dev ? partner : opartner.as<int64_t>();
    const int *dpermx = ints.as<int>(), *dylo = dpermx + n, *dyhi = dylo + n, *dpermy = dyhi + n;
    double *nrmx = nrm.as<double>(), *nrmy = nrmx + n;
    const bool vec = d % 4 == 0 && ((reinterpret_cast<uintptr_t>(xd) | reinterpret_cast<uintptr_t>(yd)) & 15) == 0;
    hipLaunchKernelGGL(k_nd_norms, dim3((unsigned)n), dim3(64), 0, st, xd, d, dpermx, nrmx);
    ACAV_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_nd_norms, dim3((unsigned)m), dim3(64), 0, st, yd, d, dpermy, nrmy);
    ACAV_HIP_TRY(hipGetLastError());
    if (plan.rt == 2)
        ACAV_TRY(launch_cross<2>(plan, vec, st, xd, yd, d, (int)m, dpermx, dpermy, dylo, dyhi, nrmx, nrmy, dtiles.as<NdTile>(), dbest,
                                 dpartner));
    else
        ACAV_TRY(launch_cross<1>(plan, vec, st, xd, yd, d, (int)m, dpermx, dpermy, dylo, dyhi, nrmx, nrmy, dtiles.as<NdTile>(), dbest,
                                 dpartner));
    if (!best_dev) ACAV_HIP_TRY(hipMemcpyAsync(best, obest.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (!partner_dev) ACAV_HIP_TRY(hipMemcpyAsync(partner, opartner.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_probedup_plan(const int64_t *probes_x, int64_t n, int m, const int64_t *labels_y, int64_t my,
                                        const int64_t *before, int k, int d, int cus, int64_t *out, int64_t *tiles, int64_t cap)
{
    ACAV_REQUIRE(probes_x && labels_y && out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(cus > 0, ACAV_EINVAL, "bad sizes");
    ACAV_TRY(check_probedup_sizes(n, my, d, m, k));
    PdEntries E;
    ACAV_TRY(probedup_entries(probes_x, n, m, std::vector<int64_t>(labels_y, labels_y + my), my, before, k, &E));
    std::vector<NdTile> list;
    const NdPlan p = probedup_tiles(E, n, m, my, cus, tiles ? &list : nullptr);
    ACAV_REQUIRE(!tiles || cap >= p.tiles, ACAV_EINVAL, "room for %lld tiles, the entries are cut into %lld", (long long)cap, (long long)p.tiles);
    out[0] = (int64_t)ND_QM * p.rt, out[1] = p.tiles, out[2] = p.blocks, out[3] = p.tiles, out[4] = (int64_t)p.lds;
    out[5] = (int64_t)p.scratch;
    if (tiles)
        for (int64_t t = 0; t < p.tiles; ++t) {
            const NdTile &e = list[(size_t)t];
            tiles[4 * t] = e.q0, tiles[4 * t + 1] = e.rows, tiles[4 * t + 2] = e.cb0, tiles[4 * t + 3] = e.blocks;
        }
    return ACAV_OK;
}

ACAV_EXPORT int acav_rows_probedup(int device, const float *x, int64_t n, const float *y, int64_t my, int d, const int64_t *probes_x,
                                   int m, const int64_t *labels_y, const int64_t *before, int k, double *best, int64_t *partner,
                                   double *best_each, void *stream)
{
    ACAV_REQUIRE(x && y && probes_x && labels_y && best && partner, ACAV_EINVAL, "NULL argument");
    ACAV_TRY(check_probedup_sizes(n, my, d, m, k));
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);

    DevBuf stage_x, stage_y, bad, ints, nrm, dtiles, eres, obest, opartner, oeach;
    StreamDrain drain = {st};
    const void *dx = nullptr, *dy = nullptr;
    const size_t total_x = (size_t)n * d, total_y = (size_t)my * d, cells = (size_t)n * m;
    ACAV_TRY(to_device(x, sizeof(float) * total_x, stage_x, st, &dx));
    if (y == x && my == n)
        dy = dx;  // the in-set use: one copy
    else
        ACAV_TRY(to_device(y, sizeof(float) * total_y, stage_y, st, &dy));
    const float *xd = static_cast<const float *>(dx), *yd = static_cast<const float *>(dy);
    ACAV_TRY(bad.ensure(sizeof(unsigned long long) * 2));  // values of x, of y that are not finite
    ACAV_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(unsigned long long) * 2, st));
    hipLaunchKernelGGL(k_nd_finite, dim3((unsigned)std::min<size_t>((total_x + 255) / 256, (size_t)cus * 8)), dim3(256), 0, st, xd,
                       total_x, bad.as<unsigned long long>());
    ACAV_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_nd_finite, dim3((unsigned)std::min<size_t>((total_y + 255) / 256, (size_t)cus * 8)), dim3(256), 0, st, yd,
                       total_y, bad.as<unsigned long long>() + 1);
    ACAV_HIP_TRY(hipGetLastError());
    unsigned long long nbad[2] = {0, 0};
    ACAV_HIP_TRY(hipMemcpyAsync(nbad, bad.p, sizeof(nbad), hipMemcpyDeviceToHost, st));
    std::vector<int64_t> probes, laby, cut;
    ACAV_TRY(fetch_i64(probes_x, n * m, &probes, st));
    ACAV_TRY(fetch_i64(labels_y, my, &laby, st));
    if (before) ACAV_TRY(fetch_i64(before, n, &cut, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(nbad[0] == 0, ACAV_EINVAL, "%llu of the %lld x %d values of x are not finite (inf or NaN)", nbad[0], (long long)n, d);
    ACAV_REQUIRE(nbad[1] == 0, ACAV_EINVAL, "%llu of the %lld x %d values of y are not finite (inf or NaN)", nbad[1], (long long)my, d);

    // the entries by (probed cluster, row) with their column ranges, y's positions by label, the tile list: the plan's
    PdEntries E;
    ACAV_TRY(probedup_entries(probes.data(), n, m, laby, my, before ? cut.data() : nullptr, k, &E));
    std::vector<NdTile> list;
    const NdPlan plan = probedup_tiles(E, n, m, my, cus, &list);
    const size_t ne = E.erow.size();

    std::vector<int> host(3 * ne + (size_t)my + cells);
    std::copy(E.erow.begin(), E.erow.end(), host.begin());
    std::copy(E.elo.begin(), E.elo.end(), host.begin() + ne);
    std::copy(E.ehi.begin(), E.ehi.end(), host.begin() + 2 * ne);
    std::copy(E.permy.begin(), E.permy.end(), host.begin() + 3 * ne);
    std::copy(E.eidx.begin(), E.eidx.end(), host.begin() + 3 * ne + (size_t)my);
    const bool best_dev = is_device_ptr(best), partner_dev = is_device_ptr(partner), each_dev = best_each && is_device_ptr(best_each);
    ACAV_TRY(upload(ints, host.data(), sizeof(int) * host.size(), st));
    if (ne) ACAV_TRY(upload(dtiles, list.data(), sizeof(NdTile) * list.size(), st));
    ACAV_TRY(nrm.ensure(sizeof(double) * (ne + (size_t)my)));
    ACAV_TRY(eres.ensure((sizeof(double) + sizeof(int64_t)) * std::max<size_t>(ne, 1)));
    if (!best_dev) ACAV_TRY(obest.ensure(sizeof(double) * (size_t)n));
    if (!partner_dev) ACAV_TRY(opartner.ensure(sizeof(int64_t) * (size_t)n));
    if (best_each && !each_dev) ACAV_TRY(oeach.ensure(sizeof(double) * cells));
    double *dbest = best_dev ? best : obest.as<double>();
    int64_t *dpartner = partner_dev ? partner : opartner.as<int64_t>();
    double *deach = !best_each ? (double *)nullptr : each_dev ? best_each : oeach.as<double>();
    const int *derow = ints.as<int>(), *delo = derow + ne, *dehi = delo + ne, *dpermy = dehi + ne, *deidx = dpermy + my;
    double *nrme = nrm.as<double>(), *nrmy = nrme + ne, *ebest = eres.as<double>();
    int64_t *epartner = reinterpret_cast<int64_t *>(ebest + std::max<size_t>(ne, 1));
    const bool vec = d % 4 == 0 && ((reinterpret_cast<uintptr_t>(xd) | reinterpret_cast<uintptr_t>(yd)) & 15) == 0;
    if (ne) {
        hipLaunchKernelGGL(k_nd_norms, dim3((unsigned)ne), dim3(64), 0, st, xd, d, derow, nrme);  // an entry's norm is its row's
        ACAV_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_nd_norms, dim3((unsigned)my), dim3(64), 0, st, yd, d, dpermy, nrmy);
        ACAV_HIP_TRY(hipGetLastError());
        if (plan.rt == 2)
            ACAV_TRY((launch_cross<2, true>(plan, vec, st, xd, yd, d, (int)my, derow, dpermy, delo, dehi, nrme, nrmy, dtiles.as<NdTile>(),
                                            ebest, epartner)));
        else
            ACAV_TRY((launch_cross<1, true>(plan, vec, st, xd, yd, d, (int)my, derow, dpermy, delo, dehi, nrme, nrmy, dtiles.as<NdTile>(),
                                            ebest, epartner)));
    }
    hipLaunchKernelGGL(k_pd_fold, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int)n, m, deidx, ebest, epartner, dbest, dpartner,
                       deach);
    ACAV_HIP_TRY(hipGetLastError());
    if (!best_dev) ACAV_HIP_TRY(hipMemcpyAsync(best, obest.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (!partner_dev) ACAV_HIP_TRY(hipMemcpyAsync(partner, opartner.p, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (best_each && !each_dev) ACAV_HIP_TRY(hipMemcpyAsync(best_each, oeach.p, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}

ACAV_EXPORT int acav_pairs_cosine_plan(int64_t pairs, int d, int cus, int64_t *out)
{
    ACAV_REQUIRE(out, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(pairs >= 0 && d >= 1 && d <= ND_MAX_D && cus > 0, ACAV_EINVAL, "bad sizes");
    const PcPlan p = paircos_plan(pairs, cus);
    out[0] = PC_WAVE, out[1] = PC_WG, out[2] = p.wgs, out[3] = p.rounds, out[4] = (int64_t)PC_LDS, out[5] = (int64_t)p.scratch;
    return ACAV_OK;
}

ACAV_EXPORT int acav_pairs_cosine(int device, const float *x, int64_t n, int d, const int64_t *pair_i, const int64_t *pair_j,
                                  int64_t pairs, double *cos, void *stream)
{
    ACAV_REQUIRE(x && cos, ACAV_EINVAL, "NULL argument");
    ACAV_REQUIRE(n >= 1 && n <= ND_MAX_N, ACAV_EINVAL, "n=%lld must be in [1, 2^31): positions are 32-bit", (long long)n);
    ACAV_REQUIRE(d >= 1 && d <= ND_MAX_D, ACAV_EINVAL, "d=%d must be in [1, %d]", d, ND_MAX_D);
    ACAV_REQUIRE(pairs >= 0, ACAV_EINVAL, "pairs=%lld must not be negative", (long long)pairs);
    ACAV_REQUIRE(pairs == 0 || (pair_i && pair_j), ACAV_EINVAL, "%lld pairs with a NULL pair_i or pair_j", (long long)pairs);
    if (pairs == 0) return ACAV_OK;
    int cus = 0;
    ACAV_TRY(use_device(device, &cus));
    hipStream_t st = static_cast<hipStream_t>(stream);

    DevBuf stage_x, stage_i, stage_j, bad, nrm, ocos;
    StreamDrain drain = {st};
    const void *dx = nullptr, *di = nullptr, *dj = nullptr;
    const size_t total = (size_t)n * d;
    ACAV_TRY(to_device(x, sizeof(float) * total, stage_x, st, &dx));
    ACAV_TRY(to_device(pair_i, sizeof(int64_t) * (size_t)pairs, stage_i, st, &di));
    ACAV_TRY(to_device(pair_j, sizeof(int64_t) * (size_t)pairs, stage_j, st, &dj));
    const float *xd = static_cast<const float *>(dx);
    const int64_t *pi = static_cast<const int64_t *>(di), *pj = static_cast<const int64_t *>(dj);
    ACAV_TRY(bad.ensure(sizeof(unsigned long long) * 2));  // [0] indices out of range, [1] values not finite
    ACAV_HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(unsigned long long) * 2, st));
    hipLaunchKernelGGL(k_pc_indices, dim3((unsigned)std::min<int64_t>((pairs + 255) / 256, 4096)), dim3(256), 0, st, pi, pj, pairs, n,
                       bad.as<unsigned long long>());
    ACAV_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_nd_finite, dim3((unsigned)std::min<size_t>((total + 255) / 256, (size_t)cus * 8)), dim3(256), 0, st, xd, total,
                       bad.as<unsigned long long>() + 1);
    ACAV_HIP_TRY(hipGetLastError());
    unsigned long long nbad[2] = {0, 0};
    ACAV_HIP_TRY(hipMemcpyAsync(nbad, bad.p, sizeof(nbad), hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    ACAV_REQUIRE(nbad[0] == 0, ACAV_EINVAL, "%llu of the 2 x %lld pair indices are outside [0, %lld)", nbad[0], (long long)pairs,
                 (long long)n);
    ACAV_REQUIRE(nbad[1] == 0, ACAV_EINVAL, "%llu of the %lld x %d values are not finite (inf or NaN)", nbad[1], (long long)n, d);

    // the norms: one per row where that is no more than one per pair end (the rows are then read once, in order), else one per
    // pair end -- the same chain on the same values either way
    const bool by_row = n <= 2 * pairs;
    const int64_t norms = by_row ? n : 2 * pairs;
    ACAV_TRY(nrm.ensure(sizeof(double) * (size_t)norms));
    double *na = nrm.as<double>(), *nb = by_row ? na : na + pairs;
    const int64_t per = by_row ? n : pairs;
    const unsigned waves = (unsigned)std::min<int64_t>(per, (int64_t)1 << 20);
    hipLaunchKernelGGL(k_pc_norms, dim3(waves), dim3(64), 0, st, xd, d, by_row ? (const int64_t *)nullptr : pi, per, na);
    ACAV_HIP_TRY(hipGetLastError());
    if (!by_row) {
        hipLaunchKernelGGL(k_pc_norms, dim3(waves), dim3(64), 0, st, xd, d, pj, per, nb);
        ACAV_HIP_TRY(hipGetLastError());
    }

    const PcPlan plan = paircos_plan(pairs, cus);
    const bool cos_dev = is_device_ptr(cos);
    if (!cos_dev) ACAV_TRY(ocos.ensure(sizeof(double) * (size_t)pairs));
    double *dcos = cos_dev ? cos : ocos.as<double>();
    const bool vec = d % 4 == 0 && (reinterpret_cast<uintptr_t>(xd) & 15) == 0;
    if (vec)
        hipLaunchKernelGGL((k_paircos<true>), dim3((unsigned)plan.wgs), dim3(256), 0, st, xd, d, pi, pj, pairs, na, nb, by_row ? 1 : 0,
                           plan.rounds, dcos);
    else
        hipLaunchKernelGGL((k_paircos<false>), dim3((unsigned)plan.wgs), dim3(256), 0, st, xd, d, pi, pj, pairs, na, nb, by_row ? 1 : 0,
                           plan.rounds, dcos);
    ACAV_HIP_TRY(hipGetLastError());
    if (!cos_dev) ACAV_HIP_TRY(hipMemcpyAsync(cos, ocos.p, sizeof(double) * (size_t)pairs, hipMemcpyDeviceToHost, st));
    ACAV_HIP_TRY(hipStreamSynchronize(st));
    return ACAV_OK;
}
