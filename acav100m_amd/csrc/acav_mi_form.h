// The launch plan of the batch-MI greedy loop (acav_mi.hip: run_greedy_tiled / run_greedy_legacy), each piece ONE pure function of
// the shape and the experiment switches.  Plain C++: no HIP type, no getenv, no handle.
//
//   greedy_plan        how many iterations a chunk runs and how many MT19937 draws their permutations take
//   fy_pick_tiling     the tile table of the tiled Fisher-Yates for a list of L0 candidates
//   mt_pick_lanes      lane blocks, lanes and superblocks of the device generator (MtStream::plan takes its numbers from here)
//   greedy_pick_form   tiled / legacy / refused, the kernel instantiations, their dynamic LDS, the per-chunk iteration plans
//   greedy_group_grids every grid of one group of FY_GROUP iterations
//
// acav_mi.hip fills GreedySwitches (greedy_switches(), on every call) and the shape and turns the form into launches;
// acav_mi_greedy_form() exposes all of it to a machine without a GPU (tests/test_greedy_form.py).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ACAV_FORM_HD __host__ __device__
#else
#define ACAV_FORM_HD
#endif

// ================================================================================================ the selection's LDS
constexpr int SEL_MAXB = 64;      // batch sizes up to here: the NARROW selection (one wave ranks the batch, lane = batch position)
constexpr int SEL_WIDEB = 1024;   // batch sizes up to here: the WIDE selection (the workgroup ranks the batch out of LDS)
constexpr int SEL_MAXBP = 8192;
constexpr int SEL_LDSP = 256;     // pairs (and their running sums) staged in LDS
constexpr int SEL_FASTBP = 2048;  // B * P up to which the scoring's labels / counts are kept for the commit ...
constexpr int SEL_FASTKP = 512;   // ... and k * P up to which the commit's phi values are staged (both: SEL_FAST)
constexpr int SEL_PHIBP = 256;    // B * P up to which the scoring's phi values are kept too (SEL_KEEPPHI)
constexpr int SEL_FAST = 1, SEL_KEEPPHI = 2;
constexpr size_t SEL_LDS_PER_WG = 160 * 1024;  // per workgroup on gfx950

struct SelShared {
    double score[SEL_MAXB];
    double SN[SEL_LDSP], Sa[SEL_LDSP], Sb[SEL_LDSP];
    long long nc;
    unsigned long long used;
    int id[SEL_MAXB], pos[SEL_MAXB], pick[SEL_MAXB];
    int pairs[2 * SEL_LDSP];
};
// the weighted selection (W: acav_mi_set_pair_weights) stages the fp32 pair weights beside the pairs; the unweighted kernels
// keep the LDS footprint of SelShared
struct SelSharedW : SelShared {
    float w[SEL_LDSP];
};

// Dynamic LDS of a selection launch:  scores [B P] f64 | labels + counts 5 x [B P] i32 (SEL_FAST) | scoring's phi [B P][6] f64
// (SEL_KEEPPHI) | commit's phi [k P][6] f64 (SEL_FAST) | label rows [B D] i32.  The mode is decided on the host for the
// largest P and D of the launch; every chunk lays its own sizes out in the same order.
struct SelLayout {
    unsigned off_c, off_phi, off_phik, off_lab, total;
};
ACAV_FORM_HD inline int sel_mode(int B, int P, int k)
{
    const long long bp = (long long)B * P, kp = (long long)k * P;
    const int fast = bp <= SEL_FASTBP && kp <= SEL_FASTKP ? SEL_FAST : 0;
    return fast | (fast && bp <= SEL_PHIBP ? SEL_KEEPPHI : 0);
}
ACAV_FORM_HD inline SelLayout sel_layout(int B, int P, int D, int k, int mode)
{
    const unsigned bp = (unsigned)B * (unsigned)P, kp = (unsigned)k * (unsigned)P;
    SelLayout l;
    l.off_c = 8u * bp;
    l.off_phi = l.off_c + ((mode & SEL_FAST) ? 20u * bp + 4u * (bp & 1u) : 0u);
    l.off_phik = l.off_phi + ((mode & SEL_KEEPPHI) ? 48u * bp : 0u);
    l.off_lab = l.off_phik + ((mode & SEL_FAST) ? 48u * kp : 0u);
    l.total = l.off_lab + 4u * (unsigned)B * (unsigned)D;
    return l;
}
// The WIDE selection (SEL_MAXB < B <= SEL_WIDEB) keeps what SelShared holds per batch position in dynamic LDS instead, behind the
// launch's SelLayout (SelWide in acav_mi.hip): 32 bytes per batch position from here on
ACAV_FORM_HD inline unsigned sel_wide_off(const SelLayout &l) { return (l.total + 7u) & ~7u; }
// dynamic LDS of a selection launch, narrow or wide
ACAV_FORM_HD inline size_t sel_smem_bytes(int B, int P, int D, int k, int mode)
{
    const SelLayout l = sel_layout(B, P, D, k, mode);
    return B > SEL_MAXB ? (size_t)sel_wide_off(l) + 32u * (size_t)B : (size_t)l.total;
}
// a WIDE batch whose label rows [B][D] do not fit one workgroup's LDS beside the rest is refused (the narrow launches keep
// leaving that to the runtime)
inline bool sel_smem_fits(int B, size_t smem) { return B <= SEL_MAXB || smem + sizeof(SelSharedW) <= SEL_LDS_PER_WG; }

// ================================================================================================ the position kernels
#ifndef ACAV_FYA_CH
#define ACAV_FYA_CH 8192
#endif
#ifndef ACAV_FYT_THREADS
#define ACAV_FYT_THREADS 1024
#endif
constexpr int FYA_CH = ACAV_FYA_CH;  // steps per k_fy_part workgroup
constexpr int FYA_THREADS = 1024;
constexpr int64_t FY_TILED_MAX = 16 << 20;
#ifndef ACAV_FY_GROUP
#define ACAV_FY_GROUP 16
#endif
constexpr int FY_GROUP = ACAV_FY_GROUP;  // iterations per launch of the position kernels and per cross-stream hand-off (an event
                                         // wait + record on the content stream costs it ~10 us per group even when long satisfied)
#ifndef ACAV_FY_DEPTH
#define ACAV_FY_DEPTH 3
#endif
constexpr int FY_DEPTH = ACAV_FY_DEPTH;     // groups of perm buffers in flight: the position kernels run up to FY_DEPTH - 1 groups ahead
constexpr int FY_NBUF = FY_DEPTH * FY_GROUP;  // of the gathers (a cross-stream hand-off costs 15-45 us: two deep, both hand-offs
                                              // of a group sat on the critical cycle and left a ~30 us bubble per group)
constexpr int GS_EPT = 4;          // outputs per thread of the gather
// defaults of the gather's XCD subset (gs_block_map; ACAV_GS_XCDS / ACAV_GS_XCD_ROT / ACAV_GS_XCD_MIN_L override them per call).
// Loop at L = 10^6, enqueue + drain us per iteration: 8 XCDs 28.5-29.4, 4 rotating 27.36, 4 fixed 32.38, 2 rotating 34.71, 1
// rotating 51.81.  Crossover, 8 -> 4 rotating: L = 5 10^5 14.5 -> 15.0 / 15.3 and 2.5 10^5
// 11.6 -> 11.9, 6.5 10^5 17.3 -> 18.4 (slower: a list well below an L2 stays resident on all eight), 8 10^5 (the list runs down
// to 7.2 10^5 in the 20 000 iterations measured) 21.97 -> 22.14 / 22.19: the crossover is at about 8 10^5
constexpr int GS_XCDS_DEFAULT = 4;
constexpr bool GS_XCD_ROT_DEFAULT = true;
constexpr long long GS_XCD_MIN_L_DEFAULT = 800000;
constexpr int FY_SHARDS = 8;       // sub-buckets per tile (capg entries each), filled by workgroups b with b % 8 == shard
constexpr int FYT_THREADS = ACAV_FYT_THREADS;  // k_fy_tile: the list walks are chains of dependent LDS reads -- many waves hide them
// Bucket entries in 4 bytes instead of an int2 (step, target) -- half of the bucket stream that k_fy_part writes and k_fy_tile reads
// back (8 of the 16 MB per iteration at L = 10^6).  A part workgroup bx appends to shard bx & 7 only, so the entry only needs
//   [31:26] bx >> 3   [25:13] step - bx * FYA_CH   [12:0] target - q_lo (the tile-local position: tiles are at most 8192 wide)
// which holds for lists of at most 512 part workgroups; longer lists (and ACAV_FY_PACK=0) keep the int2 form.
constexpr int64_t FY_PACK_MAX = FYA_CH <= 8192 ? (int64_t)512 * FYA_CH : 0;
constexpr int FY_XCDS = 8;
constexpr size_t FY_PART_STAGED_LDS = 96 * 1024;  // the staged form of k_fy_part is taken while its LDS stays within this
constexpr int64_t QUEUE_PROBE_MIN_L = 250000;     // the single-chunk list from which the three streams' queues are probed
constexpr int MT_NSLOT = 2;                       // superblocks in the generator's ring
constexpr int64_t MT_BLK_DEFAULT = 624 * 4096;    // 2.5 M words per lane block: ~0.85 ms of generation per hop

struct FyGrid {
    unsigned nx, ny, gz;  // the 3-D grid that the 1-D launch stands for; nx == 0: the launch IS that 3-D grid (ACAV_FY_XCD_AFFINE=0)
};
struct GsGrid {
    unsigned n_xcd, rot;  // rot: the first class of the set, 0..7
};
struct Grid3 {  // a launch grid in plain C++
    unsigned x = 1, y = 1, z = 1;
};

ACAV_FORM_HD inline long long fy_affine_blocks(unsigned nx, unsigned ny, unsigned gz)
{
    const unsigned items = ny * gz;
    return items < (unsigned)FY_XCDS ? (long long)nx * items : (long long)FY_XCDS * nx * ((items + FY_XCDS - 1) / FY_XCDS);
}
// the launch grid of k_fy_tile_multi / k_fy_resolve_multi: 1-D when `affine` and the 1-D grid fits a launch of `threads`-wide workgroups
inline Grid3 fy_launch_grid(bool affine, unsigned nx, unsigned ny, unsigned gz, unsigned threads, FyGrid *gr)
{
    const long long nb = fy_affine_blocks(nx, ny, gz);
    if (affine && nx > 0 && nb > 0 && nb <= 0x7fffffffll && nb * threads < (1ll << 32)) {
        *gr = {nx, ny, gz};
        return {(unsigned)nb, 1u, 1u};
    }
    *gr = {0u, ny, gz};
    return {nx, ny, gz};
}
// bit c: class c gathers
ACAV_FORM_HD inline unsigned gs_class_mask(unsigned n_xcd, unsigned rot)
{
    const unsigned m = ((1u << n_xcd) - 1u) << rot;  // n_xcd <= 8, rot < 8: 15 bits
    return (m | (m >> FY_XCDS)) & ((1u << FY_XCDS) - 1u);
}
// the 1-D grid: the selection, and the shortest row behind it that holds gather_blocks gathering workgroups
ACAV_FORM_HD inline long long gs_grid_blocks(long long gather_blocks, unsigned n_xcd, unsigned rot)
{
    if (gather_blocks <= 0) return 1;
    const unsigned mask = gs_class_mask(n_xcd, rot);
    const long long t = gather_blocks - 1 + (mask & 1u);  // the last one is the t-th (from 0) workgroup of the set, workgroup 0 counted
    unsigned r = (unsigned)(t % n_xcd), c = 0;
    for (;; ++c)
        if (mask >> c & 1u) {
            if (r == 0) break;
            --r;
        }
    return t / n_xcd * FY_XCDS + c + 1;
}
inline size_t fy_part_smem(int NT, size_t ntab, bool staged, bool pack = false)
{
    return sizeof(int) * ((staged ? 3 : 2) + (pack ? 1 : 0)) * (size_t)NT + (staged ? 2 * sizeof(int) * FYA_CH + sizeof(int) * 16 : 0) +
           sizeof(unsigned short) * ntab;
}

// ================================================================================================ the switches
struct GreedySwitches {         // the environment, read on every call of an entry point (greedy_switches() in acav_mi.hip)
    bool legacy = false;        // ACAV_FY_LEGACY=1: the global-atomic Fisher-Yates kernels (run_greedy_legacy), chunks one after another
    bool pack = true;           // ACAV_FY_PACK=0: the 8-byte bucket entries (A/B)
    bool xcd_affine = true;     // ACAV_FY_XCD_AFFINE=0: the 3-D grids of the tile and resolve kernels, every item's workgroups dealt
                                //   over all XCDs (A/B; see fy_block_map)
    int gs_xcds = GS_XCDS_DEFAULT;     // ACAV_GS_XCDS = 1, 2, 4: that many XCDs gather, 8: all of them (no padding); else refused
    const char *gs_xcds_text = nullptr;  //   (the variable as written: the refusal quotes it)
    bool gs_rot = GS_XCD_ROT_DEFAULT;  // ACAV_GS_XCD_ROT=1 moves the set by its size every launch, =0 keeps it at classes 0..n-1
    long long gs_min_l = GS_XCD_MIN_L_DEFAULT;  // ACAV_GS_XCD_MIN_L: the list length of a launch from which the subset form is used
    bool part_direct = false;   // ACAV_FY_PART_DIRECT (any value): k_fy_part without its LDS staging
    int fy_cap = 0;             // ACAV_FY_CAP: experiments: smaller tiles (a power of two in 256 .. 8192; anything else: not set)
    int fy_tiles_min = 0;       // ACAV_FY_TILES_MIN: tiles per iteration the tiling aims for (> 0; default 32)
    int fy_ecap = 0;            // ACAV_FY_ECAP: tests: fewer LDS entries per tile (>= 16), forcing the sub-ranged overload path
    int share_gen = 1;          // ACAV_MI_SHARE_GEN=0: a generator stream per chunk, =n: n streams shared by the chunks of a launch
    bool queue_probe = true;    // ACAV_MI_QUEUE_PROBE=0 skips the queue probe of a long single-chunk run
    bool timing = false;        // ACAV_MI_TIMING (any value): the loop's timing lines on stderr
};

// ================================================================================================ one chunk's plans
// The iteration plan of one chunk: how many iterations the greedy loop runs and how many MT19937 draws their
// permutations take.  Every L_t is known on the host (the list shrinks by dl per iteration: no device feedback).
struct GreedyPlan {
    int64_t iters = 0, draws = 0;
    int64_t short_l = -1;  // >= 0: the list is down to this many candidates, fewer than a batch, with the subset not yet full (ACAV_ERANGE)
};
inline GreedyPlan greedy_plan(int64_t L, int64_t subset, int B, int k, int64_t dl, int64_t max_iters)
{
    GreedyPlan gp;
    int64_t l = L;
    for (int64_t nS = 0; nS < subset && (max_iters < 0 || gp.iters < max_iters); nS += k, l -= dl, ++gp.iters) {
        if (l < B) {
            gp.short_l = l;
            break;
        }
        gp.draws += l > 1 ? l - 1 : 0;
    }
    return gp;
}

// Tiling of the tiled Fisher-Yates for a list of (at most) L0 candidates; see the kernels' header comment.
struct FyPlan {
    int gsh = 4, wcap = 256, ecap = 256, ecap_lds = 256, capg = 512, NT = 0;
    std::vector<unsigned short> table;  // (e >> gsh) -> tile
    std::vector<int> ebound;            // tile t covers e in [ebound[t], ebound[t+1])
    size_t tile_smem() const { return (size_t)wcap * 8 + (size_t)ecap_lds * 8; }
};
inline FyPlan fy_pick_tiling(int64_t L0, const GreedySwitches &sw)
{
    FyPlan fp;
    int cap = 256;
    const int cap_max = sw.fy_cap >= 256 && sw.fy_cap <= 8192 && (sw.fy_cap & (sw.fy_cap - 1)) == 0 ? sw.fy_cap : 8192;
    // at least ~32 tiles per iteration (the kernels take FY_GROUP iterations per launch: hundreds of workgroups); smaller
    // tiles only multiply 1024-thread workgroups with a few hundred entries each (8 x 100k chunks in lockstep: 4.85 us per
    // chunk-iteration at 128 tiles, 4.0 at 32)
    const int tiles_min = sw.fy_tiles_min > 0 ? sw.fy_tiles_min : 32;
    while (cap < cap_max && (int64_t)cap * tiles_min < L0) cap *= 2;
    fp.wcap = fp.ecap = cap;
    // capacity of ONE shard of a tile's bucket: with many k_fy_part workgroups the shards fill evenly (an eighth of
    // the tile's load each, 4x headroom); with few, one shard may receive everything
    fp.capg = (L0 + FYA_CH - 1) / FYA_CH >= 64 ? cap / 2 : 2 * cap;
    fp.gsh = 0;
    while ((1 << fp.gsh) < cap / 16) ++fp.gsh;
    const int gran = 1 << fp.gsh;
    const double limit = 0.7 * fp.ecap, lnL = log((double)L0);
    fp.table.assign((size_t)((L0 + gran - 1) >> fp.gsh) + 1, 0);
    int64_t e = 0;
    while (e < L0) {
        int width = 0;
        double mass = 0.0;
        do {  // expected pulls on the granule [x, x + gran): at most gran * ln(L0 / (x + 1))
            const double x = (double)(e + width);
            const double m = gran * (lnL - log(x + 1.0)) + 1.0;
            if (width > 0 && mass + (m > 0 ? m : 0) > limit) break;
            mass += m > 0 ? m : 0;
            width += gran;
        } while (width < fp.wcap && e + width < L0);
        const int t = (int)fp.ebound.size();
        fp.ebound.push_back((int)e);
        for (int64_t x = e; x < e + width; x += gran) fp.table[(size_t)(x >> fp.gsh)] = (unsigned short)t;
        e += width;
    }
    fp.ebound.push_back((int)e);
    fp.NT = (int)fp.ebound.size() - 1;
    fp.ecap_lds = sw.fy_ecap >= 16 && sw.fy_ecap < fp.ecap ? sw.fy_ecap : fp.ecap;
    return fp;
}

// The device generator of `total_draws` MT19937 words that follow a host state at word `idx` of its block.  span: the most draws
// one acquire() covers.  force_blk / force_W (acav_mt_stream_fill): the caller's lane block length (a multiple of 624) and lane
// count (a power of two) instead of the plan's own; with more than MT_NSLOT superblocks it must keep W blk >= 2 span itself
struct MtLanes {
    int64_t head = 0, blk = 0, S = 0, nblocks = 0, nsuper = 0;
    int W = 1, logW = 0;
    bool wraps = false;
};
inline MtLanes mt_pick_lanes(int64_t total_draws, int idx, int64_t span, int64_t force_blk = 0, int force_W = 0)
{
    MtLanes m;
    m.head = 624 - idx;
    const int64_t gen = total_draws > m.head ? total_draws - m.head : 0;  // words that must be generated past the host block
    if (force_blk > 0) {
        m.blk = force_blk;
        m.nblocks = (gen + m.blk - 1) / m.blk;
        m.W = force_W;
    } else if (gen <= MT_BLK_DEFAULT) {  // a single lane block, cut to size
        m.W = 1;
        m.blk = 624 * ((gen + 623) / 624);
        m.nblocks = gen > 0 ? 1 : 0;
    } else {
        m.blk = MT_BLK_DEFAULT;
        m.nblocks = (gen + m.blk - 1) / m.blk;
        m.W = 1;
        while (m.W < 32 && m.W < m.nblocks) m.W *= 2;
        if ((m.nblocks + m.W - 1) / m.W > MT_NSLOT && (int64_t)m.W * m.blk < 2 * span) {  // a slot must hold what one acquire() covers twice over
            m.blk = 624 * ((2 * span + 624 * (int64_t)m.W - 1) / (624 * (int64_t)m.W));
            m.nblocks = (gen + m.blk - 1) / m.blk;
        }
    }
    while ((1 << m.logW) < m.W) ++m.logW;
    m.S = (int64_t)m.W * m.blk;
    m.nsuper = m.nblocks ? (m.nblocks + m.W - 1) / m.W : 0;
    m.wraps = m.nsuper > MT_NSLOT;
    return m;
}

// ================================================================================================ the launch
struct GreedyShape {
    int nchunks;
    const int64_t *L, *subset;  // [nchunks]
    int B, k;
    bool keep_unselected;
    int64_t max_iters;          // < 0: no cap
    int pmax, dmax;             // the largest P and D of the launch's chunks
    bool weighted;              // some chunk has pair weights: the weighted selection for the whole launch
};
enum GreedyPath { GREEDY_TILED = 0, GREEDY_LEGACY = 1 };
enum GreedyRefusal { GREEDY_OK = 0, GREEDY_BAD_XCDS = 1, GREEDY_SHORT_LIST = 2, GREEDY_LDS = 3 };
struct GreedyForm {
    int path = GREEDY_TILED;  // the path the call takes, or would have taken but for the refusal
    // the call is refused: GREEDY_BAD_XCDS (ACAV_EINVAL), GREEDY_SHORT_LIST (ACAV_ERANGE: chunk `refused_chunk` is down to `short_l`
    // candidates), GREEDY_LDS (ACAV_EINVAL: the wide batch's sel_smem does not fit).  The messages are the caller's (greedy_refuse).
    int refusal = GREEDY_OK, refused_chunk = -1;
    int64_t short_l = -1;
    int nchunks = 0, B = 0, k = 0, pmax = 1, dmax = 1;
    bool keep_unselected = false;
    int64_t dl = 0;         // candidates consumed per iteration
    bool wide = false;      // B > SEL_MAXB: the WIDE instantiations of the resolve and gather + selection kernels
    int bcap = SEL_MAXB;    // batch capacity of tailinv and the batch buffers: the narrow layout up to SEL_MAXB
    bool weighted = false;
    std::vector<int64_t> iters, draws;  // per chunk
    int64_t iters_max = 0, lmax = 0;
    int sel_mode = 0;       // one mode for every chunk of the launch: sized for the largest P and D
    size_t sel_smem = 0;
    // ---- the tiled path only
    bool pack = false, part_staged = false, xcd_affine = true;
    size_t part_smem = 0, tile_smem = 0;
    int ntmax = 1;
    std::vector<FyPlan> tiling;  // per chunk
    // The gather's XCD subset (gs_block_map), single-chunk runs only -- the per-chunk lists of a lockstep launch are a tenth of an
    // L2 and keep their 2-D grid
    int gs_xcds = GS_XCDS_DEFAULT;
    bool gs_rot = GS_XCD_ROT_DEFAULT;
    long long gs_min_l = GS_XCD_MIN_L_DEFAULT;
    bool queue_probe = false;  // ONE chunk over a long list, and the switch: the three streams' queues are worth probing
};

// Legacy: lists beyond FY_TILED_MAX, and ACAV_FY_LEGACY=1; the form then holds the iteration plans only (the chunks run one after
// another, each sized by its own P and D when it launches).
inline GreedyForm greedy_pick_form(const GreedyShape &s, const GreedySwitches &sw)
{
    GreedyForm f;
    f.nchunks = s.nchunks, f.B = s.B, f.k = s.k, f.pmax = s.pmax, f.dmax = s.dmax;
    f.keep_unselected = s.keep_unselected, f.weighted = s.weighted;
    f.dl = s.B - (s.keep_unselected ? s.B - s.k : 0);
    f.wide = s.B > SEL_MAXB;
    f.bcap = f.wide ? s.B : SEL_MAXB;
    bool tiled = !sw.legacy;
    for (int c = 0; c < s.nchunks; ++c) {
        f.lmax = s.L[c] > f.lmax ? s.L[c] : f.lmax;
        tiled = tiled && s.L[c] <= FY_TILED_MAX;
    }
    f.path = tiled ? GREEDY_TILED : GREEDY_LEGACY;
    auto refuse = [&f](int why, int chunk = -1, int64_t short_l = -1) {
        f.refusal = why, f.refused_chunk = chunk, f.short_l = short_l;
        return f;
    };
    if (tiled && !(sw.gs_xcds == 1 || sw.gs_xcds == 2 || sw.gs_xcds == 4 || sw.gs_xcds == 8)) return refuse(GREEDY_BAD_XCDS);
    f.iters.assign((size_t)s.nchunks, 0), f.draws.assign((size_t)s.nchunks, 0);
    for (int c = 0; c < s.nchunks; ++c) {
        const GreedyPlan gp = greedy_plan(s.L[c], s.subset[c], s.B, s.k, f.dl, s.max_iters);
        if (gp.short_l >= 0) return refuse(GREEDY_SHORT_LIST, c, gp.short_l);
        f.iters[(size_t)c] = gp.iters, f.draws[(size_t)c] = gp.draws;
        f.iters_max = gp.iters > f.iters_max ? gp.iters : f.iters_max;
    }
    f.sel_mode = sel_mode(s.B, s.pmax, s.k);
    f.sel_smem = sel_smem_bytes(s.B, s.pmax, s.dmax, s.k, f.sel_mode);
    if (!tiled) return f;
    f.pack = f.lmax <= FY_PACK_MAX && sw.pack;
    f.xcd_affine = sw.xcd_affine;
    f.gs_xcds = sw.gs_xcds, f.gs_rot = sw.gs_rot, f.gs_min_l = sw.gs_min_l;
    f.queue_probe = s.nchunks == 1 && s.L[0] >= QUEUE_PROBE_MIN_L && sw.queue_probe;
    f.tiling.reserve((size_t)s.nchunks);
    size_t part_direct = 0, part_staged = 0;
    for (int c = 0; c < s.nchunks; ++c) {
        f.tiling.push_back(fy_pick_tiling(s.L[c], sw));
        const FyPlan &fp = f.tiling.back();
        f.ntmax = fp.NT > f.ntmax ? fp.NT : f.ntmax;
        const size_t ps = fy_part_smem(fp.NT, fp.table.size(), false, f.pack), pss = fy_part_smem(fp.NT, fp.table.size(), true, f.pack);
        part_direct = ps > part_direct ? ps : part_direct;
        part_staged = pss > part_staged ? pss : part_staged;
        f.tile_smem = fp.tile_smem() > f.tile_smem ? fp.tile_smem() : f.tile_smem;
    }
    // the staged form of k_fy_part wants 64 KB of LDS beside the tile table (which grows with L: 64 KB at 16 Mi candidates)
    f.part_staged = part_staged <= FY_PART_STAGED_LDS && !sw.part_direct;
    f.part_smem = f.part_staged ? part_staged : part_direct;
    if (!sel_smem_fits(s.B, f.sel_smem)) return refuse(GREEDY_LDS);
    return f;
}

// draws that chunk c's iterations [g0, g0 + FY_GROUP) read (0: the chunk is over, or its lists are down to one candidate)
inline int64_t greedy_group_draws(const GreedyForm &f, int64_t L, int c, int64_t g0)
{
    int64_t nd = 0;
    for (int64_t it = g0; it < g0 + FY_GROUP && it < f.iters[(size_t)c]; ++it) {
        const int64_t Lc = L - it * f.dl;
        nd += Lc > 1 ? Lc - 1 : 0;
    }
    return nd;
}

// Every grid of the group of iterations [g0, g0 + gz) of a tiled launch.  The longest list still in play bounds the grids.
struct GreedyGroup {
    unsigned gz = 0;  // iterations in the group: FY_GROUP but for the last, ragged one
    int ge = 0;       // event pair and buffer set of this group
    Grid3 part, tile, resolve;
    FyGrid gr_tile, gr_res;
    bool one_d = false;  // both the tile and the resolve grid are 1-D XCD-affine
    Grid3 gather[FY_GROUP];  // per iteration: (the selection of the iteration before +) the gather
    GsGrid gr_gs[FY_GROUP];
};
// gs_launches_sub: the subset-form gather launches before this group -- the rotation goes on from there; the group's are added
inline GreedyGroup greedy_group_grids(const GreedyForm &f, int64_t g0, long long *gs_launches_sub)
{
    GreedyGroup g;
    const int64_t g1 = g0 + FY_GROUP < f.iters_max ? g0 + FY_GROUP : f.iters_max;
    g.gz = (unsigned)(g1 - g0);
    g.ge = (int)((g0 / FY_GROUP) % FY_DEPTH);
    const int64_t lt = f.lmax - g0 * f.dl;
    const unsigned ny = (unsigned)f.nchunks;
    g.part = {(unsigned)((lt + FYA_CH - 1) / FYA_CH), ny, g.gz};
    g.tile = fy_launch_grid(f.xcd_affine, (unsigned)f.ntmax, ny, g.gz, FYT_THREADS, &g.gr_tile);
    g.resolve = fy_launch_grid(f.xcd_affine, (unsigned)((lt + 255) / 256), ny, g.gz, 256, &g.gr_res);
    g.one_d = g.gr_tile.nx && g.gr_res.nx;
    for (int64_t it = g0; it < g1; ++it) {
        const int64_t lit = f.lmax - it * f.dl, gather_blocks = (lit + 256 * GS_EPT - 1) / (256 * GS_EPT);
        GsGrid &gr = g.gr_gs[it - g0];
        gr = {(unsigned)FY_XCDS, 0u};
        if (f.nchunks == 1 && f.gs_xcds < FY_XCDS && lit >= f.gs_min_l) {
            gr = {(unsigned)f.gs_xcds, f.gs_rot ? (unsigned)(*gs_launches_sub * f.gs_xcds % FY_XCDS) : 0u};
            ++*gs_launches_sub;
        }
        g.gather[it - g0] = {(unsigned)gs_grid_blocks(gather_blocks, gr.n_xcd, gr.rot), ny, 1u};
    }
    return g;
}

// ================================================================================================ the draw sampler
// batch.sampler=draw (acav_mi_run_draw, k_mi_draw in acav_mi.hip): per iteration only the first B steps of randperm's swap loop.
// One workgroup per chunk runs the iterations as a loop inside the kernel; a launch runs at most DRAW_GROUP of them (at a few us
// each: tens of ms per launch, however long the list), ACAV_DRAW_GROUP=<n> lowers that for the tests.
constexpr int DRAW_GROUP = 4096;
constexpr int DRAW_THREADS = 256;
// dynamic LDS behind the selection's: win, dep, tgt, orig, prev [B] i32 each (the swap sequence of one iteration)
constexpr unsigned DRAW_ARRAYS = 5;
constexpr size_t DRAW_STATIC_LDS = sizeof(SelSharedW) + 624 * sizeof(unsigned) + 64;  // + the generator block and a flag, rounded up
ACAV_FORM_HD inline unsigned draw_lds_off(size_t sel_smem) { return ((unsigned)sel_smem + 15u) & ~15u; }
ACAV_FORM_HD inline size_t draw_smem_bytes(size_t sel_smem, int B) { return (size_t)draw_lds_off(sel_smem) + 4u * DRAW_ARRAYS * (size_t)B; }

struct DrawForm {
    int refusal = GREEDY_OK, refused_chunk = -1;  // GREEDY_SHORT_LIST (ACAV_ERANGE) or GREEDY_LDS (ACAV_EINVAL)
    int64_t short_l = -1;
    int nchunks = 0, B = 0, k = 0, pmax = 1, dmax = 1;
    bool keep_unselected = false, wide = false, weighted = false;
    int64_t dl = 0;  // the window start moves by this much per iteration: k (keep_unselected) or B
    int sel_mode = 0;
    size_t sel_smem = 0, smem = 0;  // the selection's dynamic LDS, and the launch's (with the swap arrays)
    int group = DRAW_GROUP;         // iterations per launch
    int64_t iters_max = 0, launches = 0;
    std::vector<int64_t> iters, draws;  // per chunk; draws = iters * B
};
// group_env: ACAV_DRAW_GROUP as a number (<= 0: not set); values above DRAW_GROUP do not raise it
inline DrawForm draw_pick_form(const GreedyShape &s, int group_env)
{
    DrawForm f;
    f.nchunks = s.nchunks, f.B = s.B, f.k = s.k, f.pmax = s.pmax, f.dmax = s.dmax;
    f.keep_unselected = s.keep_unselected, f.weighted = s.weighted;
    f.dl = s.keep_unselected ? s.k : s.B;
    f.wide = s.B > SEL_MAXB;
    f.group = group_env > 0 && group_env < DRAW_GROUP ? group_env : DRAW_GROUP;
    f.iters.assign((size_t)s.nchunks, 0), f.draws.assign((size_t)s.nchunks, 0);
    for (int c = 0; c < s.nchunks; ++c) {
        const GreedyPlan gp = greedy_plan(s.L[c], s.subset[c], s.B, s.k, f.dl, s.max_iters);  // the permutation loop's condition
        if (gp.short_l >= 0) {
            f.refusal = GREEDY_SHORT_LIST, f.refused_chunk = c, f.short_l = gp.short_l;
            return f;
        }
        f.iters[(size_t)c] = gp.iters, f.draws[(size_t)c] = gp.iters * s.B;
        f.iters_max = gp.iters > f.iters_max ? gp.iters : f.iters_max;
    }
    f.sel_mode = sel_mode(s.B, s.pmax, s.k);
    f.sel_smem = sel_smem_bytes(s.B, s.pmax, s.dmax, s.k, f.sel_mode);
    f.smem = draw_smem_bytes(f.sel_smem, s.B);
    if (f.smem + DRAW_STATIC_LDS > SEL_LDS_PER_WG) {
        f.refusal = GREEDY_LDS;
        return f;
    }
    f.launches = (f.iters_max + f.group - 1) / f.group;
    return f;
}
