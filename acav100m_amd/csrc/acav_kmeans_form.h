// The kernel choices of the k-means path, each ONE pure function of the shape, the device's limits and the experiment switches.
// Plain C++: no HIP type, no getenv, no handle.  train_pick_form() below, assign_pick_plan() at the end of the file.
//
// Which persistent kernel an epoch of acav_kmeans_train runs on, how many workgroups that takes and how much LDS each gets:
// acav_kmeans.hip fills the three structs and turns the TrainForm into a launch, acav_kmeans_train_form() exposes the choice to
// a machine without a GPU (tests/test_train_form.py).
//
//   d <= 1024   K <= 256 and the grid fits          narrow   8 centres x 8 rows per workgroup (k_train_persistent)
//               else, in this order                 wide     NCP x 8 centres x 8 rows, two row buffers: the smallest NCP of 2, 4, 8
//                                                            that fits 3/4 of the CUs when other clusterings share the call (a budget),
//                                                            else the smallest that fits all of them
//                 ds = 1024, > 3/4 of the CUs       wide     16 centres x 16 rows (two row passes), one row buffer
//                 nothing fits, ds <= 512           wide     16 x 8, one row buffer, in the LDS the split kernel leaves (shared)
//   d > 1024    first of (NCP, row buffers) =       wide     the tall forms: the waves loop over the 256-column blocks
//                 (1, 2) (1, 1) (2, 2) (2, 1)
//               else d <= 2048, d % 256 = 0,        split    16 x 16, the columns over pairs of workgroups
//                 K >= 512                                   (k_train_persistent_split)
//   otherwise                                       none     the per-step launches
#pragma once
#include <cstddef>
#include <cstdint>

constexpr int TP_NC = 8;       // centres per workgroup of the narrow kernel (and per centre pass of the wide one)
constexpr int TP_NR = 8;       // batch rows per workgroup (per row pass)
constexpr int TP_DS = 1024;    // LDS row stride of the narrow kernel = its widest row
constexpr int TP_MAXB = 32;    // batch rows a sweep covers
constexpr int TPW_SW = 32;     // granules per lane in the wide sweep: up to 64 centre groups
constexpr int TS_NC = 16;      // centres per workgroup of the split kernel
constexpr int TS_NR = 16;      // batch rows per workgroup
constexpr int TS_COLS = 1024;  // columns per workgroup (= TP_DS: the LDS row stride of tp_dma_block / dot_blocks)
// dynamic LDS of a split workgroup: centres and rows (16 x 1024 floats each), norms + counts, [4][4][64] partial sums, the 32 best
// labels; 64 keys of 8 bytes; 64 bytes to spare
constexpr size_t TS_SMEM = sizeof(float) * (size_t)(2 * 16 * TS_COLS + 2 * TS_NC + 4 * 4 * 64 + 32) + 8 * 64 + 64;
constexpr int TRAIN_LDS_PER_CU = 160 * 1024;

struct TrainShape {
    int d, K;
    int64_t b;
    bool aligned;  // the row pointer is 16-byte aligned
};
struct TrainLimits {
    int cus;
    int occ_narrow, occ_split;  // workgroups of the narrow / the split kernel one CU holds
    bool has_budget;            // other clusterings share the call: `room` workgroups may still become co-resident
    int room;
    int share_lds;              // > 0: bytes of LDS the ONE column-split kernel in flight leaves on every CU
};
struct TrainSwitches {          // the environment, read once by the caller (train_switches() in acav_kmeans.hip)
    bool no_persistent = false;  // ACAV_NO_PERSISTENT=1
    bool force_wide = false;     // ACAV_FORCE_WIDE=1: the 16-centre forms for shapes the narrow kernel would take
    bool tall = true;            // ACAV_TALL=0 switches the tall forms off
    int wide_ncp = -1;           // ACAV_WIDE_NCP: only this NCP (2, 4, 8; another value fits nothing); -1 = not set
    int wide_nrp = 0;            // ACAV_WIDE_NRP: 2 forces the two-row-pass form, 1 switches it off
    int split_mink = 512;        // ACAV_SPLIT_MINK: the smallest K the split kernel takes
};

enum TrainKind { TRAIN_NONE = 0, TRAIN_NARROW = 1, TRAIN_WIDE = 2, TRAIN_SPLIT = 3 };
struct TrainForm {
    int kind = TRAIN_NONE;
    int ncp = 1, nrp = 1;   // wide: centre passes (x 8 centres) and row passes (x 8 rows) per workgroup
    bool one_x = false;     // wide: one batch-row buffer instead of two
    bool ragged = false;    // d is no multiple of 256
    int ds = 0;             // wide: LDS row stride = d rounded up to 256 columns
    int gx = 0, gy = 0, gz = 0;
    int smem = 0;           // dynamic LDS bytes per workgroup
    bool shared = false;    // launched BESIDE the split kernel, in the LDS it leaves: books no CUs
    int nwg() const { return gx * gy * gz; }
};

// dynamic LDS of a wide workgroup: its centres and batch rows at stride ds, norms + counts of the centres, `parts` x 64 partial
// sums of the FMA phase, the 32 best labels.  The kernel carves the same terms in the same order.
inline size_t train_wide_lds(int centres, int xrows, int ds, int parts)
{
    return sizeof(float) * ((size_t)(centres + xrows) * ds + 2 * centres + 64 * (size_t)parts + 32);
}

inline TrainForm train_pick_form(const TrainShape &s, const TrainLimits &l, const TrainSwitches &sw)
{
    TrainForm f;
    if (sw.no_persistent || s.d % 4 != 0 || s.b > TP_MAXB || !s.aligned) return f;
    const int ds = (s.d + 255) / 256 * 256, nblk = ds / 256, three_quarters = 3 * l.cus / 4;
    const int room = l.has_budget ? l.room : l.occ_narrow * l.cus;
    f.ragged = (s.d & 255) != 0;
    // a wide form, if its grid has at most 64 centre groups and `max_wg` workgroups and its LDS fits `lds`.  Partial sums: one per
    // centre pass and column block, 4 for the matrix-core tile of 16 centres; `blocks` of them
    auto wide = [&](int ncp, int nrp, bool one_x, int blocks, int max_wg, int lds, bool shared = false) {
        const int gx = (s.K + 8 * ncp - 1) / (8 * ncp), gy = (int)((s.b + 8 * nrp - 1) / (8 * nrp));
        const size_t smem = train_wide_lds(8 * ncp, one_x ? 8 * nrp : 16, ds, (ncp == 2 ? 4 : ncp) * blocks);
        if (gx > 2 * TPW_SW || smem > (size_t)(lds < 0 ? 0 : lds) || gx * gy > max_wg) return false;
        f.kind = TRAIN_WIDE, f.ncp = ncp, f.nrp = nrp, f.one_x = one_x, f.ds = ds, f.gx = gx, f.gy = gy, f.gz = 1, f.smem = (int)smem, f.shared = shared;
        return true;
    };
    const int cu_lds = TRAIN_LDS_PER_CU - 1024;
    if (s.d <= TP_DS) {
        const int gx = (s.K + TP_NC - 1) / TP_NC, gy = (int)((s.b + TP_NR - 1) / TP_NR);
        // the exchange sweep of k_train_persistent reads 2 x 16 centre groups per row: K <= 256
        if (gx <= 32 && !sw.force_wide && gx * gy <= l.occ_narrow * l.cus) {
            if (gx * gy <= room) f.kind = TRAIN_NARROW, f.gx = gx, f.gy = gy, f.gz = 1;
            return f;
        }
        // more 8-centre groups than CUs (K = 1024): NCP x 8 centres per workgroup.  A call for one clustering takes the smallest NCP
        // that fits the device (K = 1024, d = 128: 9.8 us per step on 256 workgroups, 11.4 on 128); with several clusterings in one
        // call (budget) the grids stay within 3/4 of it first, so that two of them run side by side
        bool found = false;
        for (int pass = (sw.wide_ncp >= 0 || !l.has_budget) ? 1 : 0; pass < 2 && !found; ++pass)
            for (int c = 2; c <= 8 && !found; c *= 2)
                if (sw.wide_ncp < 0 || sw.wide_ncp == c) {
                    const int lim = pass == 0 ? three_quarters : l.cus;
                    found = wide(c, 1, false, 4, lim < room ? lim : room, cu_lds);
                }
        // K = 1024 at 768 < d <= 1024 (cfg5): NCP = 2 needs the whole device (64 centre groups x 4 row groups) and more centres
        // per workgroup do not fit next to two row buffers -- the two-row-pass form (16 centres x 16 rows, one row buffer, 64 x 2 =
        // 128 workgroups) lets two clusterings run side by side: 14.x us per step of the PAIR instead of 2 x 13.1.  Also for a LONE
        // clustering (round 6): with the tile on the matrix core the 16 x 16 form costs no more FMA time than 16 x 8 and has half the
        // workgroups in the exchange (K = d = 1024 alone 8.6 vs 9.2 us per step).  ACAV_WIDE_NRP=2 forces it, =1 switches it off (A/B).
        if (ds == TS_COLS && sw.wide_nrp != 1 && sw.wide_ncp < 0 && (sw.wide_nrp == 2 || !found || f.nwg() > three_quarters))
            found |= wide(2, 2, true, nblk, three_quarters < room ? three_quarters : room, cu_lds);
        // Round 6: no CUs left, but the ONE launch in flight is the column-split kernel (a 130 KB workgroup on every CU, 252 + 4
        // registers per lane since the exchange rewrite) -- a 16-centre form with one row buffer fits the LDS it leaves (26 KB at
        // ds = 256) and the register file beside it (231-243 + 4: profiles/r06_train_regs.txt), one workgroup per CU: cfg4's 2048-d
        // and 128-d views train side by side instead of one after the other.
        if (!found && l.share_lds > 0 && ds <= 512) wide(2, 1, true, nblk, l.cus, l.share_lds - 512, true);
        return f;
    }
    // rows wider than 1024 columns (round 4: the real SlowFast widths 1408 / 2304, and d = 2048 below K = 1024): the wide kernel
    // with ONE centre pass per workgroup (or two), its waves looping over the 256-column blocks, one batch-row buffer when two do
    // not fit -- no column split, no hand-off between workgroups.  ACAV_TALL=0 switches it off (A/B against the split kernel /
    // the per-step launches).
    if (sw.tall)
        for (int c = 1; c <= 2; ++c)
            for (int one_x = 0; one_x <= 1; ++one_x)
                if (wide(c, 1, one_x != 0, nblk, l.cus < room ? l.cus : room, cu_lds)) return f;
    // 1024 < d <= 2048 (cfg4's visual view): the columns are split over pairs of workgroups.  Worth it from K = 512 on: below that
    // the per-step launches are as fast -- 14.5 us at K = 256 -- because the two dependent hand-offs of a split step cost more than
    // the launches they replace (ACAV_SPLIT_MINK overrides)
    const int gx = (s.K + TS_NC - 1) / TS_NC, gy = (int)((s.b + TS_NR - 1) / TS_NR);
    if (s.d <= 2 * TS_COLS && !f.ragged && gx <= 2 * TPW_SW && s.K >= sw.split_mink && l.occ_split >= 1 &&
        gx * gy * 2 <= l.occ_split * l.cus && gx * gy * 2 <= (l.has_budget ? l.room : l.occ_split * l.cus))
        f.kind = TRAIN_SPLIT, f.gx = gx, f.gy = gy, f.gz = 2, f.smem = (int)TS_SMEM;
    return f;
}

// ================================================================================================ the assign sweep
// Which kernels one sweep of acav_kmeans_assign launches, on which grids and with how much LDS.  acav_kmeans_assign.hip fills the
// three structs (assign_switches() reads the environment), maps the plan to an instantiation of k_assign_f16_rw
// (assign_filter_kernel) and launches; acav_kmeans_assign_plan() exposes the plan to a machine without a GPU
// (tests/test_assign_plan.py).
//
//   the mean distance is wanted, K < 2, n < 128 or n >= 2^31 - 1,      exact    k_assign_f32 over all rows: the fast form when d % 32 = 0
//     ACAV_ASSIGN_EXACT_ONLY=1, d % 32 = 0 but unaligned rows,                  and the rows are 16-byte aligned, else the guarded one
//     d % 32 != 0 with ACAV_FILTER_PAD=0
//   otherwise                                                          filter   k_assign_f16_rw at fd = d rounded up to 32 columns (zero-
//                                                                               padded copies when d % 32 != 0), then the exact re-check
//     K <= 256                                4 waves, 128-row tiles, schedule 0, centre ring of 2; the epilogue emits the candidates
//                                             of an undecided row in place (EMIT = 2) -> k_assign_cand -> k_assign_f32 over the rest
//     K > 256, fd <= 256                      4 waves, one workgroup per (tile, group) pair (GS) -> k_assign_merge -> emission pass
//     K > 256, fd > 256                       8 waves, 256-row tiles, pairs (GS)               (EMIT = 1) -> k_assign_cand -> k_assign_f32
//     ACAV_ASSIGN_EMIT=1 at K <= 256          the lean filter (EMIT = 0) -> emission pass -> k_assign_cand -> k_assign_f32
//     no candidate path (below)               the lean filter (-> k_assign_merge) -> k_assign_f32 over every undecided row
//
// What the arms of the old nested choice only implied:
//   * the centre ring depth follows the tile: dcr = 3 with 8 waves (one workgroup per CU), 2 with 4 (two per CU);
//   * 8 waves always run schedule 2 (DMA pieces between the MFMAs), 4-wave pairs always schedule 0: ACAV_FILTER_SCHED only
//     reaches the 4-wave tile of K <= 256;
//   * scaled rows (xs) are always read non-temporally: xs => nt, whatever ACAV_FILTER_NT says;
//   * candidates are emitted in place only by ONE group on the 4-wave tile with schedule 0.  The (tile, group) pairs emit through
//     the emission pass.  Every other form has NO candidate path -- ACAV_FILTER_NW=8 or ACAV_FILTER_SCHED=2 at K <= 256,
//     ACAV_FILTER_GS=0 at K > 256, as well as ACAV_ASSIGN_EMIT=0, ACAV_ASSIGN_CAND=0 and n >= 2^27 (slots and pairs share one
//     64-bit allocator word): its undecided rows all go to the f32 list and take the full exact sweep;
//   * the emission pass always runs 128-row tiles (4 waves, no pairs, ring of 2, schedule 0), one workgroup per CU.
constexpr int AS_ROWS = 64;   // rows per workgroup of the exact sweep: 2 MFMA row tiles
constexpr int AS_BK = 32;     // feature columns per LDS stage (= the 32 canonical sumsq classes)
constexpr int FB_ROWS = 128;  // rows per workgroup (4 MFMA row tiles)
constexpr int FILTER_NW_DEFAULT = 4, FILTER_SCHED_DEFAULT = 0;  // K <= 256 defaults of k_assign_f16_rw
constexpr int FD_BK = 32;
constexpr int FD_DX = 3;  // row ring depth (2 stages = 32 KB in flight per workgroup, two workgroups per CU)
constexpr int FD_DC = 2;  // centre ring depth (1 stage in flight: an L2 round trip is shorter than a stage)
constexpr int FD_SLOT = 16384;  // bytes per ring slot: 128 rows x 32 fp32 == 256 centres x 32 bf16
constexpr unsigned CAND_MAX = 16;  // candidates per row beyond which the row takes the full exact sweep

struct AssignShape {
    int d, K;
    int64_t n;
    bool aligned;      // the row pointer is 16-byte aligned
    bool need_mean;    // the caller wants the mean distance: the filter's distances are approximate
    bool rows_scaled;  // the filter's copy of the centres asks for scaled rows (k_centers_scale): the XS instantiations
};
struct AssignLimits { int cus; };
struct AssignSwitches {        // the environment, read once by the caller (assign_switches() in acav_kmeans_assign.hip)
    bool exact_only = false;   // ACAV_ASSIGN_EXACT_ONLY=1
    bool pad = true;           // ACAV_FILTER_PAD=0: d % 32 != 0 takes the guarded exact sweep instead of padded copies
    bool cand = true;          // ACAV_ASSIGN_CAND=0: every undecided row to the full exact sweep
    int emit = 2;              // ACAV_ASSIGN_EMIT: 0 no emission at all, 1 lean filter + emission pass, else 2: in place
    long pair_cap = 0;         // ACAV_CAND_PAIR_CAP: a smaller candidate-pair pool (tests: the overflow path); 0 < v < default counts
    bool nt = true;            // ACAV_FILTER_NT=0: the default cache policy on the row DMA instead of the non-temporal one
    bool gs = true;            // ACAV_FILTER_GS=0: K > 256 loops over the groups inside one workgroup
    int nw = 0;                // ACAV_FILTER_NW=4|8: waves per workgroup; 0 = by shape
    int sched = FILTER_SCHED_DEFAULT;  // ACAV_FILTER_SCHED=2, any other value 0
};

enum AssignPath { ASSIGN_EXACT_GUARDED = 0, ASSIGN_EXACT_FAST = 1, ASSIGN_FILTER = 2 };
enum AssignError { ASSIGN_PLAN_OK = 0, ASSIGN_N_TOO_LARGE = 1 };  // a grid beyond 2^31 - 1 workgroups

// the template arguments of one k_assign_f16_rw instantiation as decimal digits, e.g. <true, 8, true, 3, 2, 0, false> = 1813200
constexpr int assign_kernel_id(bool nt, int nw, bool gs, int dcr, int sched, int emit, bool xs)
{
    return (((((nt * 10 + nw) * 10 + gs) * 10 + dcr) * 10 + sched) * 10 + emit) * 10 + xs;
}

struct AssignPlan {
    int error = ASSIGN_PLAN_OK, path = ASSIGN_EXACT_GUARDED;
    int64_t grid = 0;        // workgroups of the exact sweep over all rows (= partial sums of the mean distance)
    // ---- the filter path; all zero on the exact ones
    int fd = 0;              // the width the sweep runs at
    bool ragged = false;     // fd != d: the sweep runs on zero-padded copies of the rows and the centres
    int ngroups = 0;         // groups of 256 centres
    bool gs = false;         // one workgroup per (tile, group) pair; k_assign_merge folds the groups' records
    int nw = 0, sched = 0, dcr = 0;
    bool nt = false, xs = false;
    int emit = 0;            // EMIT of the filter launch: 2 = candidates in place, 0 = the lean kernel
    bool emit_pass = false;  // the emission pass (EMIT = 1) runs over the undecided list
    bool cand = false;       // the candidate buffers exist (and the K > 256 thresholds)
    bool und_list = false;   // filter and merge write the undecided list and its counter, k_assign_cand settles it; else the f32 list
    unsigned pair_cap = 0;
    int64_t fgrid = 0, egrid = 0;  // workgroups, threads and dynamic LDS bytes of the filter launch (f) and the emission pass (e)
    int fblock = 0, fsmem = 0, eblock = 0, esmem = 0;
    int64_t rgrid = 0;       // k_assign_f32 over the f32 list: a fixed grid strides over however many row tiles the list holds
    int cgrid = 0;           // k_assign_cand
    int filter_kernel() const { return path == ASSIGN_FILTER ? assign_kernel_id(nt, nw, gs, dcr, sched, emit, xs) : -1; }
    int emit_kernel() const { return emit_pass ? assign_kernel_id(nt, FB_ROWS / 32, false, FD_DC, 0, 1, xs) : -1; }
};

// bf16 filter + exact re-check (bit-identical labels, HBM-bound when the clusters are separated)?  Asked before the plan: the
// filter's plan needs the centre copy prepared (rows_scaled comes from it), the exact sweeps must not pay for one
inline bool assign_wants_filter(const AssignShape &s, const AssignSwitches &sw)
{
    const bool fast = s.d % AS_BK == 0 && s.aligned;
    return !s.need_mean && (s.d % FD_BK != 0 ? sw.pad : fast) && s.K >= 2 && s.n >= FB_ROWS && !sw.exact_only && s.n < 0x7fffffff;
}

inline AssignPlan assign_pick_plan(const AssignShape &s, const AssignLimits &l, const AssignSwitches &sw)
{
    AssignPlan p;
    p.grid = (s.n + AS_ROWS - 1) / AS_ROWS;
    if (p.grid > 0x7fffffff) {
        p.error = ASSIGN_N_TOO_LARGE;
        return p;
    }
    if (!assign_wants_filter(s, sw)) {
        p.path = s.d % AS_BK == 0 && s.aligned ? ASSIGN_EXACT_FAST : ASSIGN_EXACT_GUARDED;
        return p;
    }
    p.path = ASSIGN_FILTER;
    p.fd = (s.d + FD_BK - 1) / FD_BK * FD_BK;
    p.ragged = p.fd != s.d;
    // K > 256: one workgroup per (row tile, centre group) pair, the pairs of a tile side by side on one XCD, 256-row tiles (8
    // waves), centre ring of 3, DMA pieces spread between the MFMAs -- rows from HBM once.
    // (narrow views, fd <= 256: a pair is only 4-8 stages long and its ring fill and epilogue weigh as much as its stage loop
    // -- two 128-row workgroups per CU hide them under each other: d = 128, K = 1024: 0.59 vs 0.72 ms per 1.25M rows)
    p.ngroups = (s.K + 255) / 256;
    p.gs = p.ngroups > 1 && sw.gs;
    p.nw = sw.nw ? sw.nw : p.gs ? (p.fd <= 256 ? 4 : 8) : FILTER_NW_DEFAULT;
    p.dcr = p.nw == 8 ? 3 : FD_DC;  // 3 only fits the one-workgroup-per-CU tile
    p.sched = p.nw == 8 ? 2 : p.gs ? 0 : sw.sched;
    p.xs = s.rows_scaled;
    p.nt = sw.nt || p.xs;  // (nt rows are still found in L2 by the tile's other groups: PMC)
    // candidate-restricted exact re-check.  n < 2^27: slots and pairs -- at most 16 per row -- share one 64-bit allocator word
    p.cand = sw.cand && s.n < ((int64_t)1 << 27);
    const uint64_t cap = 4 * (uint64_t)s.n < 65536 ? 65536 : 4 * (uint64_t)s.n > 0x7fffffff ? 0x7fffffff : 4 * (uint64_t)s.n;
    p.pair_cap = (unsigned)(sw.pair_cap > 0 && (uint64_t)sw.pair_cap < cap ? (uint64_t)sw.pair_cap : cap);
    // K <= 256: the filter emits in place (or, ACAV_ASSIGN_EMIT=1, lists for the emission pass); K > 256: the (tile, group) pairs
    // cannot know a row's minimum over all groups -- k_assign_merge lists the undecided rows with their thresholds and the
    // emission pass runs the filter's main loop once more over those rows, all groups in one workgroup
    const bool in_place = p.ngroups == 1 && p.nw == 4 && p.sched == 0;
    p.und_list = p.cand && sw.emit != 0 && (in_place || p.gs);
    p.emit = p.und_list && in_place && sw.emit == 2 ? 2 : 0;
    p.emit_pass = p.und_list && p.emit == 0;
    const int64_t tile_rows = p.nw * 32, ntiles = (s.n + tile_rows - 1) / tile_rows;
    p.fgrid = p.gs ? (ntiles + 7) / 8 * 8 * p.ngroups : ntiles;  // pairs: whole rounds of the 8 XCDs per group
    if (p.fgrid > 0x7fffffff) {
        p.error = ASSIGN_N_TOO_LARGE;
        return p;
    }
    p.fblock = p.nw * 64;
    p.fsmem = FD_DX * p.nw * 4096 + p.dcr * FD_SLOT;
    if (p.emit_pass) {
        // one workgroup per CU (rings + lists do not fit twice), 4 waves / 128 rows: the 8-wave emission instantiations kept
        // 156-172 B of scratch and no run ever selected them outside A/B tests
        constexpr int enw = FB_ROWS / 32;
        const int64_t etiles = (s.n + FB_ROWS - 1) / FB_ROWS;
        p.egrid = etiles < l.cus ? etiles : l.cus;
        p.eblock = enw * 64;
        p.esmem = FD_DX * enw * 4096 + FD_DC * FD_SLOT + enw * 32 * (4 + 2 * (int)CAND_MAX);  // rings + lists
    }
    p.rgrid = p.grid < 2 * (int64_t)l.cus ? p.grid : 2 * (int64_t)l.cus;
    // (3 workgroups of 4 waves per CU: k_assign_cand is bound by the L2 -> L1 path -- 1, 2, 3, 4, 6 per CU all measure the same)
    p.cgrid = p.und_list ? 3 * l.cus : 0;
    return p;
}
