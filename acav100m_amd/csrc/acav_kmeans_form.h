// Which persistent kernel an epoch of acav_kmeans_train runs on, how many workgroups that takes and how much LDS each
// gets -- as ONE pure function of the shape, the device's limits and the experiment switches.  Plain C++: no HIP type, no
// getenv, no handle; acav_kmeans.hip fills the three structs and turns the TrainForm into a launch,
// acav_kmeans_train_form() exposes the choice to a machine without a GPU (tests/test_train_form.py).
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
