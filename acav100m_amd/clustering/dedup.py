"""Near-duplicates inside clusters (`cli.py dedup`, KMeans.near_duplicates, acav_rows_neardup).  No counterpart in the reference:
it removes duplicates only upstream, inside one video, with an ffmpeg signature; across videos nothing does.

Re-uploads, the same segment cut twice, a channel's static intro: fifty copies of one clip are fifty votes for one cell of the MI
selection's contingency tables, and picking one copy does nothing to make the next less attractive.  The method is SemDeDup's:
the clustering is the blocking structure, rows are compared only inside their cluster.  Near-duplicates land in the same cluster
and bitwise-equal rows always do (a label is a pure function of the row and the state); a pair that a cluster border splits is
missed -- the documented price of not doing N^2 work.

Definition on rows x [n, d] (fp32, after the view's front-end) with labels l [n] in [0, K), float64 throughout
(include/acav_hip.h states the summation order and the error bound):
  cos(i, j)  = x_i.x_j / sqrt(||x_i||^2 ||x_j||^2)
  E_i        = { j < i : l_j = l_i, ||x_j|| > 0 }: the earlier rows of the same cluster, in input order
  best[i]    = max over E_i of cos(i, j);  partner[i] = the lowest such j that attains it
  best[i] = -inf, partner[i] = -1 when E_i is empty or x_i is all zero; a zero row is never a partner
  flag[i]    = best[i] >= threshold
The rule is not transitive: a row is judged against every earlier row of its cluster, flagged or not (a chain a ~ b ~ c with a
and c apart flags b and c and keeps a).  The first occurrence wins.  Bitwise-equal rows come out within the bound of 1, not
necessarily at 1.0: a threshold of exactly 1 may miss them.  Every pair is a GPU sweep (there is no CPU path);
tests/_neardup_np.py restates the definition in numpy.

    python -m acav100m_amd.clustering.cli dedup --feature_path=<brace glob .pkl> --meta_path=<dir> \\
        --out_path=<dir of a cluster run> --clustering.cached_epoch=<e> --dedup.threshold=<t in (0, 1]> \\
        --dedup.out_path=<csv> [--dedup.view=<model_key>/<layer>] [--dedup.report_path=<json>]

Reads cache_epoch_{e}_{name} as `evaluate` does (warm-up refusal, the front-end of the cache: a whitened, projected or normalised
view is compared in the space it was clustered in), makes one pass over the row groups, gathers the chosen view's rows after the
front-end into one device buffer (only that view has to be held in one piece, the groups may stream), labels the buffer with
calc_best and runs acav_rows_neardup on it.  dedup.out_path (overwritten) holds the flagged rows in global row order, one line
each: shard_name,filename,partner_shard_name,partner_filename,similarity (repr of the float) -- a file `subset_selection/cli.py
run --exclude_path=` accepts.  dedup.report_path receives summarise's dictionary as json plus view, epoch, feature_path and
clusters_path.  Writes nothing into the cluster run's directory.  One process, one GPU.

Against a held-out set (nearest_in, KMeans.near_duplicates_in, acav_rows_crossdup): does the pool contain the evaluation sets,
do the new shards copy what is already curated?  For every row of a STREAMED pool the largest cosine to any row of a RESIDENT
held-out set y [m, d] and that row:
  E_i        = { j : ly_j = lx_i, ||y_j|| > 0 }  (no blocking: every non-zero row of y)
  best[i]    = max over E_i of cos(x_i, y_j);  partner[i] = the lowest such j, a position in y
  best[i] = -inf, partner[i] = -1 when E_i is empty or x_i is all zero
A pool row's answer depends on no other pool row, so the pool is taken one row group at a time and no [N, d] buffer of it
exists: only the held-out set has to fit the device in one piece.  A clip that is in both sets is flagged -- it IS a copy of a
held-out clip; remove it from the held-out shards if that is not wanted.  tests/_crossdup_np.py restates the definition.

    python -m acav100m_amd.clustering.cli dedup <the keys above> --dedup.against_path=<brace glob .pkl> \\
        --dedup.against_meta_path=<dir> [--dedup.blocking=none|cluster]

blocking=none (default) compares every pool row with every held-out row: no pair is missed, the cost is n m (printed before the
sweep).  blocking=cluster compares a pool row only with the held-out rows calc_best gives the same label: the in-cluster rule,
for a held-out set too large for n m (an earlier release); a bitwise copy always gets its source's label.  Both sets go
through the front-end of the cache, so a threshold read off an in-cluster run's similarity grid means the same here.  The csv
has the same layout, the partner columns naming the HELD-OUT clip; the json is summarise_against's dictionary plus view, epoch,
feature_path, clusters_path, against_path, blocking, pool_zero_rows and against_zero_rows.

Multi-probe (`--dedup.probes=m`, KMeans.probe_centers, acav_kmeans_probes, acav_rows_probedup): how large the price of the
cluster borders is, and a switch that lowers it -- the inverted file's nprobe.  A row is compared with the rows of its own
cluster and of the m - 1 centres next nearest to it (float64 distances, ties to the lower centre):
  E_i(p)     = { j : l_j = probes[i][p], ||y_j|| > 0, and j < i in the in-cluster mode }
  best[i]    = max over p < m and E_i(p) of cos(i, j);  partner[i] = the lowest such j that attains it, whatever its label
m in [1, min(16, K)], default 1: the run of today, through acav_rows_neardup / acav_rows_crossdup, byte for byte.  Valid in the
in-cluster mode and with --dedup.blocking=cluster (the pool still streams, the lists of a pool piece are computed per row
group); refused with blocking=none, where there is nothing to probe.  The csv keeps its layout.  With m > 1 the report gains
probes, pairs (compared) and flagged_by_probes [m]: entry p - 1 counts the rows whose best over their first p probed clusters
reaches the threshold -- entry 0 is what probes=1 flags, and where the curve flattens a further probe no longer pays; the verb
prints it under the similarity grid, so one run at a generous m is enough to pick m.  tests/_probedup_np.py restates both
definitions.

Duplicate groups (`--dedup.groups=True`, pairs_earlier / components / choose_kept, KMeans.duplicate_groups,
acav_rows_neardup_pairs, acav_pairs_components): the rule above gives one number per row and depends on the row order.  Rows
a < b < c of one cluster with cos(a, c) >= t, cos(b, c) >= t and cos(a, b) < t: a and b both stay and c goes; had c come
first, c would stay and a and b go.  The groups mode takes the full graph instead of its nearest-earlier forest:
  P_i        = { j in E_i : cos(i, j) >= t }: every pair, listed at its later row (offsets [n + 1], pair_j, pair_cos)
  root[i]    = the lowest row of the connected component of i in the graph of all pairs; a group: a component of >= 2 rows
  kept[i]    = True outside the groups and for one row per group: its root (keep=first) or the member with the smallest
               squared distance to its centre (keep=central; KMeans.quality's a2, ties to the lower row)
The groups as sets of rows do not depend on the order of the rows, and every row the nearest-earlier rule flags is removed.

    python -m acav100m_amd.clustering.cli dedup <the keys of the in-cluster run> --dedup.groups=True \\
        [--dedup.keep=first|central] [--dedup.max_pairs=<N>] [--dedup.groups_path=<csv>]

dedup.out_path then lists every row that is NOT kept, in global row order: shard_name,filename,kept_shard_name,kept_filename,
similarity (the largest cosine among the row's pairs, earlier or later),group_size -- still a file --exclude_path accepts.
dedup.groups_path lists every member of every group, kept ones included, by group and row: group (the global row number of the
root),group_size,kept,shard_name,filename.  The json is summarise_groups' dictionary plus the keys above.  More than
dedup.max_pairs pairs (default 2^27) are refused with the total and the five clusters that hold the most.  The three keys need
dedup.groups; the mode is refused with dedup.against_path (a bipartite question: no groups among pool rows) and with
dedup.probes > 1 (the pairs of probed clusters are a follow-up).  tests/_dupgroups_np.py restates the definition.

Confirmation in a second view (`--dedup.confirm_view=<model_key>/<layer> --dedup.confirm_threshold=<t2 in (0, 1]>`, pair_rows /
pair_cosines / confirm_pairs, KMeans.duplicate_groups(confirm=), acav_pairs_cosine): one view is a weak witness -- every lecture
over the same static slide is a video duplicate, every clip with the same licensed song an audio duplicate, a true re-upload
matches in both.  With view A = dedup.view, t = dedup.threshold, view B = dedup.confirm_view and cosB the cosine of B's rows:
  P_i'       = { j in P_i : cosB(i, j) >= t2 }
  roots, groups, kept and similarity are the definitions above over P' in place of P; similarity stays a cosine of view A, the
  largest among the row's CONFIRMED pairs; keep=central keeps using view A's a2; the blocking is view A's clustering alone.
The pass of today yields P; a second pass over the row groups gathers only the R rows that occur in a pair from view B -- through
the front-end the cache holds for B, so B is compared in the space it was clustered in -- into a [R, dB] device buffer (refused
with the sizes when it does not fit; B is never held in one piece, a streamed run reads the shards a second time; no pair in A:
no second pass), acav_pairs_cosine gives cosB of the listed pairs with acav_rows_neardup's arithmetic, chain for chain, and the
filtered list goes on to the components.  The files keep their layouts.  The report gains confirm_view, confirm_threshold,
pairs_before_confirm (pairs: the confirmed ones), groups_before_confirm and removed_before_confirm (the components of A alone)
and confirm_similarity_counts (A's pairs with cosB >= g over the grid: one run is enough to pick t2); flagged,
similarity_counts and the nearest-earlier rule of removed_beyond_nearest_rule stay those of view A alone.  The two keys go
together, need dedup.groups=True (the confirmed relation is a pair list, and the groups mode is the one that has it) and are
refused with dedup.against_path.  tests/_dupconfirm_np.py restates the definition."""
import csv
import json
import numbers
from collections import OrderedDict
from pathlib import Path

import numpy as np

from .. import _lib
from .sgd_clustering import _as_f32_2d, _device_index
from .silhouette import _labels

SIMILARITY_GRID = (0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.98, 0.99, 0.999, 0.9999)


def _probe_lists(probes, n):
    """probes [n, m] (numpy or torch, host or device) as a contiguous int64 array the library reads, and m"""
    shape = tuple(probes.shape) if hasattr(probes, "shape") else np.shape(probes)
    if len(shape) != 2 or shape[0] != n:
        raise ValueError("expected [{}, m] probe lists, got shape {}".format(n, shape))
    return _labels(probes.reshape(-1) if hasattr(probes, "reshape") else np.asarray(probes, np.int64).reshape(-1), n * shape[1]), shape[1]


def nearest_earlier(x, labels, k=None, device="cuda", probes=None, each=False):
    """(best float64 [n], partner int64 [n]) of x [n, d] with labels [n] in [0, k) (k=None: max label + 1): acav_rows_neardup.
    x and labels: numpy or torch, host or device.  probes [n, m] (KMeans.probe_centers; -1: no such slot): the earlier rows of
    the m probed clusters of every row instead of its own alone, acav_rows_probedup with y = x and before[i] = i; each=True
    (with probes) adds best_each float64 [n, m], the best of every probed cluster on its own."""
    keep, xp, n, on_gpu = _as_f32_2d(x)
    d = int(keep.shape[1])
    lab = _labels(labels, n)
    if k is None:
        k = int(lab.max()) + 1 if n else 1
    best, partner = np.empty(n, np.float64), np.empty(n, np.int64)
    lib = _lib.load_library()
    dev = keep.device.index if on_gpu else _device_index(device)
    if probes is None:
        if each:
            raise ValueError("each=True needs probes: without them there is one cluster per row")
        _lib.check(lib.acav_rows_neardup(dev, xp, n, d, _lib.ptr(lab), int(k), _lib.ptr(best), _lib.ptr(partner), None))
        return best, partner
    lists, m = _probe_lists(probes, n)
    best_each = np.empty((n, m), np.float64) if each else None
    before = np.arange(n, dtype=np.int64)
    _lib.check(lib.acav_rows_probedup(dev, xp, n, xp, n, d, _lib.ptr(lists), int(m), _lib.ptr(lab), _lib.ptr(before), int(k),
                                      _lib.ptr(best), _lib.ptr(partner), _lib.ptr(best_each), None))
    return (best, partner, best_each) if each else (best, partner)


def nearest_in(x, y, labels_x=None, labels_y=None, k=None, device="cuda", probes_x=None, each=False):
    """(best float64 [n], partner int64 [n]) of the rows of x [n, d] against the held-out rows y [m, d]: acav_rows_crossdup.
    labels_x [n] and labels_y [m] in [0, k) (k=None: the largest label of either + 1) block the pairs; both None: every pair.
    x, y and the labels: numpy or torch, host or device; a device y is used where it lies, not copied.  probes_x [n, m]
    (KMeans.probe_centers of x; needs labels_y): the rows of y in the m probed clusters of every row, acav_rows_probedup;
    labels_x is then only used for k=None.  each=True (with probes_x) adds best_each float64 [n, m]."""
    keep_x, xp, n, x_gpu = _as_f32_2d(x)
    d = int(keep_x.shape[1])
    keep_y, yp, m, y_gpu = _as_f32_2d(y, width=d)
    if probes_x is not None and labels_x is None and labels_y is not None:
        labels_x = probes_x[:, 0]
    if (labels_x is None) != (labels_y is None):
        raise ValueError("labels_x and labels_y go together: both, or neither (no blocking)")
    lab_x = lab_y = None
    if labels_x is not None:
        lab_x, lab_y = _labels(labels_x, n), _labels(labels_y, m)
        if k is None:
            k = 1 + max(int(lab_x.max()) if n else 0, int(lab_y.max()) if m else 0)
    elif k is None:
        k = 1
    best, partner = np.empty(n, np.float64), np.empty(n, np.int64)
    lib = _lib.load_library()
    dev = keep_y.device.index if y_gpu else keep_x.device.index if x_gpu else _device_index(device)
    if probes_x is None:
        if each:
            raise ValueError("each=True needs probes_x: without them there is one cluster per row")
        _lib.check(lib.acav_rows_crossdup(dev, xp, n, yp, m, d, _lib.ptr(lab_x), _lib.ptr(lab_y), int(k), _lib.ptr(best),
                                          _lib.ptr(partner), None))
        return best, partner
    if lab_y is None:
        raise ValueError("probes_x need labels_y: without blocking there is nothing to probe")
    lists, mp = _probe_lists(probes_x, n)
    best_each = np.empty((n, mp), np.float64) if each else None
    _lib.check(lib.acav_rows_probedup(dev, xp, n, yp, m, d, _lib.ptr(lists), int(mp), _lib.ptr(lab_y), None, int(k),
                                      _lib.ptr(best), _lib.ptr(partner), _lib.ptr(best_each), None))
    return (best, partner, best_each) if each else (best, partner)


MAX_PAIRS = 2 ** 27   # the default dedup.max_pairs: at 16 bytes per pair 2 GiB on the device and 2 GiB on the host
FIRST_CAP = 2 ** 20   # the room of the first call: pairs are normally far fewer than rows


def pairs_earlier(x, labels, threshold, k=None, device="cuda", max_pairs=None):
    """every pair of a cluster at cosine >= threshold, listed at its later row (acav_rows_neardup_pairs) -> (best float64 [n],
    partner int64 [n], offsets int64 [n + 1], pair_j int64 [P], pair_cos float64 [P]), P = offsets[n]: row i's earlier
    partners are pair_j[offsets[i]:offsets[i + 1]] in ascending position; best and partner are nearest_earlier's bytes.  The
    first call has room for min(max_pairs, max(n, 2^20)) pairs, a second one with the exact size runs only when that is
    exceeded.  More than max_pairs (None: 2^27) pairs: ValueError naming the total and the five clusters with the most."""
    keep, xp, n, on_gpu = _as_f32_2d(x)
    d = int(keep.shape[1])
    lab = _labels(labels, n)
    if k is None:
        k = int(lab.max()) + 1 if n else 1
    max_pairs = MAX_PAIRS if max_pairs is None else int(max_pairs)
    if max_pairs < 0:
        raise ValueError("max_pairs must not be negative, not {}".format(max_pairs))
    best, partner, offsets = np.empty(n, np.float64), np.empty(n, np.int64), np.empty(n + 1, np.int64)
    lib = _lib.load_library()
    dev = keep.device.index if on_gpu else _device_index(device)

    def sweep(cap):
        pair_j, pair_cos = (np.empty(cap, np.int64), np.empty(cap, np.float64)) if cap else (None, None)
        _lib.check(lib.acav_rows_neardup_pairs(dev, xp, n, d, _lib.ptr(lab), int(k), float(threshold), _lib.ptr(best),
                                               _lib.ptr(partner), _lib.ptr(offsets), cap, _lib.ptr(pair_j), _lib.ptr(pair_cos), None))
        return pair_j, pair_cos

    cap = min(max_pairs, max(n, FIRST_CAP))
    pair_j, pair_cos = sweep(cap)
    total = int(offsets[n])
    if total > max_pairs:
        per = np.bincount(_host(lab), weights=np.diff(offsets), minlength=int(k)).astype(np.int64)
        worst = np.argsort(-per, kind='stable')[:5]
        raise ValueError("{} pairs at cosine >= {!r}, more than max_pairs = {}; the clusters with the most: {}; raise the "
                         "threshold (or max_pairs)".format(total, float(threshold), max_pairs, ", ".join(
                             "{}: {}".format(int(c), int(per[c])) for c in worst if per[c] > 0)))
    if total > cap:
        pair_j, pair_cos = sweep(total)
    if pair_j is None:
        pair_j, pair_cos = np.empty(0, np.int64), np.empty(0, np.float64)
    return best, partner, offsets, pair_j[:total], pair_cos[:total]


def components(n, offsets, pair_j):
    """root int64 [n] of the pair list (offsets [n + 1], pair_j): the lowest position of every row's connected component, the
    row itself where it is in no pair (acav_pairs_components: host only, no device)"""
    offsets, pair_j = np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(pair_j, np.int64)
    if offsets.shape != (int(n) + 1,) or pair_j.ndim != 1 or (len(offsets) and int(offsets[-1]) != len(pair_j)):
        raise ValueError("offsets {} and pair_j {} do not belong to {} rows".format(offsets.shape, pair_j.shape, n))
    root = np.empty(int(n), np.int64)
    if n:
        _lib.check(_lib.load_library().acav_pairs_components(int(n), _lib.ptr(offsets), _lib.ptr(pair_j) if len(pair_j) else None,
                                                             _lib.ptr(root)))
    return root


def pair_cosines(x, pair_i, pair_j, device="cuda"):
    """float64 [P]: the cosine of every listed pair (pair_i[e], pair_j[e]) of x [n, d] (acav_pairs_cosine); -inf where a row is
    all zero.  Any indices in [0, n), in any order, i == j allowed.  x and the lists: numpy or torch, host or device.  For a pair
    that pairs_earlier lists for the same x these are the bytes of its pair_cos."""
    keep, xp, n, on_gpu = _as_f32_2d(x)
    d = int(keep.shape[1])
    pairs = int(pair_i.shape[0]) if hasattr(pair_i, "shape") else len(pair_i)
    pi, pj = _labels(pair_i, pairs), _labels(pair_j, pairs)
    cos = np.empty(pairs, np.float64)
    dev = keep.device.index if on_gpu else _device_index(device)
    _lib.check(_lib.load_library().acav_pairs_cosine(dev, xp, n, d, _lib.ptr(pi) if pairs else None, _lib.ptr(pj) if pairs else None,
                                                     pairs, _lib.ptr(cos), None))
    return cos


def pair_rows(offsets, pair_j):
    """(later int64 [P], rows int64 [R], ci int64 [P], cj int64 [P]) of a pair list (pure numpy): the later row of every pair,
    the ascending unique rows that occur in any pair, and the pairs re-indexed into rows: rows[ci[e]] = later[e], rows[cj[e]] =
    pair_j[e] -- a second view needs only those R rows"""
    offsets, pair_j = np.asarray(offsets, np.int64), np.asarray(pair_j, np.int64)
    later = np.repeat(np.arange(len(offsets) - 1, dtype=np.int64), np.diff(offsets))
    if later.shape != pair_j.shape:
        raise ValueError("offsets state {} pairs, pair_j holds {}".format(later.shape[0], pair_j.shape))
    rows = np.unique(np.concatenate([later, pair_j]))
    return later, rows, np.searchsorted(rows, later).astype(np.int64), np.searchsorted(rows, pair_j).astype(np.int64)


def confirm_pairs(offsets, pair_j, pair_cos, keep):
    """(offsets int64 [n + 1], pair_j int64 [P'], pair_cos float64 [P']) of the pairs where keep bool [P] is True (pure numpy):
    the same layout, the order inside a row preserved; a row all of whose pairs go has none"""
    offsets, pair_j, pair_cos = np.asarray(offsets, np.int64), np.asarray(pair_j, np.int64), np.asarray(pair_cos, np.float64)
    keep = np.asarray(keep, bool)
    n = len(offsets) - 1
    if not pair_j.shape == pair_cos.shape == keep.shape == (int(offsets[-1]),):
        raise ValueError("pair_j {}, pair_cos {} and keep {} do not belong to {} pairs".format(pair_j.shape, pair_cos.shape,
                                                                                              keep.shape, int(offsets[-1])))
    later = np.repeat(np.arange(n, dtype=np.int64), np.diff(offsets))
    out = np.zeros(n + 1, np.int64)
    out[1:] = np.cumsum(np.bincount(later[keep], minlength=n))
    return out, pair_j[keep], pair_cos[keep]


def confirm_similarity_counts(cos_b):
    """for every g of SIMILARITY_GRID how many of the first view's pairs have a cosine >= g in the second view: one run is
    enough to pick dedup.confirm_threshold"""
    cos_b = np.asarray(cos_b, np.float64)
    return OrderedDict((repr(g), int((cos_b >= g).sum())) for g in SIMILARITY_GRID)


def choose_kept(root, keep, a2=None):
    """kept bool [n]: True for the rows in no group and for one row of every group.  keep='first': the root, the group's lowest
    position.  keep='central': the member with the smallest a2 [n] (KMeans.quality(rows=True)'s float64 squared distance to the
    assigned centre; the members of a group share a cluster, so the values are comparable), ties to the lower position"""
    root = np.asarray(root, np.int64)
    n = len(root)
    if keep == 'first':
        return root == np.arange(n)
    if keep != 'central':
        raise ValueError("keep must be 'first' or 'central', not {!r}".format(keep))
    if a2 is None or np.shape(a2) != (n,):
        raise ValueError("keep='central' needs a2 [{}], the squared distances to the assigned centres".format(n))
    order = np.lexsort((np.arange(n), np.asarray(a2, np.float64), root))  # by group, then a2, then position
    head = np.ones(n, bool)
    head[1:] = root[order[1:]] != root[order[:-1]]
    kept = np.zeros(n, bool)
    kept[order[head]] = True
    return kept


def pair_similarity(n, offsets, pair_j, pair_cos):
    """float64 [n]: the largest cosine among a row's pairs, earlier or later; -inf for a row in no pair"""
    sim = np.full(int(n), -np.inf)
    later = np.repeat(np.arange(int(n)), np.diff(np.asarray(offsets, np.int64)))
    np.maximum.at(sim, later, pair_cos)
    np.maximum.at(sim, np.asarray(pair_j, np.int64), pair_cos)
    return sim


def _size_bins(sizes):
    """group sizes >= 2 counted in the bins 2, 3-4, 5-8, ...: (2^(b-1), 2^b], up to the bin of the largest"""
    sizes = np.asarray(sizes, np.int64)
    bins = OrderedDict()
    if len(sizes):
        b = np.ceil(np.log2(sizes)).astype(np.int64)  # exact for the powers of two: log2 of a float64 power of two is exact
        for e in range(1, int(b.max()) + 1):
            bins["2" if e == 1 else "{}-{}".format(2 ** (e - 1) + 1, 2 ** e)] = int((b == e).sum())
    return bins


def summarise_groups(best, partner, labels, k, threshold, offsets, root, kept, keep='first'):
    """the report of a groups run (pure numpy): summarise's dictionary and pairs (offsets[n]), groups (the components of two
    rows or more), removed (the rows not kept), removed_beyond_nearest_rule (the removed rows the nearest-earlier rule does not
    flag), group_size_counts (bins 2, 3-4, 5-8, ... by powers of two), largest_groups (the ten largest, ties to the lower
    root: size, cluster, kept row) and keep"""
    report = summarise(best, partner, labels, k, threshold)
    n = report['n']
    root, kept, lab = np.asarray(root, np.int64), np.asarray(kept, bool), np.asarray(labels, np.int64)
    offsets = np.asarray(offsets, np.int64)
    if root.shape != (n,) or kept.shape != (n,) or offsets.shape != (n + 1,):
        raise ValueError("root {}, kept {} and offsets {} do not belong to {} rows".format(root.shape, kept.shape, offsets.shape, n))
    size = np.bincount(root, minlength=n)  # at the roots
    groups = np.flatnonzero(size >= 2)
    if (kept[size[root] < 2] != True).any() or (np.bincount(root[kept], minlength=n)[groups] != 1).any():  # noqa: E712
        raise ValueError("kept does not keep every row outside the groups and exactly one row of every group")
    kept_of = np.full(n, -1, np.int64)
    kept_of[root[kept]] = np.flatnonzero(kept)
    largest = groups[np.argsort(-size[groups], kind='stable')[:10]]
    report.update([
        ('pairs', int(offsets[n])), ('groups', int(len(groups))), ('removed', int((~kept).sum())),
        ('removed_beyond_nearest_rule', int((~kept & ~flag(best, threshold)).sum())),
        ('group_size_counts', _size_bins(size[groups])),
        ('largest_groups', [OrderedDict([('size', int(size[g])), ('cluster', int(lab[g])), ('kept', int(kept_of[g]))]) for g in largest]),
        ('keep', keep)])
    return report


def flag(best, threshold):
    """bool [n]: best >= threshold (-inf, a row without an earlier row to compare with, is never flagged)"""
    return np.asarray(best, np.float64) >= float(threshold)


def probe_pairs(probes, labels_y, before=None):
    """the pairs acav_rows_probedup compares (pure numpy): over the slots of probes [n, m] that count (not -1, not a label
    repeated in the row's list) the rows of labels_y [my] with the slot's label at positions below before[i] (all: None)"""
    lists, ly = np.asarray(probes, np.int64), np.asarray(labels_y, np.int64)
    n, m = lists.shape
    counts = lists >= 0
    for p in range(1, m):
        counts[:, p] &= ~(lists[:, :p] == lists[:, p:p + 1]).any(1)
    span = len(ly) + 1
    keys = np.sort(ly * span + np.arange(len(ly)))  # by label, then position
    cut = np.full(n, len(ly), np.int64) if before is None else np.clip(np.asarray(before, np.int64), 0, len(ly))
    c = np.where(counts, lists, 0)
    rows = np.searchsorted(keys, c * span + cut[:, None]) - np.searchsorted(keys, c * span)
    return int(rows[counts].sum())


def _probe_keys(best_each, threshold, pairs):
    """the keys a report gains with probes > 1: entry p - 1 of flagged_by_probes counts the rows whose best over their first p
    probed clusters reaches the threshold -- entry 0 is what probes=1 flags, and where the curve flattens a further probe no
    longer pays"""
    each = np.asarray(best_each, np.float64)
    upto = np.maximum.accumulate(each, axis=1)
    return [('probes', int(each.shape[1])), ('pairs', int(pairs)),
            ('flagged_by_probes', [int(c) for c in (upto >= float(threshold)).sum(0)])]


def summarise(best, partner, labels, k, threshold, probes=None, best_each=None):
    """the report of one run (pure numpy): n, K, threshold, flagged and flagged_share, flagged_by_cluster [K], zero_rows -- the
    rows that have an earlier row in their cluster and yet no partner: all-zero rows, or rows all of whose earlier cluster mates
    are all-zero -- and similarity_counts: the rows with best >= g for every g of SIMILARITY_GRID, so that a threshold can be
    picked from one run.  probes [n, m] and best_each [n, m] of a multi-probe run with m > 1 (nearest_earlier(probes=,
    each=True)) add probes = m, pairs (compared) and flagged_by_probes [m]; without them, and at m = 1, the keys are today's"""
    if probes is not None and np.shape(probes)[1] > 1:
        if best_each is None or np.shape(best_each) != np.shape(probes):
            raise ValueError("probes {} need best_each of the same shape".format(np.shape(probes)))
        report = summarise(best, partner, labels, k, threshold)
        report.update(_probe_keys(best_each, threshold, probe_pairs(probes, labels, np.arange(report['n']))))
        return report
    best, partner = np.asarray(best, np.float64), np.asarray(partner, np.int64)
    lab, k = np.asarray(labels, np.int64), int(k)
    n = int(best.shape[0])
    if partner.shape != (n,) or lab.shape != (n,):
        raise ValueError("best {}, partner {} and labels {} do not belong together".format(best.shape, partner.shape, lab.shape))
    flagged = flag(best, threshold)
    first = np.ones(n, bool)  # the first row of its cluster in input order
    order = np.argsort(lab, kind='stable')
    first[order[1:]] = lab[order[1:]] != lab[order[:-1]]
    return {
        'n': n, 'K': k, 'threshold': float(threshold),
        'flagged': int(flagged.sum()), 'flagged_share': float(flagged.sum() / n) if n else float('nan'),
        'flagged_by_cluster': [int(c) for c in np.bincount(lab[flagged], minlength=k)],
        'zero_rows': int(((partner < 0) & ~first).sum()),
        'similarity_counts': OrderedDict((repr(g), int((best >= g).sum())) for g in SIMILARITY_GRID),
    }


def summarise_against(best, partner, labels_x, hist_y, k, threshold, m, probes_x=None, best_each=None):
    """the report of one run against a held-out set of m rows (pure numpy).  labels_x [n] and hist_y [k] (the held-out rows per
    cluster): blocking=cluster; both None and k = 1: no blocking.  n, m, K, threshold, flagged and flagged_share,
    flagged_by_cluster [K] (blocked only), similarity_counts as in summarise, pairs = sum over the clusters of (pool rows) x
    (held-out rows), n m when unblocked, and without_candidates: the pool rows whose cluster holds no non-zero held-out row --
    counted as the rows of the clusters in which no pool row has a partner (a cluster all of whose pool rows are all-zero
    counts too: pool_zero_rows of the verb's report tells).  probes_x [n, mp] and best_each [n, mp] of a multi-probe run with
    mp > 1 (nearest_in(probes_x=, each=True), blocked only) add probes = mp and flagged_by_probes [mp] and make pairs the
    pairs of all probed clusters; without them, and at mp = 1, the keys and values are today's"""
    if probes_x is not None and np.shape(probes_x)[1] > 1:
        if labels_x is None or best_each is None or np.shape(best_each) != np.shape(probes_x):
            raise ValueError("probes_x {} need labels_x, hist_y and best_each of the same shape".format(np.shape(probes_x)))
        report = summarise_against(best, partner, labels_x, hist_y, k, threshold, m)
        ly = np.repeat(np.arange(int(k)), np.asarray(hist_y, np.int64))  # any labels with this histogram: no cut, only counts
        keys = OrderedDict(_probe_keys(best_each, threshold, probe_pairs(probes_x, ly)))
        report['pairs'] = keys.pop('pairs')
        report.update(keys)
        return report
    best, partner, k, m = np.asarray(best, np.float64), np.asarray(partner, np.int64), int(k), int(m)
    n = int(best.shape[0])
    blocked = labels_x is not None
    if blocked != (hist_y is not None) or (not blocked and k != 1):
        raise ValueError("labels_x and hist_y go together; without them k is 1")
    lab = np.asarray(labels_x, np.int64) if blocked else np.zeros(n, np.int64)
    hist = np.asarray(hist_y, np.int64) if blocked else np.array([m], np.int64)
    if partner.shape != (n,) or lab.shape != (n,) or hist.shape != (k,) or int(hist.sum()) != m:
        raise ValueError("best {}, partner {}, labels_x {} and hist_y {} (m = {}) do not belong together".format(
            best.shape, partner.shape, lab.shape, hist.shape, m))
    flagged = flag(best, threshold)
    hist_x = np.bincount(lab, minlength=k)
    served = np.bincount(lab[partner >= 0], minlength=k) > 0  # the clusters in which a pool row found a partner
    report = OrderedDict([
        ('n', n), ('m', m), ('K', k), ('threshold', float(threshold)),
        ('flagged', int(flagged.sum())), ('flagged_share', float(flagged.sum() / n) if n else float('nan'))])
    if blocked:
        report['flagged_by_cluster'] = [int(c) for c in np.bincount(lab[flagged], minlength=k)]
    report['similarity_counts'] = OrderedDict((repr(g), int((best >= g).sum())) for g in SIMILARITY_GRID)
    report['pairs'] = int(sum(int(a) * int(b) for a, b in zip(hist_x, hist)))
    report['without_candidates'] = int(hist_x[~served].sum())
    return report


def check_against_options(opts):
    """the keys of the against mode -> (against_path, against_meta_path, blocking); against_path None: the in-cluster dedup.
    Pure: no device, no file"""
    opts = opts or {}
    path, meta, blocking = opts.get('against_path'), opts.get('against_meta_path'), opts.get('blocking')
    if path is None:
        for key, value in (('against_meta_path', meta), ('blocking', blocking)):
            if value is not None:
                raise ValueError("dedup.{} is only valid with --dedup.against_path=<brace glob of the held-out feature "
                                 "shards>".format(key))
        return None, None, None
    if not isinstance(path, str) or not path:
        raise ValueError("dedup.against_path must be a brace glob of feature .pkl shards, not {!r}".format(path))
    if meta is None:
        raise ValueError("dedup.against_path needs --dedup.against_meta_path=<dir>: the metadata of the held-out shards")
    blocking = 'none' if blocking is None else blocking
    if blocking not in ('none', 'cluster'):
        raise ValueError("dedup.blocking must be 'none' or 'cluster', not {!r}".format(blocking))
    return path, str(meta), blocking


PROBES_MAX = 16  # ACAV_PROBES_MAX (include/acav_hip.h)


def check_probes(opts, k=None):
    """dedup.probes -> m, 1 when the key is absent: an integer in [1, min(16, K)] (k: K once the cache is known), valid in the
    in-cluster mode and with dedup.blocking=cluster -- without blocking there is nothing to probe.  Pure: no device, no file"""
    opts = opts or {}
    m = opts.get('probes')
    if m is None:
        return 1
    if isinstance(m, bool) or not isinstance(m, numbers.Integral) or not 1 <= int(m) <= PROBES_MAX:
        raise ValueError("dedup.probes must be an integer in [1, min({}, K)], not {!r}".format(PROBES_MAX, m))
    if k is not None and int(m) > int(k):
        raise ValueError("dedup.probes={} exceeds the K={} clusters of the run: there are no more centres to probe".format(m, k))
    path, _meta, blocking = check_against_options(opts)
    if int(m) > 1 and path is not None and blocking != 'cluster':  # one probe is the default: the run of today
        raise ValueError("dedup.probes is refused with dedup.blocking=none: every pool row is compared with every held-out row "
                         "already, there is nothing to probe; use --dedup.blocking=cluster")
    return int(m)


def check_groups(opts):
    """the keys of the groups mode -> (groups, keep, max_pairs, groups_path); groups False: the nearest-earlier run of today.
    dedup.keep, dedup.max_pairs and dedup.groups_path are refused without dedup.groups=True, and dedup.groups with
    dedup.against_path or dedup.probes > 1.  Pure: no device, no file"""
    opts = opts or {}
    groups, keep, max_pairs, groups_path = opts.get('groups'), opts.get('keep'), opts.get('max_pairs'), opts.get('groups_path')
    if groups is not None and not isinstance(groups, bool):
        raise ValueError("dedup.groups must be True or False, not {!r}".format(groups))
    if not groups:
        for key, value in (('keep', keep), ('max_pairs', max_pairs), ('groups_path', groups_path)):
            if value is not None:
                raise ValueError("dedup.{} is only valid with --dedup.groups=True".format(key))
        return False, None, None, None
    if opts.get('against_path') is not None:
        raise ValueError("dedup.groups is refused with dedup.against_path: which pool rows copy a held-out row is a bipartite "
                         "question, there are no groups among the pool rows")
    probes = opts.get('probes')
    if probes is not None and probes != 1:
        raise ValueError("dedup.groups is refused with dedup.probes > 1: the pairs of the probed clusters are a follow-up; "
                         "use dedup.probes=1, the pairs inside the clusters")
    keep = 'first' if keep is None else keep
    if keep not in ('first', 'central'):
        raise ValueError("dedup.keep must be 'first' or 'central', not {!r}".format(keep))
    if max_pairs is not None and (isinstance(max_pairs, bool) or not isinstance(max_pairs, numbers.Integral) or int(max_pairs) < 1):
        raise ValueError("dedup.max_pairs must be a positive integer, not {!r}".format(max_pairs))
    if groups_path is not None and (not isinstance(groups_path, str) or not groups_path):
        raise ValueError("dedup.groups_path must be a csv path, not {!r}".format(groups_path))
    return True, keep, MAX_PAIRS if max_pairs is None else int(max_pairs), groups_path


def check_confirm(opts, views=None, view=None):
    """the keys of the confirmation in a second view -> (confirm_view, confirm_threshold); (None, None): the run of today.  The
    two keys go together, need dedup.groups=True and are refused with dedup.against_path; confirm_view has the form "a/b" and
    differs from dedup.view (view: the resolved one, once the cache is known) and, with views (the names the cache holds), is
    one of them.  Pure: no device, no file"""
    opts = opts or {}
    cview, cthr = opts.get('confirm_view'), opts.get('confirm_threshold')
    if cview is None and cthr is None:
        return None, None
    if cview is None or cthr is None:
        raise ValueError("dedup.confirm_view and dedup.confirm_threshold go together: --dedup.confirm_view=<model_key>/<layer> "
                         "--dedup.confirm_threshold=<t2 in (0, 1]>")
    if opts.get('against_path') is not None:
        raise ValueError("dedup.confirm_view is refused with dedup.against_path: the confirmation filters the pair list of the "
                         "groups mode, a run against a held-out set has none")
    if not opts.get('groups'):
        raise ValueError("dedup.confirm_view needs --dedup.groups=True: the confirmed relation is a pair list, and the groups mode "
                         "is the one that has it")
    if isinstance(cthr, bool) or not isinstance(cthr, numbers.Real) or not 0.0 < float(cthr) <= 1.0:
        raise ValueError("dedup.confirm_threshold must be a number in (0, 1], not {!r}".format(cthr))
    if not isinstance(cview, str) or cview.count('/') != 1:
        raise ValueError("dedup.confirm_view must be \"<model_key>/<layer>\", not {!r}".format(cview))
    view = opts.get('view') if view is None else view
    if cview == view:
        raise ValueError("dedup.confirm_view={!r} is dedup.view: a second view confirms the pairs of the first".format(cview))
    if views is not None and cview not in list(views):
        raise ValueError("dedup.confirm_view={!r} is not a view of the cache (it has {})".format(cview, ', '.join(views)))
    return cview, float(cthr)


def check_options(opts, views=None, epoch=None, k=None):
    """the `dedup` options -> (threshold, view, out_path, report_path).  Pure: no device, no file.  views: the names
    "<model_key>/<layer>" the cache holds, once it is known (None: dedup.view is only checked for its form); epoch:
    clustering.cached_epoch, when given exactly one epoch is required; k: the K of the cluster run, once it is known
    (dedup.probes is checked against it, check_probes)"""
    opts = opts or {}
    check_against_options(opts)
    check_probes(opts, k)
    check_groups(opts)
    check_confirm(opts)
    thr = opts.get('threshold')
    if thr is None:
        raise ValueError("dedup needs --dedup.threshold=<t in (0, 1]>: the cosine from which a row counts as a duplicate of an "
                         "earlier one; there is no default, the right value depends on the embedding")
    if isinstance(thr, bool) or not isinstance(thr, numbers.Real) or not 0.0 < float(thr) <= 1.0:
        raise ValueError("dedup.threshold must be a number in (0, 1], not {!r}".format(thr))
    out_path, report_path, view = opts.get('out_path'), opts.get('report_path'), opts.get('view')
    if out_path is None:
        raise ValueError("dedup needs --dedup.out_path=<csv>: where the flagged rows go")
    if view is not None and (not isinstance(view, str) or view.count('/') != 1):
        raise ValueError("dedup.view must be \"<model_key>/<layer>\", not {!r}".format(view))
    if views is not None:
        views = list(views)
        if view is None:
            if len(views) != 1:
                raise ValueError("dedup.view is required, the cache holds {} views: {}".format(len(views), ', '.join(views)))
            view = views[0]
        elif view not in views:
            raise ValueError("dedup.view={!r} is not a view of the cache (it has {})".format(view, ', '.join(views)))
        check_confirm(opts, views=views, view=view)
    if epoch is not None:
        if isinstance(epoch, (list, tuple)) and len(epoch) == 1:
            epoch = epoch[0]
        if isinstance(epoch, bool) or not isinstance(epoch, int):
            raise ValueError("dedup takes exactly one epoch, --clustering.cached_epoch=<e>, not {!r}".format(epoch))
    return float(thr), view, out_path, report_path


def dedup(args):
    """the `dedup` verb: prints a summary line and the similarity_counts row, writes dedup.out_path (and dedup.report_path),
    returns the report"""
    import torch
    from .. import shards as io
    from . import cache
    from .evaluate import load_states
    from .frontend import FrontEnd
    from .row_groups import current_device, open_row_groups, probe_shards
    from .sgd_clustering import KMeans
    opts = args.get('dedup') or {}
    if args.clustering.cached_epoch is None:
        raise ValueError("dedup needs --clustering.cached_epoch=<e>: the epoch of the cluster run whose clusters block the pairs")
    check_options(opts, epoch=args.clustering.cached_epoch)  # refused before any cache or shard is read
    epoch = args.clustering.cached_epoch
    epoch = epoch[0] if isinstance(epoch, (list, tuple)) else epoch
    saved = load_states(args, [epoch])[epoch]
    names = OrderedDict(('/'.join(key[1:]), key) for key in saved)
    threshold, view, out_path, report_path = check_options(opts, views=sorted(names))

    paths = [Path(p) for p in sorted(io.brace_expand(args.data.path))]
    sizes = io.shard_sizes_from_meta(paths, args.data.meta.path, use_cache=True)
    paths = [p for p in paths if p.stem in sizes]
    _probe, view_dims = probe_shards(args, paths)
    if view_dims is None:
        raise ValueError("none of the {} shards of {} could be read".format(len(paths), args.data.path))
    v = next((key for key in view_dims if '/'.join(key[1:]) == view), None)
    if v is None:
        raise ValueError("the shards hold no view {} (they have {})".format(view, ', '.join('/'.join(key[1:]) for key in view_dims)))
    cview, cthr = check_confirm(opts, views=sorted(names), view=view)
    vb = None
    if cview is not None:
        vb = next((key for key in view_dims if '/'.join(key[1:]) == cview), None)
        if vb is None:
            raise ValueError("the shards hold no view {} (they have {})".format(cview, ', '.join('/'.join(key[1:]) for key in view_dims)))
    dev = current_device(args)
    dt = cache.find(saved, v)
    front = FrontEnd.from_attrs(dt)
    front.check_width(v, view_dims[v])
    d = front.width_out(view_dims[v])
    if dt['centers'].shape[1] != d:
        raise ValueError("the clustering cache of epoch {} lacks view {} (width {})".format(epoch, view, d))
    km = KMeans.load(dt)
    km.args = None  # one process, one GPU, whatever run wrote the cache
    km = km.to(dev)
    K = km.centers.shape[0]
    probes = check_probes(opts, K)
    against = check_against_options(opts)
    if against[0] is not None:
        return _dedup_against(args, against, paths, sizes, view_dims, v, dt, km, threshold, view, epoch, out_path, report_path,
                              probes)

    n_total = sum(int(sizes[p.stem]) for p in paths)
    need = 4 * n_total * d
    groups = open_row_groups(args, paths, sizes, view_dims)
    free, _total = torch.cuda.mem_get_info()
    beside = groups.budget // 2 if groups.streamed else 0  # a streamed group's rows lie beside the buffer they are copied into
    if need + beside > free:  # the one view in one piece, refused before the pass starts
        raise ValueError("dedup holds view {} in one piece: {} rows x {} columns need {} bytes on the device ({} more for a row "
                         "group), {} are free; dedup a part of the shards, or a projected view".format(
                             view, n_total, d, need, beside, free))
    groups.add_front_ends({v: front})
    x, base, shard_name, filename = None, 0, [], []
    for _gi, table, rows in groups.iterate(views={v}):
        part = rows[v]
        if x is None:
            x = part if not groups.streamed else torch.empty((n_total, d), dtype=torch.float32, device=part.device)
        if groups.streamed:
            if base + part.shape[0] > n_total:
                raise RuntimeError("the shards deliver more rows than their metadata states ({})".format(n_total))
            x[base:base + part.shape[0]] = part
        base += part.shape[0]
        shard_name.extend(table.shard_name)
        filename.extend(table.filename)
    if x is None or base != x.shape[0] or base != len(filename):
        raise RuntimeError("the shards delivered {} rows, their metadata states {}: fix the metadata or drop the unreadable shards "
                           "from the list".format(base, n_total))
    labels, _ = km.calc_best(x, need_mean=False)  # a row's label is a pure function of the row and the state
    groups_mode, keep, max_pairs, groups_path = check_groups(opts)
    if groups_mode:
        confirm = None
        if vb is not None:
            frontb = FrontEnd.from_attrs(cache.find(saved, vb))  # B is compared in the space it was clustered in
            frontb.check_width(vb, view_dims[vb])
            db = frontb.width_out(view_dims[vb])

            def second_view(rows):
                """the rows `rows` (ascending global row numbers) of view B after its front-end, gathered on the device one row
                group at a time: view B is never held in one piece by this pass (a streamed run reads the shards again)"""
                need_b = 4 * len(rows) * db
                beside_b = groups.budget // 2 if groups.streamed else 4 * n_total * max(view_dims[vb], db)
                free_b, _ = torch.cuda.mem_get_info()
                if need_b + beside_b > free_b:  # refused before the second pass starts
                    raise ValueError("dedup gathers the rows of view {} that occur in a pair: {} rows x {} columns need {} bytes on "
                                     "the device ({} more for a row group), {} are free; raise dedup.threshold, or dedup a part of "
                                     "the shards".format(cview, len(rows), db, need_b, beside_b, free_b))
                groups.add_front_ends({vb: frontb})
                buf = torch.empty((len(rows), db), dtype=torch.float32, device=x.device)
                at = 0
                for _gi, _table, rows_b in groups.iterate(views={vb}):
                    part = rows_b[vb]
                    lo, hi = (int(c) for c in np.searchsorted(rows, [at, at + part.shape[0]]))
                    if hi > lo:
                        buf[lo:hi] = part[torch.from_numpy(rows[lo:hi] - at).to(part.device)]
                    at += part.shape[0]
                if at != n_total:
                    raise RuntimeError("the second pass delivered {} rows, the first {}".format(at, n_total))
                return buf

            confirm = (cview, cthr, second_view)
        return _dedup_groups(args, km, x, labels, K, threshold, keep, max_pairs, view, epoch, out_path, groups_path, report_path,
                             (shard_name, filename), confirm)
    lists = each = None
    if probes == 1:
        best, partner = nearest_earlier(x, labels, k=K)
    else:  # the earlier rows of the m nearest centres' clusters: a partner may carry another label
        lists = km.probe_centers(x, probes, labels)
        best, partner, each = nearest_earlier(x, labels, k=K, probes=lists, each=True)
    labels = labels.cpu().numpy() if hasattr(labels, "cpu") else np.asarray(labels)

    report = summarise(best, partner, labels, K, threshold, probes=lists, best_each=each)
    report.update(view=view, epoch=int(epoch), feature_path=str(args.data.path), clusters_path=str(args.data.output.path))
    out_path = _write_csv(out_path, best, partner, threshold, (shard_name, filename), (shard_name, filename))
    print("dedup: view {} epoch {}: {} of {} rows ({:.3f}%) have an earlier row of their cluster at cosine >= {!r}; {} zero rows; "
          "wrote {}".format(view, epoch, report['flagged'], report['n'], 100.0 * report['flagged_share'], threshold,
                            report['zero_rows'], out_path))
    print("rows with best >= " + "  ".join("{}: {}".format(g, c) for g, c in report['similarity_counts'].items()))
    _print_probe_curve(report)
    _write_report(report_path, report)
    return report


def _dedup_groups(args, km, x, labels, K, threshold, keep, max_pairs, view, epoch, out_path, groups_path, report_path, names,
                  confirm=None):
    """the groups mode of the verb: every pair over the threshold, their connected components, one kept row per group.
    confirm (confirm_view, confirm_threshold, second_view: rows -> their rows of that view on the device): only the pairs that
    also reach confirm_threshold in the second view count"""
    best, partner, offsets, pair_j, pair_cos = pairs_earlier(x, labels, threshold, k=K, max_pairs=max_pairs)
    n = len(best)
    before = None
    if confirm is not None:
        cview, cthr, second_view = confirm
        root_a = components(n, offsets, pair_j)  # what view A alone would join: on the host, no device
        size_a = np.bincount(root_a, minlength=n)
        before = [('confirm_view', cview), ('confirm_threshold', cthr), ('pairs_before_confirm', int(offsets[n])),
                  ('groups_before_confirm', int((size_a >= 2).sum())), ('removed_before_confirm', int(n - (size_a >= 1).sum()))]
        cos_b = np.empty(0, np.float64)
        if offsets[n]:  # no pair in view A: nothing to confirm, the second pass is skipped
            _later, rows, ci, cj = pair_rows(offsets, pair_j)
            cos_b = pair_cosines(second_view(rows), ci, cj)
        before.append(('confirm_similarity_counts', confirm_similarity_counts(cos_b)))
        offsets, pair_j, pair_cos = confirm_pairs(offsets, pair_j, pair_cos, cos_b >= cthr)
    root = components(n, offsets, pair_j)
    a2 = km.quality(x, labels, rows=True)[1][:, 0] if keep == 'central' else None
    kept = choose_kept(root, keep, a2)
    report = summarise_groups(best, partner, _host(labels), K, threshold, offsets, root, kept, keep)
    if before is not None:  # flagged, similarity_counts and the nearest-earlier rule stay those of view A alone
        report.update(before)
    report.update(view=view, epoch=int(epoch), feature_path=str(args.data.path), clusters_path=str(args.data.output.path))
    out_path = _write_removed_csv(out_path, root, kept, pair_similarity(n, offsets, pair_j, pair_cos), names)
    if groups_path is not None:
        _write_groups_csv(groups_path, root, kept, names)
    print("dedup: view {} epoch {}: {} groups at cosine >= {!r} ({} pairs), {} of {} rows removed (keep={}), {} of them beyond the "
          "nearest-earlier rule; wrote {}".format(view, epoch, report['groups'], threshold, report['pairs'], report['removed'],
                                                  report['n'], keep, report['removed_beyond_nearest_rule'], out_path))
    print("groups of size " + "  ".join("{}: {}".format(b, c) for b, c in report['group_size_counts'].items()))
    if before is not None:
        print("confirmed in view {} at cosine >= {!r}: pairs {} -> {}, groups {} -> {}, removed rows {} -> {}; pairs with a cosine "
              "there >= ".format(report['confirm_view'], report['confirm_threshold'], report['pairs_before_confirm'], report['pairs'],
                                 report['groups_before_confirm'], report['groups'], report['removed_before_confirm'],
                                 report['removed'])
              + "  ".join("{}: {}".format(g, c) for g, c in report['confirm_similarity_counts'].items()))
    _write_report(report_path, report)
    return report


def _write_removed_csv(out_path, root, kept, similarity, names):
    """the rows that are not kept, in row order: shard_name,filename of the row, then of the kept row of its group, then
    repr(similarity) -- the largest cosine among the row's pairs -- and the group's size; overwritten"""
    out_path = Path(out_path)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    n = len(root)
    size = np.bincount(root, minlength=n)
    kept_of = np.full(n, -1, np.int64)
    kept_of[root[kept]] = np.flatnonzero(kept)
    with open(out_path, 'w', newline='') as f:
        writer = csv.writer(f)
        for i in np.flatnonzero(~np.asarray(kept, bool)):
            j = int(kept_of[root[i]])
            writer.writerow([names[0][i], names[1][i], names[0][j], names[1][j], repr(float(similarity[i])), int(size[root[i]])])
    return out_path


def _write_groups_csv(groups_path, root, kept, names):
    """every member of every group, kept ones included, by group (the row number of its root) and then by row:
    group,group_size,kept (1 or 0),shard_name,filename; overwritten"""
    groups_path = Path(groups_path)
    groups_path.parent.mkdir(parents=True, exist_ok=True)
    n = len(root)
    size = np.bincount(root, minlength=n)
    members = np.flatnonzero(size[root] >= 2)
    with open(groups_path, 'w', newline='') as f:
        writer = csv.writer(f)
        for i in members[np.argsort(root[members], kind='stable')]:
            writer.writerow([int(root[i]), int(size[root[i]]), int(bool(kept[i])), names[0][i], names[1][i]])
    return groups_path


def _print_probe_curve(report):
    """under the similarity grid: what each further probe finds (multi-probe runs only)"""
    if 'flagged_by_probes' in report:
        print("flagged within the first p probed clusters  " + "  ".join(
            "{}: {}".format(p + 1, c) for p, c in enumerate(report['flagged_by_probes'])) + "  ({} pairs compared)".format(report['pairs']))


def _host(labels):
    return labels.cpu().numpy() if hasattr(labels, "cpu") else np.asarray(labels)


def _write_csv(out_path, best, partner, threshold, names, partner_names):
    """the flagged rows in row order: shard_name,filename of the row, then of its partner, then repr(best); overwritten"""
    out_path = Path(out_path)
    out_path.parent.mkdir(parents=True, exist_ok=True)
    with open(out_path, 'w', newline='') as f:
        writer = csv.writer(f)
        for i in np.flatnonzero(flag(best, threshold)):
            j = int(partner[i])
            writer.writerow([names[0][i], names[1][i], partner_names[0][j], partner_names[1][j], repr(float(best[i]))])
    return out_path


def _write_report(report_path, report):
    if report_path is not None:
        report_path = Path(report_path)
        report_path.parent.mkdir(parents=True, exist_ok=True)
        with open(report_path, 'w') as f:
            json.dump(report, f, indent=1)


def _dedup_against(args, against, paths, sizes, view_dims, v, dt, km, threshold, view, epoch, out_path, report_path, probes=1):
    """the against mode of the verb: the held-out view resident in one device buffer, one pass over the pool's row groups;
    probes > 1 (blocking=cluster): the probe lists of a pool piece are computed per row group, the pool still streams"""
    import torch
    from .. import shards as io
    from .frontend import FrontEnd
    from .row_groups import open_row_groups, probe_shards
    against_path, against_meta, blocking = against
    K = km.centers.shape[0] if blocking == 'cluster' else 1
    hpaths = [Path(p) for p in sorted(io.brace_expand(against_path))]
    hsizes = io.shard_sizes_from_meta(hpaths, Path(against_meta), use_cache=True)
    hpaths = [p for p in hpaths if p.stem in hsizes]
    m_total = sum(int(hsizes[p.stem]) for p in hpaths)
    if m_total < 1:
        raise ValueError("the held-out set is empty: no shard of {} has rows in the metadata of {}".format(against_path, against_meta))
    _probe, hdims = probe_shards(args, hpaths)
    if hdims is None:
        raise ValueError("none of the {} held-out shards of {} could be read".format(len(hpaths), against_path))
    if v not in hdims:
        raise ValueError("the held-out shards hold no view {} (they have {})".format(view, ', '.join('/'.join(key[1:]) for key in hdims)))
    if hdims[v] != view_dims[v]:
        raise ValueError("view {} has {} columns in the held-out shards and {} in the pool's".format(view, hdims[v], view_dims[v]))
    fronts = [FrontEnd.from_attrs(dt), FrontEnd.from_attrs(dt)]  # one per set: a front-end tallies the rows it meets
    for front in fronts:
        front.check_width(v, view_dims[v])
    d = fronts[0].width_out(view_dims[v])

    n_total = sum(int(sizes[p.stem]) for p in paths)
    pool, held = open_row_groups(args, paths, sizes, view_dims), open_row_groups(args, hpaths, hsizes, hdims)
    need = 4 * m_total * d
    beside = (pool.budget // 2 if pool.streamed else 4 * n_total * view_dims[v]) + (held.budget // 2 if held.streamed else 0)
    free, _total = torch.cuda.mem_get_info()
    if need + beside > free:  # only the held-out view in one piece, refused before the pass starts
        raise ValueError("dedup holds view {} of the held-out set in one piece: {} rows x {} columns need {} bytes on the device "
                         "({} more for the row groups), {} are free; compare against a part of the held-out shards, or a "
                         "projected view".format(view, m_total, d, need, beside, free))
    pool.add_front_ends({v: fronts[0]})
    held.add_front_ends({v: fronts[1]})

    y, base, hshard, hfile = None, 0, [], []
    for _gi, table, rows in held.iterate(views={v}):
        part = rows[v]
        if y is None:
            y = part if not held.streamed else torch.empty((m_total, d), dtype=torch.float32, device=part.device)
        if held.streamed:
            if base + part.shape[0] > m_total:
                raise RuntimeError("the held-out shards deliver more rows than their metadata states ({})".format(m_total))
            y[base:base + part.shape[0]] = part
        base += part.shape[0]
        hshard.extend(table.shard_name)
        hfile.extend(table.filename)
    if y is None or base != y.shape[0] or base != len(hfile):
        raise RuntimeError("the held-out shards delivered {} rows, their metadata states {}: fix the metadata or drop the unreadable "
                           "shards from the list".format(base, m_total))
    against_zero = int((torch.count_nonzero(y, dim=1) == 0).sum())
    labels_y = hist_y = None
    if blocking == 'cluster':
        labels_y, _ = km.calc_best(y, need_mean=False)  # once: a row's label is a pure function of the row and the state
        hist_y = np.bincount(_host(labels_y), minlength=K)
    pairs = n_total * m_total if hist_y is None else None
    print("dedup: view {} epoch {}: {} pool rows against {} held-out rows, blocking={}{}".format(
        view, epoch, n_total, m_total, blocking, ": {} pairs".format(pairs) if pairs is not None else ""))

    best, partner, labels_x, pool_zero, shard_name, filename, lists, each = [], [], [], 0, [], [], [], []
    for _gi, table, rows in pool.iterate(views={v}):
        part = rows[v]
        lab = None
        if blocking == 'cluster':
            lab, _ = km.calc_best(part, need_mean=False)
            labels_x.append(_host(lab))
        if probes == 1:
            b, p = nearest_in(part, y, lab, labels_y, k=K)
        else:
            lists.append(km.probe_centers(part, probes, lab))
            b, p, e = nearest_in(part, y, lab, labels_y, k=K, probes_x=lists[-1], each=True)
            each.append(e)
        best.append(b)
        partner.append(p)
        pool_zero += int((torch.count_nonzero(part, dim=1) == 0).sum())
        shard_name.extend(table.shard_name)
        filename.extend(table.filename)
    best, partner = np.concatenate(best), np.concatenate(partner)
    if len(best) != n_total or len(filename) != n_total:
        raise RuntimeError("the shards delivered {} rows, their metadata states {}: fix the metadata or drop the unreadable shards "
                           "from the list".format(len(best), n_total))
    labels_x = np.concatenate(labels_x) if blocking == 'cluster' else None

    report = summarise_against(best, partner, labels_x, hist_y, K, threshold, m_total,
                               probes_x=np.concatenate(lists) if lists else None, best_each=np.concatenate(each) if each else None)
    report.update(view=view, epoch=int(epoch), feature_path=str(args.data.path), clusters_path=str(args.data.output.path),
                  against_path=str(against_path), blocking=blocking, pool_zero_rows=pool_zero, against_zero_rows=against_zero)
    out_path = _write_csv(out_path, best, partner, threshold, (shard_name, filename), (hshard, hfile))
    print("dedup: view {} epoch {}: {} of {} rows ({:.3f}%) have a held-out row at cosine >= {!r} ({} pairs compared, {} rows "
          "without candidates); wrote {}".format(view, epoch, report['flagged'], report['n'], 100.0 * report['flagged_share'],
                                                  threshold, report['pairs'], report['without_candidates'], out_path))
    print("rows with best >= " + "  ".join("{}: {}".format(g, c) for g, c in report['similarity_counts'].items()))
    _print_probe_curve(report)
    _write_report(report_path, report)
    return report
