"""CPU: the device-free side of the dedup against a held-out set -- acav_rows_crossdup_plan on hand-made histograms against
values worked out by hand from the rule include/acav_hip.h states, its refusals, dedup.check_options / check_against_options
for the new keys, summarise_against against hand-computed values, and the CLI keys."""
import ctypes as C

import numpy as np
import pytest

PLAN_LEN = 6
LDS64, LDS128 = 8 * 64 * 65, 8 * 128 * 65  # the float64 cosine tile over the two fp32 stages


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _plan(lib, hist_x, hist_y, d=8, cus=256):
    hx, hy = np.asarray(hist_x, np.int64), np.asarray(hist_y, np.int64)
    px, py = hx.ctypes.data_as(C.c_void_p), hy.ctypes.data_as(C.c_void_p)
    out = (C.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    assert lib.acav_rows_crossdup_plan(px, py, len(hx), d, cus, out, None, 0) == 0
    tiles = np.full((out[1], 4), -7, np.int64)
    again = (C.c_int64 * PLAN_LEN)()
    assert lib.acav_rows_crossdup_plan(px, py, len(hx), d, cus, again, tiles.ctypes.data_as(C.c_void_p), len(tiles)) == 0
    assert tuple(again) == tuple(out)
    return tuple(out), tiles.tolist()


def _scratch(n, m, tiles):
    # int32: both arrays' positions and two bounds per pool row; float64: the norms; 16 bytes per tile; (best, partner)
    return 4 * (3 * n + m) + 8 * (n + m) + 16 * tiles + 16 * n


# (hist_x, hist_y) -> (H, tiles, blocks, workgroups, LDS, scratch) and the list (first position, rows, first block, blocks)
HAND = [
    # no blocking: 100 pool rows are two 64-row tiles, each walks the three blocks of 150 held-out rows; ties by position
    ([100], [150], (64, 2, 6, 2, LDS64, _scratch(100, 150, 2)), [[0, 64, 0, 3], [64, 36, 0, 3]]),
    # tile 0 = pool positions 0 ... 63 spans the labels 0, 1, 2 (runs 0-29, 30-49, 50-89): from ystart[0] = 0 to yend[2] = 180,
    # three blocks; tile 1 = positions 64 ... 89 lies in label 2: [80, 180) starts in block 1 and ends in block 2
    ([30, 20, 40], [70, 10, 100], (64, 2, 5, 2, LDS64, _scratch(90, 180, 2)), [[0, 64, 0, 3], [64, 26, 1, 2]]),
    # the labels 1 and 2 have no held-out row: their tiles' range [130, 130) is empty, 0 blocks at first block floor(130 / 64);
    # label 3's five rows [130, 135) lie in block 2
    ([64, 64, 64, 10], [130, 0, 0, 5], (64, 4, 4, 4, LDS64, _scratch(202, 135, 4)),
     [[0, 64, 0, 3], [192, 10, 2, 1], [64, 64, 2, 0], [128, 64, 2, 0]]),
    # a tile that starts in a label without held-out rows and ends in one with 70
    ([10, 10], [0, 70], (64, 1, 2, 1, LDS64, _scratch(20, 70, 1)), [[0, 20, 0, 2]]),
    # descending blocks, ties by ascending first position: y's runs are [0, 100), [100, 110), [110, 210), [210, 220), i.e. the
    # blocks 0-1, 1, 1-3 and 3
    ([64, 64, 64, 64], [100, 10, 100, 10], (64, 4, 7, 4, LDS64, _scratch(256, 220, 4)),
     [[128, 64, 1, 3], [0, 64, 0, 2], [64, 64, 1, 1], [192, 64, 3, 1]]),
]


@pytest.mark.parametrize("hist_x,hist_y,want,want_tiles", HAND, ids=["-".join(map(str, h[0])) for h in HAND])
def test_plan_by_hand(lib, hist_x, hist_y, want, want_tiles):
    out, tiles = _plan(lib, hist_x, hist_y)
    assert out == want
    assert tiles == want_tiles


def test_tile_height_switches_where_128_row_tiles_fill_the_compute_units(lib):
    # on 4 compute units: ceil(384 / 128) = 3 < 4 keeps 64-row tiles, ceil(385 / 128) = 4 switches
    out, tiles = _plan(lib, [384], [10], cus=4)
    assert out == (64, 6, 6, 6, LDS64, _scratch(384, 10, 6)) and tiles == [[64 * t, 64, 0, 1] for t in range(6)]
    out, tiles = _plan(lib, [385], [10], cus=4)
    assert out == (128, 4, 4, 4, LDS128, _scratch(385, 10, 4))
    assert tiles == [[0, 128, 0, 1], [128, 128, 0, 1], [256, 128, 0, 1], [384, 1, 0, 1]]
    # the height follows the pool rows alone: a large held-out set does not change it
    assert _plan(lib, [384], [100000], cus=4)[0][0] == 64
    # a 128-row tile over three labels: positions 0 ... 127 of the runs 0-49, 50-99, 100-384
    out, tiles = _plan(lib, [50, 50, 285], [64, 64, 1], cus=4)
    assert out[0] == 128 and sorted(tiles) == [[0, 128, 0, 3], [128, 128, 2, 1], [256, 128, 2, 1], [384, 1, 2, 1]]


def test_plan_refusals(lib):
    out = (C.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    hx, hy = np.array([300, 70], np.int64), np.array([5, 5], np.int64)
    px, py = hx.ctypes.data_as(C.c_void_p), hy.ctypes.data_as(C.c_void_p)
    tiles = np.zeros((5, 4), np.int64)
    for args in ((None, py, 2, 8, 256, out, None, 0), (px, None, 2, 8, 256, out, None, 0), (px, py, 2, 8, 256, None, None, 0),
                 (px, py, 0, 8, 256, out, None, 0), (px, py, 2, 0, 256, out, None, 0), (px, py, 2, 16385, 256, out, None, 0),
                 (px, py, 2, 8, 0, out, None, 0),
                 (px, py, 2, 8, 256, out, tiles.ctypes.data_as(C.c_void_p), 5)):  # 370 rows are 6 tiles
        assert lib.acav_rows_crossdup_plan(*args) == -1, args
    for bad in ([-1, 5], [0, 0], [2 ** 31, 0], [2 ** 30, 2 ** 30]):
        b = np.array(bad, np.int64)
        pb = b.ctypes.data_as(C.c_void_p)
        assert lib.acav_rows_crossdup_plan(pb, py, 2, 8, 256, out, None, 0) == -1, bad
        assert lib.acav_rows_crossdup_plan(px, pb, 2, 8, 256, out, None, 0) == -1, bad
    assert tuple(out) == (-7,) * PLAN_LEN and not tiles.any()


def test_check_options_for_the_new_keys():
    from acav100m_amd.clustering.dedup import check_against_options, check_options
    ok = {'threshold': 0.95, 'out_path': 'dups.csv'}
    assert check_against_options(ok) == (None, None, None)
    against = dict(ok, against_path='held/shard-{000000..000001}.pkl', against_meta_path='held/videos')
    assert check_options(against) == (0.95, None, 'dups.csv', None)  # the old answer: the new keys are only checked
    assert check_against_options(against) == ('held/shard-{000000..000001}.pkl', 'held/videos', 'none')
    assert check_against_options(dict(against, blocking='cluster'))[2] == 'cluster'
    assert check_against_options(dict(against, blocking='none'))[2] == 'none'
    for bad, match in ((dict(ok, against_path='held/x.pkl'), "against_meta_path"),
                       (dict(ok, blocking='cluster'), "only valid with"), (dict(ok, blocking='none'), "only valid with"),
                       (dict(ok, against_meta_path='held/videos'), "only valid with"),
                       (dict(against, blocking='probe'), "dedup.blocking"), (dict(against, blocking=True), "dedup.blocking"),
                       (dict(against, against_path=7), "against_path"), (dict(against, against_path=''), "against_path")):
        with pytest.raises(ValueError, match=match):
            check_options(bad)
        with pytest.raises(ValueError, match=match):
            check_against_options(bad)


def test_summarise_against_by_hand():
    from acav100m_amd.clustering.dedup import SIMILARITY_GRID, summarise_against
    inf = np.inf
    best = np.array([0.9999995, 0.5, -inf, -inf, 0.97, -inf])
    partner = np.array([2, 0, -1, -1, 4, -1])
    labels_x, hist_y = np.array([0, 0, 1, 1, 2, 2]), [3, 0, 2]
    got = summarise_against(best, partner, labels_x, hist_y, 3, 0.95, 5)
    counts = dict(zip(map(repr, SIMILARITY_GRID), [3, 2, 2, 2, 2, 2, 1, 1, 1, 1]))
    assert dict(got) == {
        'n': 6, 'm': 5, 'K': 3, 'threshold': 0.95, 'flagged': 2, 'flagged_share': 2 / 6, 'flagged_by_cluster': [1, 0, 1],
        'similarity_counts': counts,
        'pairs': 2 * 3 + 2 * 0 + 2 * 2,  # sum over the clusters of pool rows x held-out rows
        'without_candidates': 2,         # the two pool rows of cluster 1; cluster 2's last row has candidates and no partner
    }
    # a cluster whose held-out rows are all zero: it has rows in hist_y and still no candidate
    none = summarise_against(np.full(3, -inf), np.full(3, -1), np.array([0, 0, 0]), [4], 1, 0.9, 4)
    assert none['pairs'] == 12 and none['without_candidates'] == 3 and none['flagged'] == 0
    # no blocking: n m pairs, one cluster, no flagged_by_cluster
    flat = summarise_against(best, partner, None, None, 1, 0.95, 5)
    assert dict(flat) == {'n': 6, 'm': 5, 'K': 1, 'threshold': 0.95, 'flagged': 2, 'flagged_share': 2 / 6,
                          'similarity_counts': counts, 'pairs': 30, 'without_candidates': 0}
    for bad in (dict(labels_x=labels_x, hist_y=None, k=3), dict(labels_x=None, hist_y=hist_y, k=3), dict(labels_x=None, hist_y=None, k=3),
                dict(labels_x=labels_x, hist_y=[3, 0, 1], k=3), dict(labels_x=labels_x[:5], hist_y=hist_y, k=3)):
        with pytest.raises(ValueError):
            summarise_against(best, partner, bad['labels_x'], bad['hist_y'], bad['k'], 0.95, 5)


def test_parse_cli_reads_the_new_keys_and_the_defaults_gain_none():
    from acav100m_amd.config import CLUSTERING_DEFAULTS, merge, parse_cli
    command, kwargs = parse_cli(['dedup', '--feature_path=f', '--clustering.cached_epoch=3', '--dedup.threshold=0.999999',
                                 '--dedup.out_path=dups.csv', '--dedup.against_path=held/shard-{000000..000003}.pkl',
                                 '--dedup.against_meta_path=held/videos', '--dedup.blocking=cluster'])
    args = merge(CLUSTERING_DEFAULTS, kwargs)
    assert command == 'dedup' and args.get('dedup') == {
        'threshold': 0.999999, 'out_path': 'dups.csv', 'against_path': 'held/shard-{000000..000003}.pkl',
        'against_meta_path': 'held/videos', 'blocking': 'cluster'}
    assert 'dedup' not in CLUSTERING_DEFAULTS
