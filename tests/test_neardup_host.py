"""CPU: the device-free side of the near-duplicate feature -- acav_rows_neardup_plan against the rule include/acav_hip.h states
(a hand-derived table for the small histograms, a restatement of the rule for the large ones), the tile list's cover and order,
(the grid is one workgroup per tile, uncapped: there is no second round of a grid to plan), the refusals of the plan and of
dedup.check_options, the exclude list of `subset_selection run --exclude_path`, and the CLI keys."""
import ctypes as C
import hashlib
import json

import numpy as np
import pytest

PLAN_LEN = 6


@pytest.fixture(scope="module")
def lib():
    import acav100m_amd
    return acav100m_amd.load_library()


def _plan(lib, hist, d=8, cus=256, want_tiles=True):
    h = np.asarray(hist, np.int64)
    out = (C.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    assert lib.acav_rows_neardup_plan(h.ctypes.data_as(C.c_void_p), len(h), d, cus, out, None, 0) == 0
    if not want_tiles:
        return tuple(out), None
    tiles = np.full((out[1], 4), -7, np.int64)
    again = (C.c_int64 * PLAN_LEN)()
    assert lib.acav_rows_neardup_plan(h.ctypes.data_as(C.c_void_p), len(h), d, cus, again, tiles.ctypes.data_as(C.c_void_p), len(tiles)) == 0
    assert tuple(again) == tuple(out)
    return tuple(out), tiles


def _rule(hist, cus):
    """the rule as the header states it, tile by tile: (H, [(first position, rows, first block, blocks)] in tile order)"""
    n = int(sum(hist))
    H = 128 if -(-n // 128) >= cus else 64
    starts = np.repeat(np.cumsum(hist) - np.asarray(hist), hist)  # per sorted position: where its run starts
    tiles = []
    for q0 in range(0, n, H):
        q1 = min(n, q0 + H)
        cb0, cb1 = int(starts[q0]) // 64, (q1 - 1) // 64
        tiles.append((q0, q1 - q0, cb0, cb1 - cb0 + 1))
    return H, tiles


# hist -> (H, tiles, column blocks walked, workgroups, LDS bytes, scratch bytes) on 256 compute units, derived by hand from the
# rule: 64-row tiles (n < 128 * 256); tile t of ONE cluster walks the blocks 0 ... t, so T tiles walk T (T + 1) / 2;
# LDS = 8 * 64 * 65 (the float64 cosine tile over the two fp32 stages of 4 * 128 * 36); scratch = 32 n + 16 tiles
SMALL = [
    ([1], (64, 1, 1, 1, 33280, 48)), ([63], (64, 1, 1, 1, 33280, 2032)), ([64], (64, 1, 1, 1, 33280, 2064)),
    ([65], (64, 2, 3, 2, 33280, 2112)), ([129], (64, 3, 6, 3, 33280, 4176)), ([300], (64, 5, 15, 5, 33280, 9680)),
    # 371 rows: tiles 0 ... 3 lie in the first run (1 + 2 + 3 + 4 blocks), tile 4 = positions 256 ... 319 starts in it (blocks
    # 0 ... 4: 5), tile 5 = positions 320 ... 370 starts in the last run, which begins at 301 = block 4 (blocks 4 ... 5: 2)
    ([300, 0, 1, 70], (64, 6, 17, 6, 33280, 11968)),
]


@pytest.mark.parametrize("hist,want", SMALL, ids=["-".join(map(str, h)) for h, _ in SMALL])
def test_plan_table_small(lib, hist, want):
    out, tiles = _plan(lib, hist)
    assert out == want
    H, rule = _rule(hist, 256)
    assert sorted(map(tuple, tiles.tolist())) == sorted(rule)


def test_plan_tile_list_of_the_mixed_histogram(lib):
    _out, tiles = _plan(lib, [300, 0, 1, 70])
    # descending blocks, ties by ascending first position: the two-block tiles are positions 64 (first run) and 320 (last run)
    assert tiles.tolist() == [[256, 64, 0, 5], [192, 64, 0, 4], [128, 64, 0, 3], [64, 64, 0, 2], [320, 51, 4, 2], [0, 64, 0, 1]]


HIST_133 = [300 + (c % 7) - 3 for c in range(133)]  # 39 900 rows, clusters of 297 ... 303


@pytest.mark.parametrize("cus", [256, 8])
def test_plan_133_clusters(lib, cus):
    out, tiles = _plan(lib, HIST_133, d=8, cus=cus)
    n = sum(HIST_133)
    assert n == 39900
    H, rule = _rule(HIST_133, cus)
    assert H == 128  # ceil(39900 / 128) = 312 tiles of 128 rows give every one of 256 compute units a workgroup
    assert out == (128, 312, sum(t[3] for t in rule), 312, 8 * 128 * 65, 32 * n + 16 * 312)
    assert sorted(map(tuple, tiles.tolist())) == sorted(rule)
    # 64-row tiles when 128-row tiles would leave compute units idle
    out64, _ = _plan(lib, HIST_133, d=8, cus=313, want_tiles=False)
    assert out64[:2] == (64, 624) and out64[3:5] == (624, 33280)


@pytest.mark.parametrize("hist,cus", [([300, 0, 1, 70], 256), (HIST_133, 256), (HIST_133, 313), ([5000, 3, 0, 777, 64, 64, 1], 4)])
def test_tile_list_covers_every_position_once_in_triangular_ranges_by_descending_blocks(lib, hist, cus):
    out, tiles = _plan(lib, hist, cus=cus)
    n, H = sum(hist), out[0]
    seen = np.zeros(n, np.int64)
    starts = np.repeat(np.cumsum(hist) - np.asarray(hist), hist)
    for q0, rows, cb0, blocks in tiles.tolist():
        assert q0 % H == 0 and 1 <= rows <= H
        seen[q0:q0 + rows] += 1
        # from the block of the start of the first row's run up to the block of the tile's own last row: every earlier row of
        # the cluster of every row of the tile lies in them, and no block after the tile
        assert cb0 == starts[q0] // 64 and cb0 + blocks - 1 == (q0 + rows - 1) // 64
        assert all(starts[p] // 64 >= cb0 for p in range(q0, q0 + rows))
    assert (seen == 1).all()
    assert tiles[:, 3].sum() == out[2]
    key = [(-b, q) for q, _r, _c, b in tiles.tolist()]
    assert key == sorted(key)


def test_plan_refusals(lib):
    out = (C.c_int64 * PLAN_LEN)(*([-7] * PLAN_LEN))
    h = np.array([300, 70], np.int64)
    hp = h.ctypes.data_as(C.c_void_p)
    tiles = np.zeros((5, 4), np.int64)
    for args in ((None, 2, 8, 256, out, None, 0), (hp, 2, 8, 256, None, None, 0), (hp, 0, 8, 256, out, None, 0),
                 (hp, 2, 0, 256, out, None, 0), (hp, 2, 16385, 256, out, None, 0), (hp, 2, 8, 0, out, None, 0),
                 (hp, 2, 8, 256, out, tiles.ctypes.data_as(C.c_void_p), 5)):  # 370 rows are 6 tiles
        assert lib.acav_rows_neardup_plan(*args) == -1, args
    for bad in ([-1, 5], [0, 0], [2 ** 31, 0], [2 ** 30, 2 ** 30]):
        b = np.array(bad, np.int64)
        assert lib.acav_rows_neardup_plan(b.ctypes.data_as(C.c_void_p), 2, 8, 256, out, None, 0) == -1, bad
    assert tuple(out) == (-7,) * PLAN_LEN and not tiles.any()


def test_check_options():
    from acav100m_amd.clustering.dedup import check_options
    ok = {'threshold': 0.95, 'out_path': 'dups.csv'}
    assert check_options(ok) == (0.95, None, 'dups.csv', None)
    assert check_options(dict(ok, threshold=1, report_path='r.json', view='m/l'), views=['m/l', 'm/k'], epoch=[3]) == \
        (1.0, 'm/l', 'dups.csv', 'r.json')
    assert check_options(ok, views=['m/l'], epoch=2)[1] == 'm/l'  # one view: it is the one
    for bad in ({'out_path': 'x'}, dict(ok, threshold=0), dict(ok, threshold=0.0), dict(ok, threshold=1.5), dict(ok, threshold=True),
                dict(ok, threshold='0.9'), dict(ok, threshold=-0.5), dict(ok, threshold=float('nan')), {'threshold': 0.9},
                dict(ok, view='nolayer')):
        with pytest.raises(ValueError):
            check_options(bad)
    with pytest.raises(ValueError, match="dedup.view is required"):
        check_options(ok, views=['m/l', 'm/k'])
    with pytest.raises(ValueError, match="not a view"):
        check_options(dict(ok, view='m/x'), views=['m/l', 'm/k'])
    for epochs in ([1, 2], [], True, 'last'):
        with pytest.raises(ValueError, match="exactly one epoch"):
            check_options(ok, epoch=epochs)


def test_exclude_reader_and_filter(tmp_path):
    from acav100m_amd.subset_selection import exclude
    shard_names = ['s0', 's0', 's0', 's1', 's1', 's2']
    filenames = ['a.mp4', 'b.mp4', 'c.mp4', 'a.mp4', 'd.mp4', 'e.mp4']
    assignments = np.arange(12, dtype=np.int64).reshape(6, 2)
    types = [('m', 'l0'), ('m', 'l1')]
    # the dedup file's shape: five columns; the file name matches on its stem
    dups = tmp_path / 'dups.csv'
    dups.write_text("s0,b.mp4,s0,a.mp4,0.9999999\ns1,a.wav,s0,a.mp4,1.0\n\ns9,zz.mp4,s0,a.mp4,1.0\ns0,d.mp4,s0,a.mp4,1.0\n")
    keys = exclude.read_exclude(dups)
    assert keys == {('s0', 'b'), ('s1', 'a'), ('s9', 'zz'), ('s0', 'd')}
    keep, unknown = exclude.keep_mask(keys, shard_names, filenames)
    assert keep.tolist() == [True, False, True, False, True, True] and unknown == 2  # s9/zz, and d is in s1, not in s0
    got = exclude.apply_exclude(keys, (assignments, types, shard_names, filenames))
    assert np.array_equal(got[0], assignments[keep]) and got[0].flags['C_CONTIGUOUS'] and got[1] is types
    assert got[2] == ['s0', 's0', 's1', 's2'] and got[3] == ['a.mp4', 'c.mp4', 'd.mp4', 'e.mp4']
    # an output.csv of an earlier run: shard_name,filename,id,segment (the segment holds a comma, quoted by the csv module)
    out = tmp_path / 'output.csv'
    out.write_text('s2,e.mp4,vid5,"[10, 20]"\r\ns0,a.mp4,vid0,"[10, 20]"\r\n')
    keys = exclude.read_exclude(out)
    assert keys == {('s2', 'e'), ('s0', 'a')}
    assert exclude.keep_mask(keys, shard_names, filenames)[0].tolist() == [False, True, True, True, True, False]
    (tmp_path / 'short.csv').write_text("s0\n")
    with pytest.raises(ValueError, match="line 1"):
        exclude.read_exclude(tmp_path / 'short.csv')
    # an empty list drops nothing
    (tmp_path / 'none.csv').write_text("")
    assert exclude.keep_mask(exclude.read_exclude(tmp_path / 'none.csv'), shard_names, filenames)[0].all()


@pytest.mark.parametrize("measure", ["contrastive", "pca_cs", "pca"])
def test_exclude_is_refused_for_measures_that_read_feature_shards(measure, tmp_path):
    from acav100m_amd.subset_selection import exclude
    from acav100m_amd.subset_selection.cli import check_run, get_args
    with pytest.raises(ValueError, match="exclude_path"):
        exclude.check_exclude(measure, 'x.csv')
    exclude.check_exclude(measure, None)
    exclude.check_exclude('mi', 'x.csv')
    args = get_args(measure_name=measure, exclude_path=str(tmp_path / 'missing.csv'))
    with pytest.raises(ValueError, match="exclude_path"):  # before anything is read: the file does not even exist
        check_run(args)


def test_parse_cli_round_trip_and_the_defaults_stay():
    from acav100m_amd.config import CLUSTERING_DEFAULTS, SUBSET_DEFAULTS, merge, parse_cli
    command, kwargs = parse_cli(['dedup', '--feature_path=f', '--clustering.cached_epoch=3', '--dedup.threshold=0.999999',
                                 '--dedup.view=layer_vggish/layer_4', '--dedup.out_path=dups.csv', '--dedup.report_path=r.json'])
    assert command == 'dedup'
    args = merge(CLUSTERING_DEFAULTS, kwargs)
    assert args.get('dedup') == {'threshold': 0.999999, 'view': 'layer_vggish/layer_4', 'out_path': 'dups.csv', 'report_path': 'r.json'}
    assert args.clustering.cached_epoch == 3
    command, kwargs = parse_cli(['run', '--exclude_path=dups.csv', '--measure_name=mi'])
    args = merge(SUBSET_DEFAULTS, kwargs)
    assert command == 'run' and args.get('exclude_path') == 'dups.csv'
    assert merge(SUBSET_DEFAULTS, {}).get('exclude_path') is None and merge(CLUSTERING_DEFAULTS, {}).get('dedup') is None
    # the new keys are read with args.get: neither dictionary gained one, by value
    assert 'exclude_path' not in SUBSET_DEFAULTS and 'dedup' not in CLUSTERING_DEFAULTS
    digest = lambda tree: hashlib.sha256(json.dumps(tree, sort_keys=True).encode()).hexdigest()  # noqa: E731
    assert digest(SUBSET_DEFAULTS) == SUBSET_DIGEST
    assert digest(CLUSTERING_DEFAULTS) == CLUSTERING_DIGEST


# sha256 of json.dumps(<defaults>, sort_keys=True) as the dictionaries stood before the near-duplicate feature
SUBSET_DIGEST = "bd501b3882db7aafcf78ed331ae183cd218dad5663f762b43c0ca066663265ac"
CLUSTERING_DIGEST = "a19715a6ff11702f53bfa8aea54abb7060b6f02848a2f04eab4a69ea080f8921"
