"""The device MT19937 stream (k_mt_generate_lanes + k_mt_jump behind MtStream, read back by acav_mt_stream_fill) equals the
host generator word for word, at the sizes where the generator's sliding LDS window and the streaming jump can go wrong.

The window holds MT_BACK = 1078 words plus MT_WIDE = 623 words per step and slides every MT_EPOCH = 9 steps, counted in
stream words from word 0 of the host state's block: the first slide happens when word 1078 + 623 * 9 = 6685 is due.  A start
index idx makes draw r the stream word idx + r, so the four start indices move every boundary by 0, 1, 623 and 624 draws.

Host references: the short cases against acav100m_amd.rng word by word (u32), read once; the long case against numpy's
MT19937 loaded with the same state, which the host-only test below pins to the host generator (first words, and the state
acav_rng_jump leaves for every jump distance whose polynomial the fills use)."""
import numpy as np
import pytest

MT_BACK, MT_WIDE, MT_EPOCH = 1078, 623, 9
FIRST_SLIDE = MT_BACK + MT_WIDE * MT_EPOCH
SEED = 20240
N_SHORT = 624 + 3 * 4 * 624 * 32 + 1024  # the longest short case, from word 0 of the state's block
BLK_PRODUCT = 624 * 4096                  # the product's lane block


@pytest.fixture(scope="module")
def acav():
    import acav100m_amd
    acav100m_amd.load_library()
    return acav100m_amd


@pytest.fixture(scope="module")
def gpu(acav):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return acav


@pytest.fixture(scope="module")
def state(acav):
    """A state block in mid-stream (not a freshly seeded array): mt[624]."""
    g = acav.Generator(SEED)
    g.jump(5000)
    mt, _ = g.get_state()
    mt.setflags(write=False)
    return mt


@pytest.fixture(scope="module")
def host_words(acav, state):
    """Tempered words of the stream from word 0 of `state`, drawn one by one from the host generator."""
    g = acav.Generator(0)
    g.set_state(state, 0)
    out = np.fromiter((g.u32() for _ in range(N_SHORT)), np.uint32, N_SHORT)
    out.setflags(write=False)
    return out


def _numpy_mt(state, idx):
    bg = np.random.MT19937()
    bg.state = {"bit_generator": "MT19937", "state": {"key": np.array(state, np.uint32), "pos": int(idx)}}
    return bg


def _temper(y):
    y = y.copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9d2c5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xefc60000)
    y ^= y >> np.uint32(18)
    return y


def _fill(state, idx, n, blk, W):
    from acav100m_amd import _lib
    out = np.full(n + 16, 0xdeadbeef, np.uint32)  # nothing may be written past draw n
    _lib.check(_lib.load_library().acav_mt_stream_fill(_lib.ptr(np.ascontiguousarray(state)), idx, n, blk, W, _lib.ptr(out)))
    assert (out[n:] == 0xdeadbeef).all()
    return _temper(out[:n])


def _single_block(idx, n):
    """the plan's own block for a short run: one lane block, cut to size"""
    gen = max(n - (624 - idx), 0)
    return 624 * max((gen + 623) // 624, 1)


SHORT_N = [1, 623, 624, 1077, 1078, 1079, FIRST_SLIDE - 1, FIRST_SLIDE, FIRST_SLIDE + 1,
           MT_BACK + 2 * MT_WIDE * MT_EPOCH + 5]


@pytest.mark.gpu
@pytest.mark.parametrize("idx", [0, 1, 623, 624])
@pytest.mark.parametrize("n", SHORT_N)
def test_one_lane_block_equals_host_stream(gpu, state, host_words, idx, n):
    got = _fill(state, idx, n, _single_block(idx, n), 1)
    want = host_words[idx:idx + n]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"first differing draw {bad[0]} of {n} (stream word {idx + bad[0]})"


@pytest.mark.gpu
@pytest.mark.parametrize("blk", [624 * 3, 624 * 32])  # t^blk is a single term / a dense polynomial (blk > 19937)
@pytest.mark.parametrize("W", [1, 2, 4])
def test_ring_wraps_and_lanes_jump_twice(gpu, state, host_words, W, blk):
    idx = 1
    n = (624 - idx) + 3 * W * blk - 7  # three superblocks over the two-slot ring, the last one cut short
    got = _fill(state, idx, n, blk, W)
    want = host_words[idx:idx + n]
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"first differing draw {bad[0]} of {n}: lane block {(bad[0] - 623) // blk}"


@pytest.mark.gpu
def test_product_block_and_jump_polynomial(gpu, state, host_words):
    """Two lanes of the product's block length, two superblocks: lane 1 starts from t^blk, lane 0 moves on by t^(2 blk)."""
    idx, W = 624, 2
    n = 2 * BLK_PRODUCT + 1000
    got = _fill(state, idx, n, BLK_PRODUCT, W)
    want = _numpy_mt(state, idx).random_raw(n).astype(np.uint32)
    assert np.array_equal(want[:4096], host_words[idx:idx + 4096])
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"first differing draw {bad[0]} of {n}: lane block {bad[0] // BLK_PRODUCT}"


@pytest.mark.parametrize("J", sorted({blk << r for blk in (624 * 3, 624 * 32) for r in range(3)} | {BLK_PRODUCT, 2 * BLK_PRODUCT}))
def test_host_jump_polynomials_of_the_fills(acav, state, host_words, J):
    """Host only.  The fills above jump their lanes by t^(2^r blk), the polynomials acav_rng_jump derives for the same
    distances: the state it leaves equals the one J sequential draws leave (numpy's MT19937, itself equal to the host
    generator on its first words)."""
    bg = _numpy_mt(state, 624)
    assert np.array_equal(bg.random_raw(8192).astype(np.uint32), host_words[624:624 + 8192])
    bg = _numpy_mt(state, 624)
    bg.random_raw(J)
    want = bg.state["state"]
    g = acav.Generator(0)
    g.set_state(state, 624)
    g.jump(J)
    mt, pos = g.get_state()
    assert pos == int(want["pos"]) == 624
    assert np.array_equal(mt, np.asarray(want["key"], np.uint32))
