"""k-means++ (D^2) seeding for batch k-means: the initial centres of clustering.algorithm=lloyd under clustering.init=kmeans++ --
what scipy's kmeans2(minit='++') and sklearn's KMeans run; with several local trials per pick it is sklearn's greedy variant.

Definition.  Seeding runs on a sample x [m, d] (fp32, resident on the device in one piece) and returns K row indices into it.
All randomness enters as a host array u of float64 values in [0, 1).
  weight   of row i against the sample row c with shift t:  e_j = double(x_ij) - double(x_cj), p_j = e_j * e_j, D = sum_j p_j,
           W(i, c) = int64(rint(D * 2^t)).  Every operation is one rounded float64 operation (no fma), and the sum runs in one
           order that depends on d alone: lane (j // 4) % 64 owns column j and chains the p_j of its columns from +0.0 in
           ascending j; the 64 lane values are summed by an xor-butterfly, v[l] + v[l ^ o] for o = 32 ... 1.  W(c, c) = 0.
  shift    t = weight_shift(absmax of the sample, m, d): every sum of m weights stays below 2^62
  picks    with T trials per pick and u of length 1 + (K - 1) T:
           pick 0       r = min(m - 1, int(u[0] * m)), w_i = W(i, r), potential[0] = sum_i w_i
           pick s >= 1  total = sum_i w_i (0: the sample holds fewer than K distinct rows, a ValueError); for tau < T:
                        target = min(total - 1, int(u[1 + (s - 1) T + tau] * float(total))), r_tau = the least i with
                        w_0 + ... + w_i > target, pot_tau = sum_i min(w_i, W(i, r_tau)); the trial of least pot wins (the lowest
                        tau on ties): rows[s] = its row, w_i <- min(w_i, W(i, row)), potential[s] = its pot
All sums are integers, so rows and potential are a pure function of (x, K, T, u): not of the device, the grid or where x lives.
The sweeps are GPU kernels (acav_kmeanspp.hip; there is no CPU path); tests/_kmeanspp_np.py restates the seeding in numpy bit
for bit."""
import ctypes as C
import math

import numpy as np

from .. import _lib
from .sgd_clustering import _as_f32_2d, _device_index

INITS = ('random', 'kmeans++')
MAX_TRIALS = 16
MAX_SHIFT = 1000          # |t|: 2^t stays a normal double (the library's bound)
SAMPLE_PER_CENTRE = 256   # rows of the default sample per centre (faiss's max_points_per_centroid)


def _bl(n):
    return (max(int(n), 2) - 1).bit_length()


def weight_shift(absmax, m, d):
    """t = 59 - bl(m) - bl(d) - 2 E with bl(n) = bit_length(max(n, 2) - 1) (so n <= 2^bl(n)) and (_, E) = frexp(absmax).
    Proof that m weights sum to less than 2^62: |x| <= absmax < 2^E, so |e_j| < 2^(E + 1) (a difference of two fp32 values is
    exact in float64 or rounds monotonically below that power of two) and p_j <= 2^(2 E + 2).  A partial sum of n such terms is at
    most n 2^(2 E + 2), a representable bound that rounding to nearest cannot cross, so D <= d 2^(2 E + 2) <= 2^(bl(d) + 2 E + 2)
    whatever the order of the sum.  Then W <= 2^(bl(d) + 2 E + 2 + t) = 2^(61 - bl(m)) and m W <= 2^61."""
    absmax, m, d = float(absmax), int(m), int(d)
    if not math.isfinite(absmax) or absmax < 0:
        raise ValueError("absmax = {!r} is not a finite magnitude".format(absmax))
    if m < 1 or d < 1:
        raise ValueError("a sample of {} rows and {} columns".format(m, d))
    _m, e = math.frexp(absmax)
    t = 59 - _bl(m) - _bl(d) - 2 * e
    if abs(t) > MAX_SHIFT:
        raise ValueError("weight shift 2^{}: |t| must stay within {} (2^t a normal double)".format(t, MAX_SHIFT))
    return t


def uniforms(generator, count):
    """count float64 values in [0, 1): ((a >> 5) * 2^26 + (b >> 6)) / 2^53 from two successive generator.u32() draws a, b
    (MT19937's genrand_res53)"""
    out = np.empty(int(count), np.float64)
    for i in range(int(count)):
        a, b = generator.u32(), generator.u32()
        out[i] = ((a >> 5) * 67108864 + (b >> 6)) / 9007199254740992.0
    return out


def trials_for(k, trials):
    """local trials per pick: 1 is the classical algorithm, 'auto' min(16, 2 + floor(ln k)) (sklearn's rule), an int in [1, 16]
    is taken as is"""
    if trials == 'auto':
        return min(MAX_TRIALS, 2 + int(math.floor(math.log(max(int(k), 1)))))
    if isinstance(trials, bool) or not isinstance(trials, (int, np.integer)) or not 1 <= int(trials) <= MAX_TRIALS:
        raise ValueError("clustering.init_trials must be 'auto' or an integer in [1, {}], not {!r}".format(MAX_TRIALS, trials))
    return int(trials)


def check_init(args):
    """clustering.init is 'random' or 'kmeans++' (lloyd only); clustering.init_trials is 'auto' or in [1, 16];
    clustering.init_sample is None or an integer >= clustering.ncentroids.  Pure: no device, no file.  -> the init"""
    init = 'random' if args.clustering.init is None else args.clustering.init  # (a hand-built args tree without the key)
    if not isinstance(init, str) or init not in INITS:
        raise ValueError("clustering.init must be 'random' or 'kmeans++', not {!r}".format(init))
    if init == 'kmeans++':
        algo = args.clustering.algorithm or 'sgd'
        if algo != 'lloyd':
            raise ValueError("clustering.init=kmeans++ seeds batch k-means: it needs clustering.algorithm=lloyd, not {!r}".format(algo))
        trials = args.clustering.init_trials
        trials_for(int(args.clustering.ncentroids), 1 if trials is None else trials)
        sample = args.clustering.init_sample
        if sample is not None:
            if isinstance(sample, bool) or not isinstance(sample, int) or sample < int(args.clustering.ncentroids):
                raise ValueError("clustering.init_sample={!r} must be None or an integer of at least clustering.ncentroids={}".format(
                    sample, args.clustering.ncentroids))
    return init


def sample_size(n, k, sample=None):
    """rows of the seeding sample: min(n, sample or 256 k)"""
    return min(int(n), int(sample) if sample is not None else SAMPLE_PER_CENTRE * int(k))


def weights(x, cand_rows, t, stream=None):
    """W(i, c) of every row i of x [m, d] (numpy or torch, host or device) against each row c of cand_rows, with shift t ->
    int64 numpy [T, m]: acav_kmeanspp_weights"""
    keep, xp, m, on_gpu = _as_f32_2d(x)
    d = int(keep.shape[1])
    cand = np.ascontiguousarray(cand_rows, np.int64).reshape(-1)
    out = np.empty((len(cand), m), np.int64)
    lib = _lib.load_library()
    _lib.check(lib.acav_kmeanspp_weights(keep.device.index if on_gpu else _device_index("cuda"), xp, m, d, _lib.ptr(cand), len(cand),
                                         int(t), _lib.ptr(out), stream))
    return out


def seed(x, k, trials=1, generator=None, u=None, stream=None):
    """k seeds of the sample x [m, d] (numpy or torch, host or device) -> (rows int64 [k], potential int64 [k]):
    acav_kmeanspp_seed.  u (float64 [1 + (k - 1) T], given explicitly) overrides the generator, whose next 2 (1 + (k - 1) T)
    draws are the uniforms otherwise.  Fewer than k distinct rows: ValueError."""
    from .lloyd import rows_absmax
    keep, xp, m, on_gpu = _as_f32_2d(x)
    d, k = int(keep.shape[1]), int(k)
    T = trials_for(k, trials)
    if not 1 <= k <= m:
        raise ValueError("{} seeds from a sample of {} rows".format(k, m))
    need = 1 + (k - 1) * T
    if u is None:
        from ..rng import default_generator
        u = uniforms(generator if generator is not None else default_generator, need)
    u = np.ascontiguousarray(u, np.float64)
    if u.shape != (need,):
        raise ValueError("u has shape {}, {} seeds with {} trials need {} values".format(u.shape, k, T, need))
    t = weight_shift(rows_absmax(keep), m, d)
    rows, potential = np.empty(k, np.int64), np.empty(k, np.int64)
    lib = _lib.load_library()
    _lib.check(lib.acav_kmeanspp_seed(keep.device.index if on_gpu else _device_index("cuda"), xp, m, d, k, T, _lib.ptr(u), t,
                                      _lib.ptr(rows), _lib.ptr(potential), stream))
    return rows, potential
