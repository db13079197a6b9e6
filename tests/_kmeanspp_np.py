"""numpy restatement of the k-means++ seeding as the clustering stage defines it (acav100m_amd/clustering/kmeanspp.py), written
from the definition and sharing no code with the package:

  weight    W(i, c) = int64(rint(D * 2^t)), D = sum_j p_j, p_j = e_j * e_j, e_j = float64(x_ij) - float64(x_cj): numpy float64
            operations, each rounded once (numpy has no fma).  THE ORDER OF THE SUM, a function of d alone: lane l = (j // 4) % 64
            owns column j and chains the p_j of its columns from +0.0 in ascending j; the 64 lane values are summed by an
            xor-butterfly, v[l] <- v[l] + v[l ^ o] for o = 32, 16, 8, 4, 2, 1 (every lane ends with the same bits; lane 0 is
            read).  Columns past d are zero on both sides: they add +0.0 and change no bit.
  shift     t = 59 - bl(m) - bl(d) - 2 E, bl(n) = bit_length(max(n, 2) - 1), (_, E) = frexp(absmax of the sample)
  uniforms  ((a >> 5) * 2^26 + (b >> 6)) / 2^53 from two successive 32-bit draws a, b
  picks     pick 0: r = min(m - 1, int(u[0] * m)), w = W(., r).  Pick s >= 1: total = sum w (0: ValueError); per trial tau < T
            target = min(total - 1, int(u[1 + (s - 1) T + tau] * float(total))), r_tau = the least i with w_0 + ... + w_i >
            target, pot_tau = sum min(w, W(., r_tau)); the least pot wins, the lowest tau on ties."""
import math

import numpy as np

LANES = 64
BLOCK = 1024  # rows of a block of the library's block sums (the sizes around it are the tests' edge cases)


def bl(n):
    return (max(int(n), 2) - 1).bit_length()


def shift_of(absmax, m, d):
    _m, e = math.frexp(float(absmax))
    return 59 - bl(m) - bl(d) - 2 * e


def sq_dist(x, c):
    """D of every row of x [m, d] against the row c [d] -> float64 [m], in the stated order"""
    x = np.asarray(x, np.float32)
    m, d = x.shape
    dpad = -(-d // (4 * LANES)) * 4 * LANES
    e = np.zeros((m, dpad), np.float64)
    e[:, :d] = x.astype(np.float64) - np.asarray(c, np.float32).astype(np.float64)[None, :]
    p = (e * e).reshape(m, dpad // (4 * LANES), LANES, 4)  # [row, group of the lane, lane, column of the group]
    lanes = np.zeros((m, LANES), np.float64)
    for g in range(p.shape[1]):
        for q in range(4):
            lanes = lanes + p[:, g, :, q]
    idx = np.arange(LANES)
    o = LANES // 2
    while o:
        lanes = lanes + lanes[:, idx ^ o]
        o //= 2
    return lanes[:, 0].copy()


def weights(x, cand_rows, t):
    """-> int64 [T, m]"""
    x = np.asarray(x, np.float32)
    return np.stack([np.rint(sq_dist(x, x[int(c)]) * 2.0 ** t).astype(np.int64) for c in cand_rows])


def uniforms(draw_u32, count):
    out = np.empty(count, np.float64)
    for i in range(count):
        a, b = int(draw_u32()), int(draw_u32())
        out[i] = ((a >> 5) * 2 ** 26 + (b >> 6)) / 2.0 ** 53
    return out


def trials_for(k, trials):
    return min(16, 2 + int(math.floor(math.log(k)))) if trials == 'auto' else int(trials)


def draw(w, target):
    """the least i with w_0 + ... + w_i > target"""
    run = 0
    for i, wi in enumerate(w.tolist()):
        run += wi
        if run > target:
            return i
    raise AssertionError("target beyond the total")


def seed(x, k, T, u, t=None):
    """-> (rows int64 [k], potential int64 [k]); ValueError when the sample holds fewer than k distinct rows"""
    x = np.asarray(x, np.float32)
    m, d = x.shape
    u = np.asarray(u, np.float64)
    assert u.shape == (1 + (k - 1) * T,)
    if t is None:
        t = shift_of(np.abs(x).max(), m, d)
    rows, potential = np.empty(k, np.int64), np.empty(k, np.int64)
    rows[0] = min(m - 1, int(u[0] * m))
    w = weights(x, [rows[0]], t)[0]
    potential[0] = int(w.sum())
    for s in range(1, k):
        total = int(w.sum())
        if total == 0:
            raise ValueError("only {} distinct rows".format(s))
        best = None
        for tau in range(T):
            target = min(total - 1, int(float(u[1 + (s - 1) * T + tau]) * float(total)))
            r = draw(w, target)
            cand = np.minimum(w, weights(x, [r], t)[0])
            pot = int(cand.sum())
            if best is None or pot < best[0]:
                best = (pot, r, cand)
        potential[s], rows[s], w = best
    return rows, potential
