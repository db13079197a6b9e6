"""float64 numpy restatement of the clustering-quality definitions (acav_kmeans_quality / clustering/evaluate.py), the error
bounds the GPU tests hold the kernel to, and the seeded inputs those tests run on.

Definitions (exact arithmetic on the stored fp32 values, evaluated in float64 in the difference form):
    D_ik = sum_j (x_ij - c_kj)^2,  a2_i = D_{i,l_i},  b2_i = min_{k != l_i} D_ik (+inf when K = 1),
    displaced_i = (b2_i < a2_i),  s_i = (sqrt b2_i - sqrt a2_i) / max(sqrt a2_i, sqrt b2_i) (0 when both are 0 or K = 1)
    per cluster: count, sum a2, sum sqrt a2, sum s, sum displaced, sum min(a2, b2)

Bounds.  The kernel evaluates D = (||x||^2 + ||c||^2) - 2 x.c in float64 (u = 2^-53).  Whatever the summation order, each of
the three sums of d terms is within gamma_d of exact relative to its sum of magnitudes, and |2 x.c| <= ||x||^2 + ||c||^2, so
|D - D_exact| <= 2 gamma_{d+2} (||x||^2 + ||c||^2) ~= 2 (d + 2) 2^-53 (...).  tol_dist is 8 x that: (d + 2) 2^-50 (...).

Propagation (tol_sqrt, tol_s), v >= 0 computed with |v - v_ref| <= t:
    |sqrt v - sqrt v_ref| = |v - v_ref| / (sqrt v + sqrt v_ref) <= t / sqrt v_ref, and also <= sqrt |v - v_ref| <= sqrt t;
    the correctly rounded sqrt adds 2^-53 relative (2^-52 charged).
    s = f(p, q) = (q - p) / max(p, q) with p = sqrt a2, q = sqrt b2: both partial derivatives are bounded by 1 / max(p, q), and
    on the segment from the reference point to the computed one max(p, q) >= m_ref - max(dp, dq), hence
    |s - s_ref| <= (dp + dq) / (m_ref - max(dp, dq)) when that denominator is positive and 2 (|s| <= 1) otherwise; the
    subtraction and the division add 2^-53 each relative to |s| <= 1 (2^-51 charged).  K = 1: s = 0 on both sides, bound 0.
"""
import numpy as np

COLS = 6
COUNT, SUM_A2, SUM_SQRT_A2, SUM_S, DISPLACED, SUM_MIN = range(COLS)


def distances(x, c, chunk_bytes=1 << 28):
    """D [n, K] float64, difference form, in row chunks that keep the [rows, K, d] temporary under chunk_bytes"""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    n, d = x.shape
    K = c.shape[0]
    c8 = c.astype(np.float64)
    out = np.empty((n, K), np.float64)
    step = max(1, int(chunk_bytes // (8 * K * d)))
    for a in range(0, n, step):
        out[a:a + step] = ((x[a:a + step, None, :].astype(np.float64) - c8[None]) ** 2).sum(-1)
    return out


def row_reference(D, labels):
    """-> a2, b2, index of the centre attaining b2 (-1 when K = 1), displaced, s"""
    n, K = D.shape
    labels = np.asarray(labels, np.int64)
    idx = np.arange(n)
    a2 = D[idx, labels]
    masked = D.copy()
    masked[idx, labels] = np.inf
    kb = masked.argmin(1) if K > 1 else np.full(n, -1, np.int64)
    b2 = masked[idx, kb] if K > 1 else np.full(n, np.inf)
    p, q = np.sqrt(a2), np.sqrt(b2)
    m = np.maximum(p, q)
    with np.errstate(invalid='ignore', divide='ignore'):
        s = np.where((m > 0) & np.isfinite(q), (q - p) / m, 0.0)
    return a2, b2, kb, b2 < a2, s


def cluster_reference(a2, b2, displaced, s, labels, K):
    """[K, COLS] float64 per-cluster sums -- compose's input"""
    out = np.zeros((K, COLS), np.float64)
    labels = np.asarray(labels, np.int64)
    for col, val in ((COUNT, np.ones(len(labels))), (SUM_A2, a2), (SUM_SQRT_A2, np.sqrt(a2)), (SUM_S, s),
                     (DISPLACED, displaced.astype(np.float64)), (SUM_MIN, np.minimum(a2, b2))):
        out[:, col] = np.bincount(labels, weights=val, minlength=K)
    return out


def tol_dist(x, c, k):
    """per-row bound on |D_{i,k_i} - exact|: (d + 2) 2^-50 (||x_i||^2 + ||c_{k_i}||^2); k < 0 (no such centre) -> 0"""
    x8, c8 = np.asarray(x, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    d = x8.shape[1]
    k = np.asarray(k, np.int64)
    cn = np.where(k >= 0, (c8 ** 2).sum(1)[np.maximum(k, 0)], 0.0)
    return np.where(k >= 0, (d + 2) * 2.0 ** -50 * ((x8 ** 2).sum(1) + cn), 0.0)


def tol_sqrt(v_ref, t):
    r = np.sqrt(v_ref)
    with np.errstate(divide='ignore', invalid='ignore'):
        dv = np.where(r > 0, np.minimum(np.sqrt(t), t / r), np.sqrt(t))
    dv = np.where(np.isfinite(v_ref), dv, 0.0)  # b2 = +inf (K = 1) is +inf on both sides
    return dv + 2.0 ** -52 * np.where(np.isfinite(r), r + dv, 0.0)


def tol_s(a2_ref, b2_ref, ta, tb):
    dp, dq = tol_sqrt(a2_ref, ta), tol_sqrt(b2_ref, tb)
    m = np.maximum(np.sqrt(a2_ref), np.sqrt(b2_ref))
    room = m - np.maximum(dp, dq)
    with np.errstate(divide='ignore', invalid='ignore'):
        t = np.where(room > 0, np.minimum(2.0, (dp + dq) / room + 2.0 ** -51), 2.0)
    return np.where(np.isfinite(b2_ref), t, 0.0)


class Reference:
    """everything the GPU tests compare against, for rows x, centres c and labels (computed once per case)"""

    def __init__(self, x, c, labels):
        self.K = c.shape[0]
        self.labels = np.asarray(labels, np.int64)
        self.D = distances(x, c)
        self.a2, self.b2, self.kb, self.displaced, self.s = row_reference(self.D, self.labels)
        self.ta, self.tb = tol_dist(x, c, self.labels), tol_dist(x, c, self.kb)
        # rows whose displaced flag the bound cannot decide
        with np.errstate(invalid='ignore'):
            self.undecided = np.abs(self.a2 - self.b2) <= 2.0 * np.maximum(self.ta, self.tb)
        self.cluster = cluster_reference(self.a2, self.b2, self.displaced, self.s, self.labels, self.K)
        rows = {SUM_A2: self.ta, SUM_SQRT_A2: tol_sqrt(self.a2, self.ta), SUM_S: tol_s(self.a2, self.b2, self.ta, self.tb),
                SUM_MIN: np.maximum(self.ta, self.tb)}
        # float sums: the rows' bounds plus count 2^-52 |sum| for the additions
        self.cluster_tol = np.zeros((self.K, COLS), np.float64)
        for col, t in rows.items():
            self.cluster_tol[:, col] = (np.bincount(self.labels, weights=t, minlength=self.K) +
                                        self.cluster[:, COUNT] * 2.0 ** -52 * np.abs(self.cluster[:, col]))
        self.cluster_tol[:, DISPLACED] = np.bincount(self.labels, weights=self.undecided.astype(np.float64), minlength=self.K)


# ------------------------------------------------------------------------------------------------ seeded inputs
NOISE = np.array([1.0, 0.4])
SHAPES = [(1, 4, 2), (63, 7, 5), (65, 88, 33), (1000, 128, 64), (777, 1024, 257), (300, 2048, 1024), (129, 352, 1)]


def large_shapes(cus):
    """(n, d, K) at which every workgroup of k_quality takes several row tiles on a device of `cus` compute units (kind
    'discount').  The grid is min(tiles, cus * per_cu) with 64 rows per tile and per_cu = 4 workgroups per CU while their LDS
    allows, 1 at K = 2048; every n is 64 m + 1, so the last tile holds one row and is not its workgroup's first:
        small K, at least 2 tiles per workgroup | two centre passes (K > 64) and a column tail (d = 32 + 8) | the largest K:
        [K][6] sums carried over tiles, most clusters without a row"""
    return [(8 * cus * 64 + 65, 8, 5), (8 * cus * 64 + 65, 40, 70), (2 * cus * 64 + 65, 4, 2048)]


def make_case(n, d, K, kind='discount', seed=0):
    """-> x [n,d] fp32, centres [K,d] fp32, counts [K] fp32, count.  Even clusters are under-used in the state (counts below
    (count / K) ** 0.7, the library's discount divides their distances by 5), the rows are drawn around the odd ones with noise
    NOISE[row % 2]: the discount moves a row whenever an under-used centre is within sqrt 5 times its own distance -- the even
    rows (own distance^2 ~ d, another centre's ~ 3 d) move, the odd ones (~ 0.16 d against ~ 2.16 d) stay.
    kind: 'discount' | 'warm' (centres ~ 1e-5, data ~ 1: the state right after the warm-up) | 'scaled' (everything x 1e3) |
    'special' (K >= 9: centres 1 and 3 identical and far out with rows 1..5 around them, centre 5 far out without a row,
    row 0 identical to centre 7)"""
    rs = np.random.RandomState(1000 * seed + n + 7 * d + 13 * K)
    c = rs.randn(K, d).astype(np.float32)
    under = np.zeros(K, bool)
    if K > 1:
        under[::2] = True
    origin = np.flatnonzero(~under)
    if kind == 'special':
        origin = origin[origin > 5]
    src = origin[rs.randint(len(origin), size=n)]
    x = (c[src] + NOISE[np.arange(n) % 2, None] * rs.randn(n, d)).astype(np.float32)
    count, counts = 100 * K, np.where(under, 10.0, 190.0).astype(np.float32)  # threshold 100 ** 0.7 = 25.1
    if kind == 'warm':
        c = (rs.rand(K, d) * 1e-5).astype(np.float32)
        x = rs.randn(n, d).astype(np.float32)
        count, counts = 10 * K, np.where(under, 2.0, 18.0).astype(np.float32)  # threshold 10 ** 0.7 = 5.01
    elif kind == 'scaled':
        x, c = x * np.float32(1e3), c * np.float32(1e3)
    elif kind == 'special':
        c[1] += np.float32(10.0)
        c[3] = c[1]
        c[5] -= np.float32(10.0)
        x[1:6] = (c[1] + rs.randn(5, d)).astype(np.float32)
        x[0] = c[7]
    elif kind != 'discount':
        raise ValueError(kind)
    return x, c, counts, count


def discount_labels(x, c, counts, count, p=0.7, r=5.0):
    """what calc_best does, in float64 (first index on ties): for choosing and checking the seeded inputs without a GPU --
    the GPU tests take their labels from calc_best itself"""
    D = distances(x, c)
    under = np.asarray(counts, np.float32) < np.float32((count / c.shape[0]) ** p)
    return np.where(under[None], D / r, D).argmin(1)
