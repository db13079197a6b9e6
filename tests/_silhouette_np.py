"""float64 restatement of the exact silhouette (acav100m_amd.clustering.silhouette, acav_rows_silhouette) in DIFFERENCE form,
dist(i, j) = sqrt(sum_c (x_ic - x_jc)^2): no cancellation, so it is the reference the kernel's expanded form is bounded against.

Bounds (include/acav_hip.h), with u = 2^-53, gamma_n = n u / (1 - n u), N_i = ||x_i||^2:
  pair    Delta_ij = 2 gamma_{d+2} (N_i + N_j) bounds the kernel's squared distance, hence its distance is within
          e_ij = min(sqrt(Delta_ij), Delta_ij / dist_ij) (1 + 2^-52) of the exact one; the restatement's own distance (d squares,
          d - 1 adds, a square root) is within gamma_{d+2} dist_ij, which is added to e_ij.  Duplicates (dist = 0): sqrt(Delta_ij).
  mean    over n terms: (sum_j e_ij) / n from the terms, plus gamma_{n+1} relative of the computed mean (the chain and the division).
  A_i     the mean over the row's own cluster without itself (n = n_l - 1); exactly 0 when n_l = 1.
  B_i     the minimum of the other clusters' means m_k with tolerances t_k: the computed minimum is at most m_k* + t_k* (k* the exact
          argmin) and at least min_k (m_k - t_k).
  s_i     (B - A) / max(A, B) rises with B and falls with A: it lies between s(A + tA, B - tB) and s(A - tA, B + tB), plus 2^-51 for
          the two roundings of the quotient; exactly 0 for the only row of its cluster.
"""
import numpy as np

U = 2.0 ** -53


def gamma(n):
    return n * U / (1.0 - n * U)


def s_of(A, B, single):
    """(B - A) / max(A, B); 0 where both are 0 and for the only row of its cluster"""
    A, B = np.maximum(A, 0.0), np.maximum(B, 0.0)
    top = np.maximum(A, B)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(np.isinf(top), np.where(np.isinf(B), 1.0, -1.0), (B - A) / top)
    s = np.where((top == 0) | single, 0.0, s)
    return s


class Reference:
    """A, B, s and their tolerances tA, tB, ts for the query rows `rows` (default: all) of x [M, d] fp32 with labels in [0, k)"""

    def __init__(self, x, labels, k, rows=None):
        x = np.ascontiguousarray(x, np.float32)
        x64 = x.astype(np.float64)
        lab = np.asarray(labels, np.int64)
        M, d = x.shape
        q = np.arange(M) if rows is None else np.asarray(rows, np.int64)
        self.rows, self.labels, self.k = q, lab, int(k)
        nrm = (x64 * x64).sum(1)
        D = np.empty((len(q), M))
        for a, i in enumerate(q):
            diff = x64 - x64[i]
            D[a] = np.sqrt((diff * diff).sum(1))
        delta = 2.0 * gamma(d + 2) * (nrm[q][:, None] + nrm[None, :])
        with np.errstate(divide="ignore", invalid="ignore"):
            E = np.minimum(np.sqrt(delta), np.where(D > 0, delta / D, np.inf)) * (1.0 + 2.0 ** -52) + gamma(d + 2) * D
        D[np.arange(len(q)), q] = 0.0  # j == i takes no part
        E[np.arange(len(q)), q] = 0.0
        self.dist = D
        sizes = np.bincount(lab, minlength=self.k)
        onehot = np.zeros((M, self.k))
        onehot[np.arange(M), lab] = 1.0
        own = lab[q]
        den = np.tile(sizes.astype(np.float64), (len(q), 1))
        den[np.arange(len(q)), own] -= 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = (D @ onehot) / den
            term = (E @ onehot) / den
            tol = term + gamma(np.maximum(den, 0) + 1) * (mean + term) + M * U * mean  # (+ the restatement's own matrix product)
        single = sizes[own] == 1
        ar = np.arange(len(q))
        self.A = np.where(single, 0.0, mean[ar, own])
        self.tA = np.where(single, 0.0, tol[ar, own])
        other = np.tile(sizes > 0, (len(q), 1))
        other[ar, own] = False
        m_o = np.where(other, mean, np.inf)
        t_o = np.where(other, tol, 0.0)
        star = np.argmin(m_o, axis=1)
        self.B = m_o[ar, star]
        low = np.where(other, mean - tol, np.inf).min(1)
        with np.errstate(invalid="ignore"):
            self.tB = np.where(np.isinf(self.B), 0.0, np.maximum(t_o[ar, star], self.B - low))
        self.single, self.sizes = single, sizes
        self.s = s_of(self.A, self.B, single)
        hi = s_of(self.A - self.tA, self.B + self.tB, single)
        lo = s_of(self.A + self.tA, self.B - self.tB, single)
        self.ts = np.where(single, 0.0, np.maximum(hi - self.s, self.s - lo) + 2.0 ** -51)

    def check(self, A, B, s=None, what=""):
        """the figures against the restatement within the bounds (prints the largest deviation and its bound first)"""
        pairs = [("A", A, self.A, self.tA), ("B", B, self.B, self.tB)] + ([("s", s, self.s, self.ts)] if s is not None else [])
        for name, got, want, tol in pairs:
            got = np.asarray(got, np.float64)
            both_inf = np.isinf(got) & np.isinf(want) & (got == want)
            with np.errstate(invalid="ignore"):
                dev = np.where(both_inf, 0.0, np.abs(got - want))
            worst = int(np.argmax(dev - tol))
            print("{} {}: max |dev| {:.3g}, at row {} dev {:.3g} against {:.3g}".format(what, name, dev.max(), worst, dev[worst], tol[worst]))
            assert (dev <= tol).all(), (what, name, worst, got[worst], want[worst], tol[worst])


def mixture(sizes, d, seed, spread=0.6, labels_of=None):
    """rows of a Gaussian mixture, cluster c in sizes[c] rows (0: a label value without a member), shuffled -> (x fp32 [M, d],
    labels int64 [M]); labels_of: the label value of each entry of sizes (default: its index)"""
    rs = np.random.RandomState(seed)
    sizes = np.asarray(sizes, np.int64)
    values = np.arange(len(sizes)) if labels_of is None else np.asarray(labels_of, np.int64)
    lab = np.repeat(values, sizes)
    centres = rs.randn(len(sizes), d)
    x = centres[np.repeat(np.arange(len(sizes)), sizes)] + spread * rs.randn(len(lab), d)
    order = rs.permutation(len(lab))
    return x[order].astype(np.float32), lab[order]


def random_labels(m, d, k, seed):
    """m rows with labels drawn uniformly from [0, k): singletons and absent values as they fall"""
    rs = np.random.RandomState(seed)
    lab = rs.randint(0, k, m).astype(np.int64)
    x = (rs.randn(k, d)[lab] + 0.6 * rs.randn(m, d)).astype(np.float32)
    return x, lab


def duplicates(seed):
    """96 x 64, 3 clusters: row a of cluster 0 equals row b of cluster 1, and rows c, e of cluster 2 are equal -> (x, labels, pairs)"""
    x, lab = mixture([32, 32, 32], 64, seed)
    a, b = np.flatnonzero(lab == 0)[3], np.flatnonzero(lab == 1)[7]
    c, e = np.flatnonzero(lab == 2)[[1, 20]]
    x[b] = x[a]
    x[e] = x[c]
    return x, lab, ((int(a), int(b)), (int(c), int(e)))


def cases(block=64):
    """name -> (x, labels, k) of the seeded GPU-test inputs; block: the column block of the plan (runs that end on a block
    boundary and one row past it)"""
    out = {}
    out["tails_65x88_k33"] = random_labels(65, 88, 33, 1) + (33,)                   # one past a tile and a block, d % 32 != 0
    out["tails_65x87_k33"] = random_labels(65, 87, 33, 2) + (33,)                   # d % 4 != 0: the guarded loads
    out["two_599_1"] = mixture([599, 1], 128, 3) + (2,)                             # a run over ten blocks, a singleton
    out["absent_values"] = mixture([40, 1, 50, 39], 40, 4, labels_of=[1, 3, 6, 7]) + (9,)  # values 0, 2, 4, 5, 8 have no member
    out["block_ends"] = mixture([block, block + 1, block - 1, block], 32, 5) + (4,)  # runs end on 64 | 129 | 192 | 256
    out["wide_1024"] = mixture([60, 97, 100], 1024, 6) + (3,)
    out["wide_2304"] = mixture([60, 97, 100], 2304, 7) + (3,)
    x, lab, _pairs = duplicates(8)
    out["duplicates"] = (x, lab, 3)
    return out
