"""Float64 restatement of clustering.pca (acav100m_amd/clustering/pca.py) for the tests: the definition, the shifted sums the
device accumulates, and the seeded test data."""
import numpy as np

SLICE = 1024  # ACAV_SCATTER_SLICE (include/acav_hip.h)


def flip(v):
    """sklearn's svd_flip(u_based_decision=False) on the rows of v: the entry of largest magnitude (the first on a tie) positive"""
    v = np.array(v, np.float64)
    top = np.argmax(np.abs(v), axis=1)
    return v * np.sign(v[np.arange(v.shape[0]), top])[:, None]


def fit(x, p):
    """the Definition -> dict: mean64 / components64 (before the rounding), mean / components (fp32), explained_variance,
    total_variance, spectrum (every eigenvalue, descending), S (the scatter matrix)"""
    x = np.asarray(x, np.float32).astype(np.float64)
    n, d = x.shape
    if n <= p:
        raise ValueError("{} rows cannot carry {} principal components (N <= p)".format(n, p))
    mean = x.mean(0)
    c = x - mean
    S = c.T @ c
    cov = S / np.float64(n - 1)
    w, v = np.linalg.eigh(cov)
    w, v = w[::-1], v[:, ::-1].T
    comps = flip(v[:p])
    return {'mean64': mean, 'components64': comps, 'mean': mean.astype(np.float32), 'components': comps.astype(np.float32),
            'explained_variance': w[:p].copy(), 'total_variance': np.float64(np.trace(cov)), 'spectrum': w, 'S': S}


def project64(x, mean32, comp32):
    """sum_j (x_ij - mean32_j) comp32_kj in float64 -> (y, sum_j |x_ij - mean32_j| |comp32_kj|)"""
    c = np.asarray(x, np.float32).astype(np.float64) - np.asarray(mean32, np.float32).astype(np.float64)
    k = np.asarray(comp32, np.float32).astype(np.float64)
    return c @ k.T, np.abs(c) @ np.abs(k).T


def shifted_sums(x, shift):
    """E = x - shift in float64 (exact) -> (sum_rows E, E^T E, |E|^T |E|, sum_rows |E|)"""
    e = np.asarray(x, np.float32).astype(np.float64) - np.asarray(shift, np.float32).astype(np.float64)
    a = np.abs(e)
    return e.sum(0), e.T @ e, a.T @ a, a.sum(0)


def recipe(n, d, seed):
    """the test data, fp32 [n, d]: up to 12 planted directions (a random orthonormal frame) with variances 64, 32, 16, ... --
    clear gaps between the leading eigenvalues -- over isotropic noise of std 0.01 and per-column offsets in [-5, 5]; then
    column 0 constant 0.1f and column 2 = 1e4 + 1e-2 randn (where d allows): the column that a raw sum x x^T would ruin"""
    rs = np.random.RandomState(seed)
    r = max(1, min(12, d - 2))
    q, _ = np.linalg.qr(rs.randn(d, r))
    lam = 64.0 * 0.5 ** np.arange(r)
    x = (rs.randn(n, r) * np.sqrt(lam)) @ q.T + 0.01 * rs.randn(n, d) + rs.uniform(-5, 5, d)
    x = x.astype(np.float32)
    x[:, 0] = np.float32(0.1)
    if d > 2:
        x[:, 2] = (1e4 + 1e-2 * rs.randn(n)).astype(np.float32)
    return x
