"""CPU: the float64 restatement of clustering.pca (tests/_pca_np.py) against sklearn.decomposition.PCA(svd_solver='full') on a
float64 copy of the recipe.  Both sides are references: their disagreement on the well-separated leading components was
measured (eigh of the covariance against the SVD of the centred rows, sklearn 1.7.2) and 16 x that is asserted:

    shape        max |components - sklearn|   max rel |explained_variance - sklearn|   max |fit_transform - sklearn| / max |y|
    1000 x 88    2.64e-15                     2.04e-15                                 2.68e-15
    257 x 88     3.22e-15                     1.94e-15                                 1.00e-15
    4000 x 40    5.94e-15                     2.55e-15                                 3.32e-15
"""
import numpy as np
import pytest

from tests import _pca_np as R

MEASURED = {"components": 5.94e-15, "explained_variance": 2.55e-15, "fit_transform": 3.32e-15}
LEAD = 8  # the planted variances halve from one direction to the next: these components are well determined


@pytest.mark.parametrize("n,d,seed", [(1000, 88, 3), (257, 88, 4), (4000, 40, 5)])
def test_restatement_against_sklearn(n, d, seed):
    decomposition = pytest.importorskip("sklearn.decomposition")
    x = R.recipe(n, d, seed)
    x64 = x.astype(np.float64)
    p = 16
    f = R.fit(x, p)
    sk = decomposition.PCA(n_components=p, svd_solver="full")
    y_sk = sk.fit_transform(x64)
    w = f["explained_variance"]
    assert (w[:LEAD - 1] > 1.5 * w[1:LEAD]).all()  # the gaps the recipe promises
    dc = np.abs(f["components64"][:LEAD] - sk.components_[:LEAD]).max()  # signs included
    de = (np.abs(w[:LEAD] - sk.explained_variance_[:LEAD]) / sk.explained_variance_[:LEAD]).max()
    y = (x64 - f["mean64"]) @ f["components64"][:LEAD].T
    dy = np.abs(y - y_sk[:, :LEAD]).max() / np.abs(y_sk[:, :LEAD]).max()
    print("n {} d {}: components {:.3g} explained_variance {:.3g} fit_transform {:.3g}".format(n, d, dc, de, dy))
    assert dc <= 16 * MEASURED["components"]
    assert de <= 16 * MEASURED["explained_variance"]
    assert dy <= 16 * MEASURED["fit_transform"]
    assert np.abs(f["mean64"] - sk.mean_).max() <= 1e-12 * np.abs(sk.mean_).max()
    tv = x64.var(0, ddof=1).sum()
    assert abs(f["total_variance"] - tv) <= 1e-12 * tv
    assert f["mean"].dtype == np.float32 and f["components"].dtype == np.float32 and f["components"].shape == (p, d)
    assert (np.diff(w) <= 0).all() and w.shape == (p,)


def test_sign_rule():
    v = np.array([[0.1, -0.9, 0.3],      # the largest entry is negative: the row is flipped
                  [0.5, -0.5, 0.1],      # a tie: the FIRST entry of largest magnitude decides -- no flip
                  [-0.5, 0.5, 0.1],      # the same tie the other way round: flipped
                  [0.0, 0.2, -0.1]])
    got = R.flip(v)
    assert np.array_equal(got, np.array([[-0.1, 0.9, -0.3], [0.5, -0.5, 0.1], [0.5, -0.5, -0.1], [0.0, 0.2, -0.1]]))
    f = R.fit(R.recipe(300, 20, 1), 6)
    top = np.argmax(np.abs(f["components64"]), axis=1)
    assert (f["components64"][np.arange(6), top] > 0).all()


def test_too_few_rows_are_refused():
    x = R.recipe(16, 40, 2)
    for p in (16, 17, 40):
        with pytest.raises(ValueError, match="N <= p"):
            R.fit(x, p)
    assert R.fit(x, 15)["components"].shape == (15, 40)
