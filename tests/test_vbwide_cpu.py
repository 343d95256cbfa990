"""The algorithm of the wide variational mixture fit (csrc/vbgmm.hip, vbwide_*), restated in float64 numpy (tests/vbwide_ref.py), against
sklearn.mixture.BayesianGaussianMixture on every parity case -- no GPU.  What the kernels add to this is summation order alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vbwide_ref as V  # noqa: E402


@pytest.mark.parametrize("i", range(len(V.CASES)), ids=V.IDS)
def test_restatement_matches_sklearn(i):
    """Cold fit on X1 from sklearn's k-means labels, warm refit on X2: the iteration counts of the table (each decidable on sklearn's own lower
    bounds: V.reference asserts it), converged_, and lower bound / weights / means / covariances within the project's bars."""
    kw = V.kwargs(i)
    mine = V.NumpyVB(**kw)
    for f, (X, snap) in enumerate(zip(V.samples(i), V.reference(i))):
        mine.fit(X, labels=V.kmeans_labels(X, kw["n_components"]) if f == 0 else None)
        assert (mine.n_iter_, mine.converged_) == (snap["n_iter_"], snap["converged_"]) and snap["n_iter_"] == V.CASES[i][-1][f]
        V.assert_close(mine, V.Snap(snap))


def test_shifted_prior_moments_equal_numpy_cov():
    """covariance_prior_ from the second moments about the fp32-rounded mean is np.cov to round-off, also far from the origin."""
    X = (V.samples(6)[0] + 1000.0).astype(np.float32)
    vb = V.NumpyVB(2, max_iter=0).fit(X, labels=np.zeros(len(X), dtype=int) + np.arange(len(X)) % 2)
    np.testing.assert_allclose(vb.cov_prior, np.cov(X.astype(np.float64).T), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(vb.mean_prior, X.astype(np.float64).mean(0), rtol=1e-15)
