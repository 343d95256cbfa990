"""Shared by tests/test_emgmm_wide_cpu.py and tests/test_gpu_emgmm_wide.py: the parity cases of the EM fit on 80 .. 256 dimensions
(csrc/emgmm_wide.hip).  The mixtures, sklearn's arguments, the bars, the numpy restatement of the algorithm and the decidability precondition are
those of the narrow fit (tests/emgmm_ref.py): the wide kernels differ from the narrow ones in how the sums are cut, not in what they compute."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from emgmm_ref import BAR_LB, BARS, KW, NumpyEM, assert_close, assert_iteration_count_is_decidable, data, sklearn_fit  # noqa: E402,F401

# N, R, K, max_iter, centres, spread, seed, sklearn n_iter (cold, warm; None = cold fit only)
CASES = [
    (1100, 80, 3, 200, 4, 0.06, 1, (19, 24)),      # the narrowest width; overlapping components: 40 % of the rows have a responsibility strictly
                                                   # inside (1e-6, 1 - 1e-6) -- the case that exercises the soft E-step
    (1500, 144, 3, 200, 3, 0.05, 3, (4, 25)),      # nine column blocks: a statistics wavefront owns one to three of them, 12 row splits
    (2051, 256, 2, 200, 3, 0.04, 5, (2, 35)),      # R at the limit, ragged last slice (3 samples), 17 row splits
    (1027, 96, 2, 200, 3, 0.25, 1, (4, 3)),        # ragged slice and ragged split, well separated
    (300, 96, 4, 200, 4, 0.25, 1, (2, 3)),         # 75 samples per component in 96 dimensions: rank-deficient covariances that only reg_covar makes
                                                   # factor, |precisions_cholesky_| up to 6e2 -- the regime of the production fast fit
    (1100, 80, 3, 3, 4, 0.06, 1, (3, None)),       # the first case stopped at max_iter: not converged, one ConvergenceWarning
]
IDS = ["%dx%dx%d-%d" % c[:4] for c in CASES]
ATTRS = ("weights_", "means_", "covariances_", "precisions_cholesky_")


@functools.lru_cache(maxsize=None)
def reference(i):
    """sklearn's cold fit (+ warm refit) of case i, computed once per process and shared: per fit a dict of n_iter_, converged_, lower_bound_, the
    parameters and the number of ConvergenceWarnings.  Each fit first passes the precondition that round-off cannot decide its iteration count,
    and gives the iteration count written beside the case."""
    from sklearn.mixture import GaussianMixture
    N, R, K, max_iter, centres, spread, seed, n_iters = CASES[i]
    ref = GaussianMixture(n_components=K, max_iter=max_iter, **KW)
    out = []
    for X, n_iter in zip(data(N, R, centres, spread, seed), n_iters):
        if n_iter is None:
            break
        warned = sklearn_fit(ref, X)
        assert_iteration_count_is_decidable(ref, KW["tol"], max_iter)
        assert ref.n_iter_ == n_iter, (ref.n_iter_, n_iter)
        snap = dict(n_iter_=ref.n_iter_, converged_=ref.converged_, lower_bound_=ref.lower_bound_, warned=len(warned))
        snap.update({a: getattr(ref, a).copy() for a in ATTRS})
        out.append(snap)
    return out


class WideNumpyEM(NumpyEM):
    """NumpyEM with its two slow steps restated for these widths -- the same sums, cut differently (like the kernels): the second moments as one
    matrix product per component instead of an einsum over [N, K, R, R], the triangular inverse a row at a time instead of an element at a time
    (row i of L^-1 from rows 0 .. i-1: X[i, :i] = -L[i, :i] X[:i, :i] / L[i, i], the terms with X[p, c] = 0 for p < c included)."""

    def _stats(self, X, resp):
        xt = X - self.c
        return resp.sum(0), resp.T @ xt, np.stack([(resp[:, k, None] * xt).T @ xt for k in range(self.K)])

    @staticmethod
    def _tri_inv(Lk):
        X = np.zeros_like(Lk)
        for i in range(Lk.shape[0]):
            X[i, :i] = -(Lk[i, :i] @ X[:i, :i]) / Lk[i, i]
            X[i, i] = 1.0 / Lk[i, i]
        return X


def bar_ratio(a, b, bar):
    """max |a - b| / (atol + rtol |b|): <= 1 is np.testing.assert_allclose(a, b, rtol, atol) holding."""
    rtol, atol = bar
    return float((np.abs(a - b) / (atol + rtol * np.abs(b))).max())


# The rank-deficient case.  Its covariances have condition number ~ 1e6 (75 samples in 96 dimensions, held up by reg_covar = 1e-6), so
# precisions_cholesky_ = L^-T carries ~ 1e6 eps |P| ~ 1e-7 of round-off whatever the order of the sums -- against entries of 1e-3 beside entries of
# 9e2 the elementwise bar (1e-6 relative, 1e-9 absolute) is not one that float64 arithmetic in another order can be held to.  MEASURED on the host
# (tests/test_emgmm_wide_cpu.py prints it): bar_ratio of NumpyEM's precisions_cholesky_ against sklearn's is 0.57 on the cold fit -- inside BARS --
# and 14.33 on the warm refit (max |diff| 1.5e-7 at max |P| = 876; covariances agree to 1e-15); WideNumpyEM, another order of the same sums, gives
# 0.68 and 9.70.  The bar of that one array on that one fit is therefore NumpyEM's own measured error there, times ten for sums cut differently again
# (the kernels; WideNumpyEM).  Everything else of the case, and its cold fit, stays at BARS.  MEASURED on the MI355X: the kernels'
# precisions_cholesky_ is at 0.48 of BARS on the cold fit and at 0.16 of the widened bar (23 times BARS) on the warm refit.
RANK_DEFICIENT = 4
NUMPY_PCHOL_RATIO = (0.57, 14.33)       # NumpyEM's error over the bar of precisions_cholesky_, cold fit / warm refit, as measured on the host
OTHER_ORDER = 10.0                      # room for another order of the same float64 sums


def kmeans_labels(X1, K):
    from sklearn.cluster import KMeans
    from sklearn.utils import check_random_state
    return KMeans(n_clusters=K, n_init=1, random_state=check_random_state(KW["random_state"])).fit(X1.astype(np.float64)).labels_


def numpy_pchol_ratio():
    """(cold, warm): bar_ratio of NumpyEM's precisions_cholesky_ against sklearn's on the rank-deficient case, measured here and now; everything else
    of the case is asserted to hold BARS.  NUMPY_PCHOL_RATIO records what this returned when the bar was derived (sklearn 1.7.2)."""
    N, R, K, max_iter, centres, spread, seed, _ = CASES[RANK_DEFICIENT]
    X1, X2 = data(N, R, centres, spread, seed)
    mine = NumpyEM(K, tol=KW["tol"], reg_covar=KW["reg_covar"], max_iter=max_iter)
    out = []
    for X, lab, snap in zip((X1, X2), (kmeans_labels(X1, K), None), reference(RANK_DEFICIENT)):
        mine.fit(X, lab)
        assert (mine.n_iter_, mine.converged_) == (snap["n_iter_"], snap["converged_"])
        for name in ("weights_", "means_", "covariances_"):
            assert bar_ratio(getattr(mine, name), snap[name], BARS[name]) <= 1.0, name
        out.append(bar_ratio(mine.precisions_cholesky_, snap["precisions_cholesky_"], BARS["precisions_cholesky_"]))
    return tuple(out)


def bars_for(i, f):
    """BARS for fit f (0 cold, 1 warm) of case i.  Where NumpyEM itself misses the bar of precisions_cholesky_ on the rank-deficient case (its warm
    refit), that bar is NumpyEM's measured error times OTHER_ORDER: (1.433e-4 relative, 1.433e-7 absolute)."""
    bars = dict(BARS)
    if i == RANK_DEFICIENT and NUMPY_PCHOL_RATIO[f] > 1.0:
        bars["precisions_cholesky_"] = tuple(NUMPY_PCHOL_RATIO[f] * OTHER_ORDER * b for b in BARS["precisions_cholesky_"])
    return bars


def assert_close_case(i, f, dev, ref):
    """emgmm_ref.assert_close with the bars of (case, fit); prints every figure before it asserts."""
    lb = abs(dev.lower_bound_ - ref.lower_bound_) / abs(ref.lower_bound_)
    bars = bars_for(i, f)
    ratios = {name: bar_ratio(getattr(dev, name), getattr(ref, name), bars[name]) for name in ATTRS}
    print("%s fit %d: lower bound rel %.3e (bar %.0e); error / bar: %s" % (IDS[i], f, lb, BAR_LB, ", ".join("%s %.3g" % kv for kv in ratios.items())))
    assert lb <= BAR_LB, (dev.lower_bound_, ref.lower_bound_)
    for name in ATTRS:
        np.testing.assert_allclose(getattr(dev, name), getattr(ref, name), rtol=bars[name][0], atol=bars[name][1], err_msg=name)


class Snap:
    def __init__(self, d):
        self.__dict__.update(d)
