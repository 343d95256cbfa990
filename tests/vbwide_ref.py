"""Shared by tests/test_vbwide_cpu.py and tests/test_gpu_vbgmm_wide.py: the parity cases of the wide variational mixture fit (8 < R <= 64), sklearn's
own fits of them (computed once per process), and a float64 numpy restatement of the ALGORITHM of the vbwide_* kernels of csrc/vbgmm.hip: one shift
vector, shifted raw moments centred in the M-step, the data-derived priors from moments about the same shift, Cholesky + triangular inverse, sklearn's
lower bound and loop.  The restatement and the kernels differ in summation order only; it pins the algorithm against sklearn on machines without a GPU
and is what a tolerance wider than the project's bars would have to be derived from."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emgmm_ref as E  # noqa: E402

DIST, PROC = "dirichlet_distribution", "dirichlet_process"

# N, R, K, prior type, max_iter, tol, centres, spread, seed (tests/emgmm_ref.data), sklearn 1.7 n_iter (cold, warm)
CASES = [
    (2051, 16, 30, DIST, 300, 1e-3, 7, 0.5, 1, (124, 12)),       # exact tile, ragged N, an R the engine takes
    (2048, 12, 50, PROC, 30, 1e-3, 9, 0.6, 5, (30, 30)),         # R inside one tile, long stick, stops at the cap
    (1100, 33, 6, PROC, 200, 1e-3, 8, 0.35, 12, (28, 17)),       # R just past a tile multiple
    (1300, 64, 3, DIST, 200, 1e-3, 5, 0.25, 8, (7, 3)),          # R at the limit
    (1000, 64, 64, PROC, 5, 0.0, 30, 0.3, 2, (5, 5)),            # full K x R width
    (600, 9, 1, PROC, 5, 0.0, 3, 1.0, 9, (5, 5)),                # first wide R, K = 1 (empty stick prefix and tail)
    (257, 17, 2, DIST, 5, 0.0, 3, 0.5, 3, (5, 5)),               # four full slices and a one-sample slice
    (5003, 24, 8, PROC, 60, 1e-3, 5, 0.5, 6, (41, 3)),           # many slices, several row splits
]
IDS = ["%dx%dx%d" % c[:3] for c in CASES]
RANDOM_STATE = 7
ATTRS = ("weights_", "means_", "covariances_")

# the project's bars for fits that centre raw moments (tests/emgmm_ref.py, test_vbgmm_sharded_statistics_fit_matches_sklearn_one_rank)
BAR_LB = E.BAR_LB
BARS = {a: E.BARS[a] for a in ATTRS}


def kwargs(i):
    """The constructor arguments of case i, for sklearn's class and the device class alike."""
    N, R, K, ptype, max_iter, tol, *_ = CASES[i]
    return dict(n_components=K, covariance_type="full", tol=tol, reg_covar=1e-6, max_iter=max_iter, n_init=1, weight_concentration_prior_type=ptype,
                weight_concentration_prior=0.1, warm_start=True, random_state=RANDOM_STATE)


def samples(i):
    N, R, _K, _p, _m, _t, centres, spread, seed, _n = CASES[i]
    return E.data(N, R, centres, spread, seed)


@functools.lru_cache(maxsize=None)
def reference(i):
    """sklearn's cold fit and warm refit of case i, computed once: per fit a dict of n_iter_, converged_, lower_bound_, the parameters and the number
    of ConvergenceWarnings.  Each fit first passes the precondition that round-off cannot decide its iteration count, and has the table's count."""
    from sklearn.mixture import BayesianGaussianMixture
    kw, n_iters = kwargs(i), CASES[i][-1]
    ref = BayesianGaussianMixture(**kw)
    out = []
    for X, n_iter in zip(samples(i), n_iters):
        warned = E.sklearn_fit(ref, X)
        E.assert_iteration_count_is_decidable(ref, kw["tol"], kw["max_iter"])
        assert ref.n_iter_ == n_iter, (ref.n_iter_, n_iter)
        snap = dict(n_iter_=ref.n_iter_, converged_=ref.converged_, lower_bound_=ref.lower_bound_, warned=len(warned))
        snap.update({a: getattr(ref, a).copy() for a in ATTRS})
        out.append(snap)
    return out


class Snap:
    def __init__(self, d):
        self.__dict__.update(d)


def assert_close(dev, ref):
    assert abs(dev.lower_bound_ - ref.lower_bound_) <= BAR_LB * abs(ref.lower_bound_), (dev.lower_bound_, ref.lower_bound_)
    for name, (rtol, atol) in BARS.items():
        np.testing.assert_allclose(getattr(dev, name), getattr(ref, name), rtol=rtol, atol=atol, err_msg=name)


def kmeans_labels(X32, K):
    """The labels BaseMixture._initialize_parameters gives a cold fit with random_state = RANDOM_STATE."""
    from sklearn.cluster import KMeans
    from sklearn.utils import check_random_state
    return KMeans(n_clusters=K, n_init=1, random_state=check_random_state(RANDOM_STATE)).fit(X32.astype(np.float64)).labels_


class NumpyVB:
    """The device algorithm in float64 numpy.  fit(X, labels=None): labels = the hard assignment of a cold start, None = warm start."""

    def __init__(self, n_components, weight_concentration_prior_type=PROC, weight_concentration_prior=None, mean_precision_prior=None, tol=1e-3,
                 reg_covar=1e-6, max_iter=100, **_unused):
        self.K, self.ptype, self.tol, self.reg_covar, self.max_iter = n_components, weight_concentration_prior_type, tol, reg_covar, max_iter
        self.wc = 1.0 / n_components if weight_concentration_prior is None else weight_concentration_prior
        self.mpp = 1.0 if mean_precision_prior is None else mean_precision_prior

    def _stats(self, X, resp):
        xt = X - self.c                                                   # exact: c is an fp32 vector, X fp32 values in float64
        s2 = np.stack([(xt * resp[:, k:k + 1]).T @ xt for k in range(self.K)])
        return resp.sum(0), resp.T @ xt, s2

    def _m_step(self, nk_raw, s1, s2):
        K, R = s1.shape
        nk = nk_raw + 10 * np.finfo(np.float64).eps
        if self.ptype == DIST:
            self.wa, self.wb = self.wc + nk, np.zeros(K)
        else:
            self.wa, self.wb = 1.0 + nk, self.wc + np.hstack((np.cumsum(nk[::-1])[-2::-1], 0))
        self.mean_precision_ = self.mpp + nk
        xk = (s1 + self.c[None] * nk_raw[:, None]) / nk[:, None]
        self.means_ = (self.mpp * self.mean_prior[None] + nk[:, None] * xk) / self.mean_precision_[:, None]
        self.dof = R + nk
        d = xk - self.c[None]
        sk = s2 - (s1[:, :, None] * d[:, None, :] + d[:, :, None] * s1[:, None, :]) + nk_raw[:, None, None] * d[:, :, None] * d[:, None, :]
        sk = sk / nk[:, None, None] + self.reg_covar * np.eye(R)[None]
        dx = xk - self.mean_prior[None]
        cov = self.cov_prior[None] + nk[:, None, None] * sk + (nk * self.mpp / self.mean_precision_)[:, None, None] * dx[:, :, None] * dx[:, None, :]
        self.covariances_ = cov / self.dof[:, None, None]
        self.precisions_cholesky_ = np.empty_like(cov)
        for k in range(K):
            Lk = np.linalg.cholesky(self.covariances_[k])                  # raises LinAlgError on a non-positive pivot
            self.precisions_cholesky_[k] = E.NumpyEM._tri_inv(Lk).T

    def _log_weights(self):
        from scipy.special import digamma
        if self.ptype == DIST:
            return digamma(self.wa) - digamma(self.wa.sum())
        dab = digamma(self.wa + self.wb)
        return digamma(self.wa) - dab + np.hstack((0, np.cumsum(digamma(self.wb) - dab)[:-1]))

    def _e_step(self, X):
        from scipy.special import digamma
        N, R = X.shape
        log_det = np.log(np.diagonal(self.precisions_cholesky_, axis1=1, axis2=2)).sum(1)
        log_lambda = R * np.log(2.0) + digamma(0.5 * (self.dof[None] - np.arange(R)[:, None])).sum(0)
        ck = (-0.5 * R * np.log(2 * np.pi) + log_det - 0.5 * R * np.log(self.dof) + 0.5 * (log_lambda - R / self.mean_precision_) + self._log_weights())
        w = np.empty((N, self.K))
        for k in range(self.K):
            y = (X - self.means_[k]) @ self.precisions_cholesky_[k]
            w[:, k] = ck[k] - 0.5 * (y * y).sum(1)
        mx = w.max(1)
        log_resp = w - (mx + np.log(np.exp(w - mx[:, None]).sum(1)))[:, None]
        return log_resp

    def _lower_bound(self, log_resp):
        from scipy.special import betaln, gammaln
        R = self.means_.shape[1]
        ld = np.log(np.diagonal(self.precisions_cholesky_, axis1=1, axis2=2)).sum(1) - 0.5 * R * np.log(self.dof)
        log_wishart = np.sum(-(self.dof * ld + self.dof * R * 0.5 * np.log(2.0) + gammaln(0.5 * (self.dof[None] - np.arange(R)[:, None])).sum(0)))
        if self.ptype == DIST:
            log_norm_weight = gammaln(self.wa.sum()) - gammaln(self.wa).sum()
        else:
            log_norm_weight = -np.sum(betaln(self.wa, self.wb))
        return -np.sum(np.exp(log_resp) * log_resp) - log_wishart - log_norm_weight - 0.5 * R * np.sum(np.log(self.mean_precision_))

    def fit(self, X32, labels=None):
        X = X32.astype(np.float64)
        N = X.shape[0]
        self.mean_prior = X.sum(0) / N
        self.c = self.mean_prior.astype(np.float32).astype(np.float64)     # one shift per fit: the fp32-rounded global mean
        xt, d = X - self.c, self.mean_prior - self.c
        self.cov_prior = (xt.T @ xt - N * d[:, None] * d[None, :]) / (N - 1.0)
        if labels is not None:
            resp = np.zeros((N, self.K))
            resp[np.arange(N), labels] = 1.0
            self._m_step(*self._stats(X, resp))
            self.lower_bound_ = -np.inf
        self.converged_, self.n_iter_ = False, 0
        for it in range(1, self.max_iter + 1):
            log_resp = self._e_step(X)
            self._m_step(*self._stats(X, np.exp(log_resp)))
            lb = self._lower_bound(log_resp)
            change, self.lower_bound_, self.n_iter_ = lb - self.lower_bound_, lb, it
            if abs(change) < self.tol:
                self.converged_ = True
                break
        if self.ptype == DIST:
            self.weights_ = self.wa / self.wa.sum()
        else:
            tot = self.wa + self.wb
            w = self.wa / tot * np.hstack((1, np.cumprod((self.wb / tot)[:-1])))
            self.weights_ = w / w.sum()
        return self
