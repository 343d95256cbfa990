"""Shared by tests/test_emgmm_cpu.py and tests/test_gpu_emgmm.py: the test mixtures, the parity cases, and a float64 numpy restatement of the
ALGORITHM of csrc/emgmm.hip (one shift vector, shifted raw moments centred in the M-step, Cholesky + triangular inverse, the fit_predict loop).
The restatement and the kernels differ in summation order only; it pins the algorithm against sklearn on machines without a GPU and is
what a tolerance wider than the project's bars would have to be derived from."""
import warnings

import numpy as np


def _mix(rng, R, centres, spread):
    return rng.normal(0, spread, (centres, R)), 0.5 * np.eye(R)[None] + rng.normal(0, 0.5 / np.sqrt(R), (centres, R, R))


def _draw(rng, mix, n):
    c, A = mix; i = rng.integers(0, len(c), n)
    return (c[i] + np.einsum("nij,nj->ni", A[i], rng.normal(size=(n, c.shape[1])))).astype(np.float32)


def data(N, R, centres, spread, seed):
    """(X1, X2): the samples of a cold fit and of its warm-started refit, both from the SAME mixture."""
    rng = np.random.default_rng(seed)
    mix = _mix(rng, R, centres, spread)
    X1 = _draw(rng, mix, N)
    X2 = _draw(rng, mix, N)
    return X1, X2


# N, R, K, max_iter, centres, spread, seed, sklearn n_iter (cold, warm; None = cold fit only)
CASES = [
    (600, 3, 7, 200, 9, 1.0, 9, (23, 7)),          # R below one MFMA tile
    (1027, 8, 7, 200, 9, 0.6, 5, (22, 6)),         # ragged slice, R = 8
    (1100, 33, 6, 200, 8, 0.35, 4, (14, 11)),      # R just past a tile multiple
    (2051, 16, 5, 200, 7, 0.5, 1, (20, 4)),        # exact tile, ragged N
    (1300, 64, 3, 200, 5, 0.25, 8, (7, 3)),        # R at the limit
    (5003, 2, 12, 2000, 5, 1.5, 5, (9, 5)),        # many slices
    (4099, 64, 30, 3, 30, 0.3, 2, (3, None)),      # full K R width, unconverged; the refit would leave a component 15 samples in 64 dimensions
    (129, 5, 1, 200, 3, 1.0, 5, (2, 3)),           # two full slices and a one-sample slice, K = 1
    (257, 17, 2, 200, 3, 0.5, 4, (4, 5)),          # two components at an R just past a tile, one-sample last slice
]
KW = dict(covariance_type="full", tol=1e-3, reg_covar=1e-6, n_init=1, warm_start=True, random_state=7)

# the project's bars of the sharded VB fit (tests/test_gpu_vbgmm.py), which also centres raw moments: (relative, absolute floor).
# precisions_cholesky_ is a function of the covariance alone (Cholesky + triangular inverse) and takes the covariance's bar; the numpy restatement
# below, which differs from the kernels in summation order only, sits at <= 1.2e-9 absolute / 3e-12 relative from sklearn on every case of CASES.
BAR_LB = 1e-8
BARS = {"weights_": (1e-7, 1e-11), "means_": (1e-7, 1e-9), "covariances_": (1e-6, 1e-9), "precisions_cholesky_": (1e-6, 1e-9)}


def assert_iteration_count_is_decidable(ref, tol, max_iter):
    """So that round-off cannot decide the iteration count: on the reference's own lower_bounds_ the last |change| is <= 0.97 tol and the one
    before it >= 1.03 tol, or the fit ended at max_iter."""
    lb = np.asarray(ref.lower_bounds_)
    if not ref.converged_:
        assert len(lb) == max_iter
        return
    prev = ref._emgmm_prev_lb
    ch = np.abs(np.diff(np.concatenate([[prev], lb])))
    assert ch[-1] <= 0.97 * tol, ch[-3:]
    assert len(ch) < 2 or ch[-2] >= 1.03 * tol, ch[-3:]


def sklearn_fit(ref, X):
    """ref.fit(float64 copy of X), remembering the lower bound the fit started from (-inf for a cold start)."""
    ref._emgmm_prev_lb = ref.lower_bound_ if (ref.warm_start and hasattr(ref, "converged_")) else -np.inf
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ref.fit(X.astype(np.float64))
    return [x for x in w if x.category.__name__ == "ConvergenceWarning"]


def assert_close(dev, ref):
    assert abs(dev.lower_bound_ - ref.lower_bound_) <= BAR_LB * abs(ref.lower_bound_), (dev.lower_bound_, ref.lower_bound_)
    for name, (rtol, atol) in BARS.items():
        np.testing.assert_allclose(getattr(dev, name), getattr(ref, name), rtol=rtol, atol=atol, err_msg=name)


class NumpyEM:
    """The device algorithm in float64 numpy.  fit(X, labels=None): labels = the hard assignment of a cold start, None = warm start."""

    def __init__(self, n_components, tol=1e-3, reg_covar=1e-6, max_iter=100):
        self.K, self.tol, self.reg_covar, self.max_iter = n_components, tol, reg_covar, max_iter

    def _stats(self, X, resp):
        xt = X - self.c                                                   # exact: c is an fp32 vector, X fp32 values in float64
        nk = resp.sum(0)
        s1 = resp.T @ xt
        s2 = np.einsum("nk,ni,nj->kij", resp, xt, xt)
        return nk, s1, s2

    def _m_step(self, nk_raw, s1, s2, n_samples, first):
        K, R = s1.shape
        nk = nk_raw + 10 * np.finfo(np.float64).eps
        self.weights_ = nk / n_samples if first else nk / nk.sum()
        self.means_ = (s1 + self.c[None] * nk_raw[:, None]) / nk[:, None]
        d = self.means_ - self.c[None]
        cov = s2 - (s1[:, :, None] * d[:, None, :] + d[:, :, None] * s1[:, None, :]) + nk_raw[:, None, None] * d[:, :, None] * d[:, None, :]
        cov = cov / nk[:, None, None] + self.reg_covar * np.eye(R)[None]
        self.covariances_ = cov
        self.precisions_cholesky_ = np.empty_like(cov)
        for k in range(K):
            Lk = np.linalg.cholesky(cov[k])                                # raises LinAlgError on a non-positive pivot
            self.precisions_cholesky_[k] = self._tri_inv(Lk).T
        self.log_det_ = np.log(np.diagonal(self.precisions_cholesky_, axis1=1, axis2=2)).sum(1)

    @staticmethod
    def _tri_inv(Lk):
        R = Lk.shape[0]
        X = np.zeros_like(Lk)
        for c in range(R):
            X[c, c] = 1.0 / Lk[c, c]
            for i in range(c + 1, R):
                X[i, c] = -(Lk[i, c:i] @ X[c:i, c]) / Lk[i, i]
        return X

    def _e_step(self, X):
        N, R = X.shape
        lp = np.empty((N, self.K))
        for k in range(self.K):
            y = (X - self.means_[k]) @ self.precisions_cholesky_[k]
            lp[:, k] = -0.5 * (R * np.log(2 * np.pi) + (y * y).sum(1)) + self.log_det_[k] + np.log(self.weights_[k])
        mx = lp.max(1)
        lpn = np.log(np.exp(lp - mx[:, None]).sum(1)) + mx
        return lpn, np.exp(lp - lpn[:, None])

    def fit(self, X32, labels=None):
        X = X32.astype(np.float64)
        N = X.shape[0]
        self.c = (X.sum(0) / N).astype(np.float32).astype(np.float64)       # one shift per fit: the fp32-rounded global mean
        if labels is not None:
            resp = np.zeros((N, self.K))
            resp[np.arange(N), labels] = 1.0
            self._m_step(*self._stats(X, resp), N, True)
            self.lower_bound_ = -np.inf
        self.converged_, self.n_iter_ = False, 0
        for it in range(1, self.max_iter + 1):
            lpn, resp = self._e_step(X)
            self._m_step(*self._stats(X, resp), N, False)
            lb = lpn.sum() / N
            change, self.lower_bound_, self.n_iter_ = lb - self.lower_bound_, lb, it
            if abs(change) < self.tol:
                self.converged_ = True
                break
        return self
