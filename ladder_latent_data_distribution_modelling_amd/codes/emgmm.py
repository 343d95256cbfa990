"""Device-resident replacement for the sklearn mixture object of the baseline "GMM" prior (codes/base.py:101-106, 699-710, 749-767).

`DeviceGaussianMixture` keeps sklearn.mixture.GaussianMixture's constructor arguments and fitted attributes (`weights_`, `means_`,
`covariances_`, `precisions_cholesky_`, `n_iter_`, `lower_bound_`, `converged_`) for the options the reference uses
(covariance_type='full', init_params='kmeans'; warm_start; n_init restarts), but runs the EM loop in float64 on samples that never
leave the GPU (csrc/emgmm.hip or csrc/emgmm_wide.hip, both 1 <= K <= 64: the family is looked up by the samples' width at fit time, operation "em" of
mixture_forms.py), on one GPU or with the samples sharded over the data-parallel ranks.  The k-means
initialisation of a cold fit (codes/mixture_fit.py, shared with codes/vbgmm.py) is sklearn's on the host with kmeans_backend="sklearn" (the
default) and the same algorithm on the device with kmeans_backend="hip" or "hip_wide" (codes/kmeans.py, whatever word was used: the same labels,
tests/test_gpu_kmeans.py, tests/test_gpu_kmeans_wide.py); either way a fit with the same `random_state` reproduces sklearn's to float64 round-off.
"""
import numpy as np
import torch

from .. import _lib as L
from ..mixture_forms import family, sized_workspace
from . import mixture_fit as MF


class DeviceGaussianMixture:
    def __init__(self, n_components=1, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1, init_params="kmeans",
                 weights_init=None, means_init=None, precisions_init=None, warm_start=False, random_state=None, device="cuda:0",
                 label_broadcast=None, kmeans_backend="sklearn"):
        if covariance_type != "full" or init_params != "kmeans":
            raise NotImplementedError("the HIP fit covers covariance_type='full', init_params='kmeans' (what the reference uses)")
        if weights_init is not None or means_init is not None or precisions_init is not None:
            raise NotImplementedError("the HIP fit starts from k-means labels: weights_init / means_init / precisions_init are not supported")
        self.n_components, self.tol, self.reg_covar, self.max_iter, self.n_init = int(n_components), tol, reg_covar, int(max_iter), int(n_init)
        self.covariance_type, self.init_params = covariance_type, init_params
        self.warm_start, self.random_state = warm_start, random_state
        self.device = torch.device(device)
        self._label_broadcast = label_broadcast       # data-parallel hook: rank 0's k-means labels -> every rank
        self.kmeans_backend = MF.check_kmeans_backend(kmeans_backend)
        self._state = None

    # -------------------------------------------------------------------------------------------------------------
    def fit(self, X, y=None):
        """X: [N,R] torch tensor on the device (preferred) or array-like."""
        return self.fit_sharded(X, MF.OneRank(), check_every=16)

    def _initial_labels(self, Xd, comm, rs):
        return MF.initial_labels_for(self.kmeans_backend, Xd, comm, self.n_components, rs, self._label_broadcast)

    def fit_sharded(self, X_local, comm, check_every=8):
        """The fit with the samples SHARDED over the data-parallel ranks: `X_local` [N_local, R] are THIS rank's samples, `comm` the engine's
        communicator.  The loop is MF.fit_sliced's: per EM iteration E-step + local statistics, all-reduce of 1 + K (1 + R + R^2) doubles
        (the sum of log_prob_norm travels with the moments: the lower bound is a global mean), M-step + convergence test."""
        K, R = self.n_components, int(np.shape(X_local)[1])
        form = family("em", K, R)
        mws, m_mid = sized_workspace(form.factor_workspace_bytes, self.device, K, R)       # (alive until every launch of the fit is enqueued)

        def moments(Xd, comm, f64, st, check):
            Nl, R = Xd.shape
            mom = f64(L.query(form.shift_doubles, R))                          # [ sum_n x_n | N ]: the shift vector and the global count
            L.call(form.shift, Xd.data_ptr(), Nl, R, mom.data_ptr(), st)
            comm.allreduce_(mom)
            check(int(mom[-1].item()))
            self.converged_ = False                                            # (sklearn sets it before the first restart: a failed fit leaves it)
            return mom

        fam = MF.Family(form, moments, lambda mom: (mom.data_ptr(),), m_mid, "EM mixture fit")
        MF.keep_best(self, MF.fit_sliced(self, X_local, comm, check_every, fam))
        self._R = self.means_dev.shape[1]
        return self

    def _prepare_state(self, state, R):
        """precisions_cholesky_ / log-determinants for the covariances already in `state`; raises sklearn's ValueError on an ill-defined one."""
        form = family("em", self.n_components, R)
        ws, mid = sized_workspace(form.factor_workspace_bytes, self.device, self.n_components, R)
        L.call(form.prepare, state.data_ptr(), self.n_components, R, *mid, torch.cuda.current_stream(self.device).cuda_stream)
        MF.read_tail(state)                                                    # (synchronises: `ws` outlives the kernels)

    # float64 views of the fitted parameters, as sklearn exposes them (layout: csrc/em_state.h)
    def _unpack(self):
        K, R = self.n_components, self._R
        s = self._state.cpu().numpy()
        o = np.cumsum([0, K, K * R, K * R * R, K * R * R])
        return (s[o[0]:o[1]].copy(), s[o[1]:o[2]].reshape(K, R).copy(), s[o[2]:o[3]].reshape(K, R, R).copy(),
                s[o[3]:o[4]].reshape(K, R, R).copy())

    @property
    def weights_(self):
        return self._unpack()[0]

    @property
    def means_(self):
        return self._unpack()[1]

    @property
    def covariances_(self):
        return self._unpack()[2]

    @property
    def precisions_cholesky_(self):
        return self._unpack()[3]
