"""Device-resident replacement for the sklearn mixture object of codes/base.py:93-99.

`DeviceBayesianGaussianMixture` keeps sklearn.mixture.BayesianGaussianMixture's constructor arguments and fitted
attributes (`weights_`, `means_`, `covariances_`, `n_iter_`, `lower_bound_`, `converged_`) for the options the reference
uses (covariance_type='full'; dirichlet_distribution for the per-epoch "fast" fit, dirichlet_process for the final
"accurate" fit; warm_start; n_init restarts), but runs the variational loop as one persistent-workgroup HIP launch
(`ladder_vbgmm_fit`, csrc/vbgmm.hip) on samples that never leave the GPU.  The k-means initialisation of a cold fit is
sklearn.cluster.KMeans on the host (exactly the call BaseMixture._initialize_parameters makes) with kmeans_backend="sklearn", the
default, and the same algorithm on the device with kmeans_backend="hip" (codes/kmeans.py: the same labels; "hip_wide", the word of the wide
"GMM" prior, is accepted and means the same here, since this fit ends at 64 dimensions); either way a fit with the
same `random_state` reproduces sklearn's to float64 round-off (tests/test_gpu_vbgmm.py, tests/test_gpu_kmeans.py).

Width of the representation (operation "vb" of mixture_forms.py): the packed tier runs the thread-per-sample kernels (the persistent launch below
SLICED_FIT_MIN_SAMPLES samples, the sharded entries from there on and for sharded fits); the dense tier runs the float64-MFMA entries for every N
-- the passes the EM fit of codes/emgmm.py uses (csrc/fit_mfma.h) -- with the same protocol, state front and fitted attributes
(tests/test_gpu_vbgmm_wide.py); there is no wide family.  1 <= K <= 64 for both.  The fit takes every dense width: the engine's dense mixture term
and SLP interpolation (csrc/slp_wide.hip: n_step * R <= 2048) also need R % 4 == 0.
"""
import numpy as np
import torch

from .. import _lib as L
from ..mixture_forms import VB_PACKED, family
from . import mixture_fit as MF


# from this many samples on, fit() runs one E-step launch over 256-sample slices (one workgroup each) + one M-step launch per variational
# iteration instead of the single persistent workgroup: 3.8 ms -> ~30 us per iteration at the 20 096 samples of the accurate fit
SLICED_FIT_MIN_SAMPLES = 1024
NARROW_MAX_R = VB_PACKED.hi              # past this width the fit runs the dense tier's entries for every N; the persistent launch is the packed tier's


class DeviceBayesianGaussianMixture:
    def __init__(self, n_components=1, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1,
                 init_params="kmeans", weight_concentration_prior_type="dirichlet_process", weight_concentration_prior=None,
                 mean_precision_prior=None, warm_start=False, random_state=None, device="cuda:0", label_broadcast=None,
                 kmeans_backend="sklearn"):
        if covariance_type != "full" or init_params != "kmeans":
            raise NotImplementedError("the HIP fit covers covariance_type='full', init_params='kmeans' (what the reference uses)")
        if weight_concentration_prior_type not in ("dirichlet_distribution", "dirichlet_process"):
            raise ValueError(weight_concentration_prior_type)
        self.n_components, self.tol, self.reg_covar, self.max_iter, self.n_init = int(n_components), tol, reg_covar, int(max_iter), int(n_init)
        self.weight_concentration_prior_type = weight_concentration_prior_type
        self.weight_concentration_prior = weight_concentration_prior
        self.mean_precision_prior = mean_precision_prior
        self.warm_start, self.random_state = warm_start, random_state
        self.device = torch.device(device)
        self._label_broadcast = label_broadcast       # data-parallel hook: rank 0's k-means labels -> every rank
        self.kmeans_backend = MF.check_kmeans_backend(kmeans_backend)
        self._state = None

    # -------------------------------------------------------------------------------------------------------------
    def _prior_args(self):
        """(prior type, weight concentration prior, mean precision prior) as the kernels take them, with sklearn's defaults 1 / K and 1."""
        return (0 if self.weight_concentration_prior_type == "dirichlet_distribution" else 1,
                1.0 / self.n_components if self.weight_concentration_prior is None else float(self.weight_concentration_prior),
                1.0 if self.mean_precision_prior is None else float(self.mean_precision_prior))

    def fit(self, X, y=None):
        """X: [N,R] torch tensor on the device (preferred) or array-like."""
        K = self.n_components
        Xd = MF.device_samples(X, self.device)
        N, R = Xd.shape
        MF.check_sample_count(N, K)
        if R > NARROW_MAX_R or N >= SLICED_FIT_MIN_SAMPLES:
            return self.fit_sharded(Xd, MF.OneRank(), check_every=16)
        form = family("vb", K, R)
        ptype, wc, mp = self._prior_args()
        ws = torch.empty(L.query(form.fit_workspace_bytes, N, K), dtype=torch.uint8, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        do_init, rs, n_fits = MF.fit_plan(self)

        def one_fit():
            state = torch.zeros(L.query(form.state_doubles, K, R), dtype=torch.float64, device=self.device) if do_init else self._state
            labels = self._initial_labels(Xd, MF.OneRank(), rs) if do_init else None
            w, m, c = MF.feed_tensors(K, R, self.device)
            L.call(form.fit, Xd.data_ptr(), N, K, R, labels.data_ptr() if labels is not None else None, state.data_ptr(),
                   ptype, wc, mp, float(self.reg_covar), float(self.tol), self.max_iter, w.data_ptr(), m.data_ptr(), c.data_ptr(),
                   ws.data_ptr(), ws.numel(), st)
            return state, w, m, c                          # (the one host sync of the fit: the tail read of best_of_restarts)

        return MF.keep_best(self, MF.best_of_restarts(n_fits, one_fit))

    def _initial_labels(self, Xd, comm, rs):
        return MF.initial_labels_for(self.kmeans_backend, Xd, comm, self.n_components, rs, self._label_broadcast)

    # -------------------------------------------------------------------------------------------------------------
    def fit_sharded(self, X_local, comm, check_every=8):
        """The same fit with the samples SHARDED over the data-parallel ranks (exchange step C5 of SURVEY 2.3 as north_star words it:
        an all-reduce of the mixture's sufficient statistics): `X_local` [N_local, R] are THIS rank's samples, `comm` the engine's
        communicator (all-reduce over RCCL / xGMI).  The loop is MF.fit_sliced's: per variational iteration E-step + local statistics,
        all-reduce of 1 + K + K R + K R^2 doubles, M-step + lower bound + convergence test; the result does not depend on `check_every`.
        The dense tier's family runs the same loop, with the data-derived priors from two small all-reduces ([sum x | N], then the second
        moments about the shift that defines)."""
        Xd = MF.device_samples(X_local, self.device)
        R = Xd.shape[1]
        form = family("vb", self.n_components, R)
        ptype, wc, mp = self._prior_args()

        def moments(Xd, comm, f64, st, check):
            Nl = Xd.shape[0]
            mom = f64(L.query(form.moments_doubles, R))
            if form.moments_by_pass:
                L.call(form.moments, Xd.data_ptr(), Nl, R, mom.data_ptr(), 0, st)
                comm.allreduce_(mom[:R + 1])                                   # [ sum x | N ]: the shift, mean_prior_ and the global count
                check(int(mom[R].item()))
                L.call(form.moments, Xd.data_ptr(), Nl, R, mom.data_ptr(), 1, st)
                comm.allreduce_(mom[R + 1:])                                   # sum x~ x~^T about that shift: covariance_prior_
            else:
                L.call(form.moments, Xd.data_ptr(), Nl, R, mom.data_ptr(), st)
                comm.allreduce_(mom)
                n_glob = torch.full((1,), float(Nl), dtype=torch.float64, device=self.device)
                comm.allreduce_(n_glob)
                check(int(n_glob.item()))
            return mom

        fam = MF.Family(form, moments, lambda mom: (ptype, mom.data_ptr()) if form.estep_takes_moments else (ptype,), (ptype, wc, mp),
                        "sharded mixture fit")
        return MF.keep_best(self, MF.fit_sliced(self, Xd, comm, check_every, fam))

    # float64 views of the fitted parameters, as sklearn exposes them
    def _unpack(self):
        K = self.n_components
        s = self._state.cpu().numpy()
        R = self.means_dev.shape[1]
        wa, wb = s[:K], s[K:2 * K]
        means = s[4 * K:4 * K + K * R].reshape(K, R)
        cov = s[4 * K + K * R:4 * K + K * R + K * R * R].reshape(K, R, R)
        if self.weight_concentration_prior_type == "dirichlet_distribution":
            w = wa / wa.sum()
        else:
            tot = wa + wb
            w = wa / tot * np.hstack((1, np.cumprod((wb / tot)[:-1])))
            w = w / w.sum()
        return w, means.copy(), cov.copy()

    @property
    def weights_(self):
        return self._unpack()[0]

    @property
    def means_(self):
        return self._unpack()[1]

    @property
    def covariances_(self):
        return self._unpack()[2]
