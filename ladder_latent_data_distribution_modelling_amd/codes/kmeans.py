"""Device-resident k-means: the labels a cold mixture fit starts from (codes/base.py:93-106 through BaseMixture._initialize_parameters).

`DeviceKMeans` keeps sklearn.cluster.KMeans' constructor arguments and fitted attributes (`labels_`, `cluster_centers_`, `n_iter_`,
`inertia_`) for the options the mixtures use (n_init=1, algorithm="lloyd", init "k-means++" or an array), but runs k-means++ seeding and
Lloyd's iteration in float64 on samples that never leave the GPU (csrc/kmeans.hip or csrc/kmeans_wide.hip: the family is looked up by the samples'
width at fit time, operation "kmeans" of mixture_forms.py).  The host contributes the
random numbers of the seeding (codes/mixture_fit.py: kmeans_draws consumes the generator exactly as sklearn does) and reads the `done`
flag and four scalars; with the same `random_state` a fit gives sklearn's labels and iteration count (tests/test_gpu_kmeans.py,
tests/test_gpu_kmeans_wide.py).
"""
import numpy as np
import torch

from .. import _lib as L
from ..mixture_forms import family
from . import mixture_fit as MF


class DeviceKMeans:
    def __init__(self, n_clusters=8, n_init=1, max_iter=300, tol=1e-4, init="k-means++", random_state=None, algorithm="lloyd", device="cuda:0"):
        if n_init != 1 or algorithm != "lloyd":
            raise NotImplementedError("the HIP k-means covers n_init=1, algorithm='lloyd' (what the mixture fits use)")
        if isinstance(init, str) and init != "k-means++":
            raise NotImplementedError("the HIP k-means starts from init='k-means++' or an array of centres")
        if int(max_iter) < 1:
            raise ValueError("max_iter must be >= 1, got %r" % (max_iter,))
        self.n_clusters, self.n_init, self.max_iter, self.tol, self.init = int(n_clusters), 1, int(max_iter), float(tol), init
        self.random_state, self.algorithm = random_state, algorithm
        self.device = torch.device(device)
        self._state = None

    def fit(self, X, y=None, check_every=16):
        """X: [N,R] torch tensor on the device (preferred) or array-like.  Seeding and up to max_iter + 1 assign / update pairs are enqueued
        without waiting; the `done` flag is read every `check_every` iterations (the result does not depend on it)."""
        from sklearn.utils import check_random_state
        K = self.n_clusters
        Xd = MF.device_samples(X, self.device)
        N, R = Xd.shape
        if N < K:
            raise ValueError("n_samples=%d should be >= n_clusters=%d." % (N, K))
        form = family("kmeans", K, R)
        st = torch.cuda.current_stream(self.device).cuda_stream
        state = torch.zeros(L.query(form.state_doubles, K, R), dtype=torch.float64, device=self.device)
        ws = torch.empty(L.query(form.workspace_bytes, N, K, R), dtype=torch.uint8, device=self.device)
        labels = torch.empty(N, dtype=torch.int32, device=self.device)
        head = (Xd.data_ptr(), N, K, R)
        if isinstance(self.init, str):
            first, u = MF.kmeans_draws(check_random_state(self.random_state), N, K)
            start = torch.as_tensor(np.concatenate([[float(first)], u.ravel()])).to(self.device)
            assert start.numel() == L.query(form.draws_doubles, K)
        else:
            centres = np.ascontiguousarray(self.init, dtype=np.float64)
            if centres.shape != (K, R):
                raise ValueError("The shape of the initial centers %s does not match the number of clusters %d and features %d."
                                 % (centres.shape, K, R))
            start = torch.as_tensor(centres).to(self.device)
        L.call(form.seed if isinstance(self.init, str) else form.set_centres, *head, start.data_ptr(), state.data_ptr(), ws.data_ptr(), ws.numel(), st)
        lib = L.load()
        assign_fn, update_fn = getattr(lib, form.assign), getattr(lib, form.update)
        a_tail = (state.data_ptr(), labels.data_ptr(), ws.data_ptr(), ws.numel(), st)
        u_head = head + (labels.data_ptr(), state.data_ptr(), self.tol, self.max_iter)
        u_tail = (ws.data_ptr(), ws.numel(), st)
        # (pair max_iter + 1 is the assignment against the final centres of a fit that did not stop on unchanged labels)
        MF.iterate_until_done(lambda it: assign_fn(*head, it, *a_tail), lambda it: update_fn(*u_head, it, *u_tail), None, None, state[-1:], 1,
                              self.max_iter + 1, check_every, "k-means")
        tail = state[-4:].cpu().numpy()
        self.inertia_, self.n_iter_, self._status = float(tail[0]), int(tail[1]), int(tail[2])
        self._state, self.labels_dev, self._shape = state, labels, (K, R)
        self.n_features_in_ = R
        return self

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    @property
    def labels_(self):
        return self.labels_dev.cpu().numpy()

    @property
    def cluster_centers_(self):
        K, R = self._shape
        return self._state[:K * R].reshape(K, R).cpu().numpy()
