"""Every output of the three device mixture fits on fixed seeded inputs, written to one .npz -- for whichever library LADDER_HIP_LIB names.

    LADDER_HIP_LIB=/path/to/libladder_hip.so python profiles/fit_outputs.py out.npz
    python profiles/fit_outputs.py --compare a.npz b.npz        # table of np.array_equal per array (NaN positions must match too)

Run it once per build, each in a fresh process (in a checkout of the other commit where the Python differs too: the tool uses the public classes
only), and compare: two builds whose fit kernels compute the same thing give equal arrays bit for bit.  Per fit it records the float64 state, the
fp32 feed, n_iter_ / converged_ / lower_bound_ and -- for the fits that exchange statistics, through a one-rank communicator that keeps a
reference to what it is handed -- the all-reduced `stats` of the last iteration.  Cases: EM cold + warm on emgmm_ref.CASES[0..3]; the wide
variational fit cold + warm on vbwide_ref.CASES 0, 2, 5, 6 (both prior types, K = 1, R = 9 / 17 / 33, a one-sample last slice); the narrow one at
N = 600 (persistent kernel) and N = 1100 (sliced), R = 2 and 8, both prior types; per family max_iter = 0, an ill-defined covariance, and
check_every = 1 and 16.  k-means labels come from sklearn with a fixed random_state, so both builds start from the same labels.
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mixture_outputs import compare  # noqa: E402


class KeepingComm:
    """One rank with the exchange switched on: every collective is the identity; keeps the tensors all-reduced, so the last one is `stats`."""
    on, rank, world, group = True, 0, 1, None

    def __init__(self):
        self.reduced = []

    def allreduce_(self, t):
        self.reduced.append(t)
        return t

    @staticmethod
    def broadcast_(t, src):
        return t

    class dist:
        @staticmethod
        def all_gather(parts, x, group=None):
            parts[0].copy_(x)


def main(out_path):
    import torch
    import emgmm_ref as E
    import vbwide_ref as V
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.codes import mixture_fit as MF
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.codes.vbgmm import DeviceBayesianGaussianMixture
    out = {"library": np.array(os.environ.get("LADDER_HIP_LIB", L.LIB_PATH))}
    last, read_tail = {}, MF.read_tail
    MF.read_tail = lambda state: (last.update(state=state), read_tail(state))[1]         # the state of a fit that raises is kept too

    def record(tag, gm, Xs, check_every=None):
        """fit() on each of Xs in turn (cold, then warm), or fit_sharded through a KeepingComm if check_every is given."""
        for f, X in enumerate(Xs):
            comm, err = KeepingComm(), 0
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                try:
                    gm.fit(torch.as_tensor(X).cuda()) if check_every is None else gm.fit_sharded(torch.as_tensor(X).cuda(), comm, check_every=check_every)
                except ValueError:
                    err = 1
            torch.cuda.synchronize()
            t = "%s_fit%d" % (tag, f)
            out[t + "_state"] = last["state"].cpu().numpy()
            out[t + "_raised"] = np.array(err)
            if check_every is not None:
                out[t + "_stats"] = comm.reduced[-1].cpu().numpy()
                out[t + "_exchanges"] = np.array([x.numel() for x in comm.reduced])
            if not err:
                out[t + "_tail"] = np.array([gm.lower_bound_, gm.n_iter_, gm.converged_], dtype=np.float64)
                for name in ("weights_dev", "means_dev", "covariances_dev"):
                    out["%s_%s" % (t, name)] = getattr(gm, name).cpu().numpy()

    def em(K, max_iter, **kw):
        return DeviceGaussianMixture(n_components=K, max_iter=max_iter, **dict(E.KW, **kw))

    def vb(K, ptype, max_iter, **kw):
        return DeviceBayesianGaussianMixture(**dict(dict(n_components=K, covariance_type="full", max_iter=max_iter, weight_concentration_prior_type=ptype,
                                                         weight_concentration_prior=0.1, warm_start=True, random_state=7), **kw))

    # ---- EM
    for i in range(4):
        N, R, K, max_iter, centres, spread, seed, _ = E.CASES[i]
        Xs = E.data(N, R, centres, spread, seed)
        record("em_%dx%dx%d" % (N, R, K), em(K, max_iter), Xs)
        record("em_%dx%dx%d_sharded" % (N, R, K), em(K, max_iter), Xs, check_every=8)
    N, R, K, max_iter, centres, spread, seed, _ = E.CASES[2]
    Xs = E.data(N, R, centres, spread, seed)
    for ce in (1, 16):
        record("em_check_every%d" % ce, em(K, max_iter), Xs, check_every=ce)
    record("em_max_iter0", em(K, 0), Xs[:1], check_every=8)
    record("em_ill_defined", em(2, 100, reg_covar=0.0), [np.full((80, 12), 0.5, dtype=np.float32)], check_every=8)

    # ---- wide variational
    for i in (0, 2, 5, 6):
        record("vbwide_%s" % V.IDS[i], DeviceBayesianGaussianMixture(**V.kwargs(i)), V.samples(i))
        record("vbwide_%s_sharded" % V.IDS[i], DeviceBayesianGaussianMixture(**V.kwargs(i)), V.samples(i), check_every=8)
    for ce in (1, 16):
        record("vbwide_check_every%d" % ce, DeviceBayesianGaussianMixture(**V.kwargs(2)), V.samples(2), check_every=ce)
    record("vbwide_max_iter0", DeviceBayesianGaussianMixture(**dict(V.kwargs(2), max_iter=0)), V.samples(2)[:1], check_every=8)
    record("vbwide_ill_defined", vb(2, V.PROC, 100, reg_covar=0.0), [np.full((80, 12), 0.5, dtype=np.float32)], check_every=8)

    # ---- narrow variational: the persistent kernel below SLICED_FIT_MIN_SAMPLES, the sliced kernels from there on
    for N in (600, 1100):
        for R, K in ((2, 10), (8, 7)):
            for ptype in (V.DIST, V.PROC):
                Xs = E.data(N, R, 6, 1.0, 100 + R)
                tag = "vb_%dx%dx%d_%s" % (N, R, K, ptype)
                record(tag, vb(K, ptype, 100), Xs)
                record(tag + "_sharded", vb(K, ptype, 100), Xs, check_every=8)
    Xs = E.data(1100, 8, 6, 1.0, 108)
    for ce in (1, 16):
        record("vb_check_every%d" % ce, vb(7, V.PROC, 100), Xs, check_every=ce)
    for N in (600, 1100):
        record("vb_%d_max_iter0" % N, vb(7, V.PROC, 0), [Xs[0][:N]])
    record("vb_max_iter0_sharded", vb(7, V.PROC, 0), Xs[:1], check_every=8)
    record("vb_ill_defined_persistent", vb(2, V.DIST, 100, reg_covar=0.0), [np.full((64, 2), 0.5, dtype=np.float32)])
    record("vb_ill_defined_sharded", vb(2, V.DIST, 100, reg_covar=0.0), [np.full((64, 2), 0.5, dtype=np.float32)], check_every=8)

    np.savez(out_path, **out)
    print("wrote %d arrays to %s (library: %s)" % (len(out), out_path, out["library"]))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
