"""Time of the variational mixture fit on a wide representation: the device fit (codes/vbgmm.py -> csrc/vbgmm.hip, vbwide_*)
against the host path `gm_fit_backend: "sklearn"` (device -> host copy of the samples, sklearn.mixture.BayesianGaussianMixture.fit) and, per
iteration, against the device EM fit (codes/emgmm.py) at the same (N, K, R): N = 20 096 (the accurate fit), K = 30, R = 16 and R = 64.

    python profiles/tools/vbwide_fit_time.py [--out profiles/vbwide_fit_time.json] [--widths 16 64] [--reps 5] [--host-reps 1]

fit: a cold fit with max_iter = 50 and tol = 0 (exactly 50 iterations; the k-means labels of the cold start are sklearn's on the host on both
sides), HIP events around fit() on the device, wall time on the host.  per iteration: 50 warm-started iterations from the same fitted state, for
the variational and the EM fit alike, HIP events around fit(), over 50.  One warm-up run, then the median of `reps` runs; the host leg runs
`host-reps` times without a warm-up (minutes at R = 64).  One JSON document.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if not any(os.path.isdir(os.path.join(p, "ladder_latent_data_distribution_modelling_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)

N, K, CENTRES, SPREAD, MAX_ITER = 20096, 30, 30, 0.3, 50
VB = dict(n_components=K, covariance_type="full", tol=0.0, reg_covar=1e-6, n_init=1, weight_concentration_prior_type="dirichlet_process",
          weight_concentration_prior=0.1, random_state=7)
EM = dict(n_components=K, covariance_type="full", tol=0.0, reg_covar=1e-6, n_init=1, random_state=7)


def _draw(rng, R, n):
    c, A = rng.normal(0, SPREAD, (CENTRES, R)), 0.5 * np.eye(R)[None] + rng.normal(0, 0.5 / np.sqrt(R), (CENTRES, R, R))
    i = rng.integers(0, CENTRES, n)
    return (c[i] + np.einsum("nij,nj->ni", A[i], rng.normal(size=(n, R)))).astype(np.float32)


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def _med(secs):
    return dict(seconds_median=round(statistics.median(secs), 5), seconds_min=round(min(secs), 5), seconds_max=round(max(secs), 5))


def cold_fit(cls, kw, Xd, reps):
    secs = []
    for r in range(1 + reps):
        gm = cls(max_iter=MAX_ITER, warm_start=False, **kw)
        s = _events(lambda: gm.fit(Xd))
        assert gm.n_iter_ == MAX_ITER
        if r:
            secs.append(s)
    return _med(secs), gm


def warm_iterations(cls, kw, Xd, reps):
    gm = cls(max_iter=2, warm_start=True, **kw).fit(Xd)
    start = gm._state.clone()
    gm.max_iter = MAX_ITER
    secs = []
    for r in range(1 + reps):
        gm._state.copy_(start)
        s = _events(lambda: gm.fit(Xd))
        assert gm.n_iter_ == MAX_ITER
        if r:
            secs.append(s)
    return dict(_med(secs), ms_per_iteration_median=round(1e3 * statistics.median(secs) / MAX_ITER, 4))


def host_fit(Xd, reps):
    from sklearn.mixture import BayesianGaussianMixture
    secs = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gm = BayesianGaussianMixture(max_iter=MAX_ITER, warm_start=False, **VB).fit(Xd.cpu().numpy().astype(np.float64))
        secs.append(time.perf_counter() - t0)
        assert gm.n_iter_ == MAX_ITER
    return _med(secs), gm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vbwide_fit_time.json"))
    ap.add_argument("--widths", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("vbwide_fit_time.py measures on the GPU: none found")
    warnings.simplefilter("ignore")                                                  # (every run ends unconverged by construction)
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.codes.vbgmm import DeviceBayesianGaussianMixture
    rows = []
    for R in a.widths:
        Xd = torch.as_tensor(_draw(np.random.default_rng(11), R, N)).cuda()
        row = dict(R=R)
        row["device_fit"], gd = cold_fit(DeviceBayesianGaussianMixture, VB, Xd, a.reps)
        row["device_vb_iterations"] = warm_iterations(DeviceBayesianGaussianMixture, VB, Xd, a.reps)
        row["device_em_iterations"] = warm_iterations(DeviceGaussianMixture, EM, Xd, a.reps)
        row["vb_over_em_per_iteration"] = round(row["device_vb_iterations"]["ms_per_iteration_median"] /
                                                row["device_em_iterations"]["ms_per_iteration_median"], 3)
        print(json.dumps(row), flush=True)
        if a.host_reps:
            row["host_sklearn_fit"], gh = host_fit(Xd, a.host_reps)
            row["host_over_device_fit"] = round(row["host_sklearn_fit"]["seconds_median"] / row["device_fit"]["seconds_median"], 1)
            # faster and different is not faster: both legs ran the same 50 iterations from the same labels
            row["lower_bound_rel_difference"] = float(abs(gd.lower_bound_ - gh.lower_bound_) / abs(gh.lower_bound_))
            row["covariance_max_rel_difference"] = float(np.abs(gd.covariances_ - gh.covariances_).max() / np.abs(gh.covariances_).max())
        rows.append(row)
        print(json.dumps(row), flush=True)
    import sklearn
    doc = dict(what="variational mixture fit, N = %d, K = %d: cold fit of %d iterations (seconds) and %d warm-started iterations (ms per iteration), "
                    "HIP events around fit(), one warm-up, median of %d" % (N, K, MAX_ITER, MAX_ITER, a.reps),
               N=N, K=K, centres=CENTRES, spread=SPREAD, max_iter=MAX_ITER, reps=a.reps, host_reps=a.host_reps,
               device_name=torch.cuda.get_device_name(0), sklearn=sklearn.__version__, host_threads=os.environ.get("OMP_NUM_THREADS"), rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
