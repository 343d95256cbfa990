"""Per-iteration time of the EM fit of the "GMM" prior: the device fit (codes/emgmm.py -> csrc/emgmm.hip) against what the
sklearn backend runs for the same call (BaseTrain._fit_GMM_z: device -> host copy of the samples, sklearn.mixture.GaussianMixture.fit on the host,
the float64 broadcast buffer), at the sample counts of the per-epoch fit (2 048) and of the accurate fit (20 096), R = 64, K = 30.

    python profiles/tools/emgmm_fit_time.py [--out profiles/emgmm_fit_time.json] [--sizes 2048 20096] [--reps 5]

Both legs start every timed run from the SAME fitted state (a cold fit of two iterations, not timed: its k-means is host work in both backends) and
run exactly `max_iter` = 20 warm-started EM iterations (tol = 0 never stops early); the time per iteration is the run's wall time, ended by a device
synchronise, over 20.  Warm-up runs first (code objects, allocator, BLAS threads), then the median of `reps` runs; min and max are kept.  The host leg
uses the threads the environment gives it (OMP_NUM_THREADS; recorded).  One JSON document; no GPU, no result.
"""
import argparse
import copy
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

R, K, CENTRES, SPREAD, MAX_ITER = 64, 30, 30, 0.3, 20


def _mix(rng, R, centres, spread):
    return rng.normal(0, spread, (centres, R)), 0.5 * np.eye(R)[None] + rng.normal(0, 0.5 / np.sqrt(R), (centres, R, R))


def _draw(rng, mix, n):
    c, A = mix; i = rng.integers(0, len(c), n)
    return (c[i] + np.einsum("nij,nj->ni", A[i], rng.normal(size=(n, c.shape[1])))).astype(np.float32)


def _summary(secs):
    per_it = sorted(1e3 * s / MAX_ITER for s in secs)
    return dict(ms_per_iteration_median=round(statistics.median(per_it), 4), ms_per_iteration_min=round(per_it[0], 4),
                ms_per_iteration_max=round(per_it[-1], 4), run_seconds=[round(s, 5) for s in secs])


def device_leg(Xd, reps, warmup):
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    kw = dict(n_components=K, covariance_type="full", tol=0.0, reg_covar=1e-6, n_init=1, warm_start=True, random_state=7)
    gm = DeviceGaussianMixture(max_iter=2, **kw).fit(Xd)
    start = gm._state.clone()
    gm.max_iter = MAX_ITER
    secs = []
    for r in range(warmup + reps):
        gm._state.copy_(start)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gm.fit(Xd)
        torch.cuda.synchronize()
        if r >= warmup:
            secs.append(time.perf_counter() - t0)
        print("device run %d: %.4f s" % (r, time.perf_counter() - t0), file=sys.stderr, flush=True)
        assert gm.n_iter_ == MAX_ITER and not gm.converged_
    return dict(_summary(secs), lower_bound=gm.lower_bound_), gm


def host_leg(Xd, reps, warmup):
    """What BaseTrain._fit_GMM_z runs with the sklearn backend: samples to the host as float64, the fit, the broadcast buffer and its host copy."""
    from sklearn.mixture import GaussianMixture
    kw = dict(n_components=K, covariance_type="full", tol=0.0, reg_covar=1e-6, n_init=1, warm_start=True, random_state=7)
    gm0 = GaussianMixture(max_iter=2, **kw).fit(Xd.cpu().numpy().astype(np.float64))
    gm0.max_iter = MAX_ITER
    secs = []
    for r in range(warmup + reps):
        gm = copy.deepcopy(gm0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gm.fit(Xd.cpu().numpy().astype(np.float64))
        buf = torch.zeros(K + K * R + K * R * R, dtype=torch.float64, device=Xd.device)
        buf.copy_(torch.as_tensor(np.concatenate([gm.weights_.ravel(), gm.means_.ravel(), gm.covariances_.ravel()])))
        buf.cpu().numpy()
        torch.cuda.synchronize()
        if r >= warmup:
            secs.append(time.perf_counter() - t0)
        print("host run %d: %.4f s" % (r, time.perf_counter() - t0), file=sys.stderr, flush=True)
        assert gm.n_iter_ == MAX_ITER and not gm.converged_
    return dict(_summary(secs), lower_bound=float(gm.lower_bound_)), gm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emgmm_fit_time.json"))
    ap.add_argument("--sizes", type=int, nargs="+", default=[2048, 20096])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("emgmm_fit_time.py measures on the GPU: none found")
    warnings.simplefilter("ignore")                                                  # (every run ends unconverged by construction)
    rng = np.random.default_rng(11)
    mix = _mix(rng, R, CENTRES, SPREAD)
    rows = []
    for N in a.sizes:
        Xd = torch.as_tensor(_draw(rng, mix, N)).cuda()
        dev, gd = device_leg(Xd, a.reps, a.warmup)
        host, gh = host_leg(Xd, a.reps, 1)
        # faster and different is not faster: both legs ran the same 2 + 20 iterations from the same labels
        agree = float(np.abs(gd.covariances_ - gh.covariances_).max() / np.abs(gh.covariances_).max())
        rows.append(dict(n_samples=N, device=dev, host_sklearn=host, covariance_max_rel_difference=agree,
                         host_over_device=round(host["ms_per_iteration_median"] / dev["ms_per_iteration_median"], 1)))
        print(json.dumps(rows[-1]), flush=True)
    import sklearn
    doc = dict(what="EM fit of the GMM prior: ms per EM iteration, %d warm-started iterations per run, median of %d runs" % (MAX_ITER, a.reps),
               R=R, K=K, centres=CENTRES, spread=SPREAD, max_iter=MAX_ITER, reps=a.reps, device_name=torch.cuda.get_device_name(0),
               sklearn=sklearn.__version__, host_threads=os.environ.get("OMP_NUM_THREADS"), rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
