"""Per-iteration time of the variational Bayesian mixture fit (codes/vbgmm.py -> csrc/vbgmm.hip) on both of its paths: the
persistent one-workgroup kernel at N = 1 000 and the sliced E-step / M-step launches at N = 20 096 (the accurate fit), R = 8, K = 50,
Dirichlet-distribution weights.

    python profiles/tools/vbgmm_fit_time.py [--out profiles/vbgmm_fit_time.json] [--lib other/libladder_hip.so ...] [--reps 5]

Every timed run starts from the SAME cloned state (a cold fit of two iterations, not timed: its k-means is host work) and runs exactly `max_iter`
warm-started iterations (tol = 0 never stops early); the time per iteration is the run's wall time, ended by a device synchronise, over `max_iter`.
Warm-up runs first, then the median of `reps` runs; min and max are kept.  A process loads one library, so every library is measured in a child
process of its own (`--lib [label=]path`: further libraries to time with the same script, e.g. one built from another commit; the tree's own comes first).
One JSON document; no GPU, no result.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if not any(os.path.isdir(os.path.join(p, "ladder_latent_data_distribution_modelling_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)

R, K, CENTRES = 8, 50, 12
LEGS = (("persistent", 1000, 100), ("sliced", 20096, 200))                         # (path, samples, timed iterations per run)


def _samples(rng, n):
    c, A = rng.normal(0, 2.0, size=(CENTRES, R)), rng.normal(0, 0.35, size=(CENTRES, R, R))
    idx = rng.integers(0, CENTRES, n)
    return (c[idx] + np.einsum("nij,nj->ni", A[idx], rng.normal(size=(n, R)))).astype(np.float32)


def leg(path, N, max_iter, reps, warmup):
    from ladder_latent_data_distribution_modelling_amd.codes import vbgmm
    assert (N >= vbgmm.SLICED_FIT_MIN_SAMPLES) == (path == "sliced")
    Xd = torch.as_tensor(_samples(np.random.default_rng(N), N)).cuda()
    gm = vbgmm.DeviceBayesianGaussianMixture(n_components=K, covariance_type="full", tol=0.0, max_iter=2, n_init=1, warm_start=True, random_state=7,
                                             weight_concentration_prior_type="dirichlet_distribution", weight_concentration_prior=0.1).fit(Xd)
    start = gm._state.clone()
    gm.max_iter = max_iter
    secs = []
    for r in range(warmup + reps):
        gm._state.copy_(start)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gm.fit(Xd)
        torch.cuda.synchronize()
        if r >= warmup:
            secs.append(time.perf_counter() - t0)
        print("%s run %d: %.4f s" % (path, r, time.perf_counter() - t0), file=sys.stderr, flush=True)
        assert gm.n_iter_ == max_iter and not gm.converged_
    per_it = sorted(1e3 * s / max_iter for s in secs)
    return dict(path=path, n_samples=N, max_iter=max_iter, ms_per_iteration_median=round(statistics.median(per_it), 5),
                ms_per_iteration_min=round(per_it[0], 5), ms_per_iteration_max=round(per_it[-1], 5), run_seconds=[round(s, 5) for s in secs],
                lower_bound=gm.lower_bound_)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vbgmm_fit_time.json"))
    ap.add_argument("--lib", nargs="*", default=[], help="[label=]path of further libladder_hip.so files to time, each in a child process")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:                                                                      # one library (LADDER_HIP_LIB, or the tree's): its legs as one JSON line
        if not torch.cuda.is_available():
            sys.exit("vbgmm_fit_time.py measures on the GPU: none found")
        warnings.simplefilter("ignore")                                              # (every run ends unconverged by construction)
        print(json.dumps(dict(device_name=torch.cuda.get_device_name(0), legs=[leg(path, N, it, a.reps, a.warmup) for path, N, it in LEGS])), flush=True)
        return
    libs = []
    for lib in [None] + a.lib:
        lib, path = (None, None) if lib is None else lib.split("=", 1) if "=" in lib else (lib, lib)
        env = dict(os.environ) if lib is None else dict(os.environ, LADDER_HIP_LIB=os.path.abspath(path))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup)], env=env,
                           stdout=subprocess.PIPE, text=True, timeout=300)
        if p.returncode != 0:
            sys.exit("the measurement of %s failed (exit %d): nothing further is run" % (lib or "the tree's library", p.returncode))
        libs.append(dict(library=lib or "this tree", **json.loads(p.stdout.strip().splitlines()[-1])))
        print(json.dumps(libs[-1]), flush=True)
    doc = dict(what="variational Bayesian mixture fit: ms per iteration, warm-started runs of max_iter iterations, median of %d runs" % a.reps,
               R=R, K=K, centres=CENTRES, prior="dirichlet_distribution", reps=a.reps, libraries=libs)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
