"""Per-iteration time of the EM fit of the "GMM" prior on a WIDE code: the device fit (codes/emgmm.py -> csrc/emgmm_wide.hip)
with its E-step, statistics and M-step launches separated, against sklearn.mixture.GaussianMixture on the same samples on the host, at the sample
counts of the per-epoch fit (2 048) and of the accurate fit (20 032) of the reference's shipped CelebA config (code_size 256, n_mixtures 50), and at
R = 128.

    python profiles/tools/emgmm_wide_fit_time.py [--out profiles/emgmm_wide_time.json] [--trace-dir DIR] [--shapes N,K,R ...]

The parent process never opens the GPU.  Per shape it starts, one after the other,
  * a child (`--child N K R`) that runs a cold fit of two iterations (not timed: its k-means is host work) and then, from that SAME fitted state every
    time, exactly MAX_ITER = 20 warm-started EM iterations (tol = 0 never stops early): wall time ended by a device synchronise, over 20; warm-up runs
    first, then the median of `reps` runs;
  * the same child with one timed run under `rocprofv3 --kernel-trace` (a run of its own: tracing slows the host), from whose kernel records the parent
    takes the MEDIAN duration of each kernel -- the E-step (emw_estep_kernel + emw_rows_kernel), the statistics (emw_stats_kernel + fit_reduce_kernel)
    and the M-step (emw_mstep_kernel + emgmm_finish_kernel) -- and the issued float64 rate: the multiply-adds the MFMA instructions of a launch
    execute, counted from the shapes below (zero blocks that are skipped are not counted; padding rows of the last slice or split are), times two,
    over the kernel's time;
  * and runs the host leg itself: GaussianMixture from the same k-means labels, a cold fit of one iteration, then `host_iters` warm-started iterations
    timed once, with the threads the environment gives it (OMP_NUM_THREADS; recorded).
One JSON document; no GPU, no result.
"""
import argparse
import glob
import json
import os
import sqlite3
import statistics
import subprocess
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if not any(os.path.isdir(os.path.join(p, "ladder_latent_data_distribution_modelling_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)

SPREAD, MAX_ITER = 0.3, 20
KW = dict(covariance_type="full", tol=0.0, reg_covar=1e-6, n_init=1, warm_start=True, random_state=7)
PHASES = {"estep": ("emw_estep_kernel", "emw_rows_kernel"), "statistics": ("emw_stats_kernel", "fit_reduce_kernel"),
          "mstep": ("emw_mstep_kernel", "emgmm_finish_kernel")}


def samples(N, K, R):
    """N fp32 samples of a K-component mixture in R dimensions, from a seed: the same in every process."""
    rng = np.random.default_rng(11)
    c, A = rng.normal(0, SPREAD, (K, R)), 0.5 * np.eye(R)[None] + rng.normal(0, 0.5 / np.sqrt(R), (K, R, R))
    i = rng.integers(0, K, N)
    out = np.empty((N, R), np.float32)
    for k in range(K):                                                               # (component by component: no [N, R, R] gather)
        sel = np.flatnonzero(i == k)
        out[sel] = c[k] + rng.normal(size=(len(sel), R)) @ A[k].T
    return out


def issued_fma(N, K, R):
    """Multiply-adds of the v_mfma_f64_16x16x4_f64 instructions one E-step / one statistics launch executes (1024 each)."""
    nb, slices = R // 16, (N + 63) // 64
    rows = max(128, (N + 31) // 32)
    rows = (rows + 3) // 4 * 4
    steps = sum((min(N, r0 + rows) - r0 + 3) // 4 for r0 in range(0, N, rows))
    return dict(estep=slices * K * 4 * 4 * (nb * (nb + 1) // 2) * 1024, statistics=K * steps * (nb * (nb + 1) // 2 + nb) * 1024)


def child(N, K, R, reps, warmup):
    import torch
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    if not torch.cuda.is_available():
        sys.exit("emgmm_wide_fit_time.py measures on the GPU: none found")
    warnings.simplefilter("ignore")                                                  # (every run ends unconverged by construction)
    Xd = torch.as_tensor(samples(N, K, R)).cuda()
    gm = DeviceGaussianMixture(n_components=K, max_iter=2, **KW).fit(Xd)
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
    cov = gm.covariances_
    print(json.dumps(dict(run_seconds=secs, lower_bound=gm.lower_bound_, cov_checksum=float(np.abs(cov).sum()), cov_max=float(np.abs(cov).max()))))


def _run_child(N, K, R, reps, warmup, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child", str(N), str(K), str(R), "--reps", str(reps), "--warmup", str(warmup)]
    p = subprocess.run(["timeout", "-k", "10", "300"] + cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit("child failed (%d): %s" % (p.returncode, " ".join(cmd)))
    return json.loads(p.stdout.strip().splitlines()[-1])


def kernel_medians(trace_dir):
    """-> {kernel name without namespace and arguments: (median ns, launches)} over every rocpd database under trace_dir."""
    durs = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True):
        for name, d in sqlite3.connect(path).execute("select name, duration from kernels"):
            durs.setdefault(name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0], []).append(d)
    return {n: (statistics.median(d), len(d)) for n, d in durs.items()}


def host_leg(X, K, iters):
    from sklearn.mixture import GaussianMixture
    gm = GaussianMixture(n_components=K, max_iter=1, **KW).fit(X)
    gm.max_iter = iters
    t0 = time.perf_counter()
    gm.fit(X)
    dt = time.perf_counter() - t0
    assert gm.n_iter_ == iters
    return dict(iterations=iters, ms_per_iteration=round(1e3 * dt / iters, 2), run_seconds=round(dt, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "emgmm_wide_time.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "profiles", "out", "emgmm_wide_trace"))
    ap.add_argument("--shapes", nargs="+", default=["2048,50,256", "20032,50,256", "2048,50,128", "20032,50,128"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--child", nargs=3, type=int, metavar=("N", "K", "R"))
    a = ap.parse_args()
    if a.child:
        return child(*a.child, a.reps, a.warmup)
    warnings.simplefilter("ignore")
    rows = []
    for shape in a.shapes:
        N, K, R = (int(v) for v in shape.split(","))
        dev = _run_child(N, K, R, a.reps, a.warmup)
        per_it = sorted(1e3 * s / MAX_ITER for s in dev["run_seconds"])
        tdir = os.path.join(a.trace_dir, "%dx%dx%d" % (N, K, R))
        _run_child(N, K, R, 1, 1, prefix=("rocprofv3", "--kernel-trace", "-d", tdir, "--"))
        med, fma = kernel_medians(tdir), issued_fma(N, K, R)
        phases = {}
        for phase, names in PHASES.items():
            kernels = {n: dict(median_us=round(med[n][0] / 1e3, 2), launches=med[n][1]) for n in names}
            phases[phase] = dict(kernels=kernels, us_per_iteration=round(sum(k["median_us"] for k in kernels.values()), 2))
            if phase in fma:
                phases[phase]["issued_fma"] = fma[phase]
                phases[phase]["issued_f64_tflops"] = round(2 * fma[phase] / (med[names[0]][0] * 1e-9) / 1e12, 2)
        kernel_ms = sum(p["us_per_iteration"] for p in phases.values()) / 1e3
        host = host_leg(samples(N, K, R).astype(np.float64), K, a.host_iters)
        row = dict(n_samples=N, K=K, R=R,
                   device=dict(ms_per_iteration_median=round(statistics.median(per_it), 4), ms_per_iteration_min=round(per_it[0], 4),
                               ms_per_iteration_max=round(per_it[-1], 4), kernel_ms_per_iteration=round(kernel_ms, 4), lower_bound=dev["lower_bound"]),
                   phases=phases, host_sklearn=host, host_over_device=round(host["ms_per_iteration"] / statistics.median(per_it), 1))
        rows.append(row)
        print(json.dumps(row), flush=True)
    import sklearn
    import torch
    doc = dict(what="EM fit of the GMM prior on a wide code: ms per EM iteration (%d warm-started iterations per run, median of %d runs), per-kernel median "
                    "times from a rocprofv3 kernel trace of one such run, sklearn on the host on the same samples" % (MAX_ITER, a.reps),
               spread=SPREAD, max_iter=MAX_ITER, reps=a.reps, torch=torch.__version__, sklearn=sklearn.__version__,
               host_threads=os.environ.get("OMP_NUM_THREADS"), rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
