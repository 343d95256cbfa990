"""Wall time of the k-means of a cold WIDE mixture fit: the host leg (device -> host copy, sklearn.cluster.KMeans, labels back -- what every cold fit of
the "GMM" prior beyond 64 dimensions did before csrc/kmeans_wide.hip) against the device leg (codes/kmeans.py -> csrc/kmeans_wide.hip), at the sample
counts of the per-epoch fit (2 048) and of the accurate fit (20 032) of the reference's shipped CelebA config (code_size 256, n_mixtures 50): the
k-means alone, the cold DeviceGaussianMixture fit with kmeans_backend "sklearn" against "hip_wide", and the device time of every entry point of one
fit ("K-means on the device").

    python profiles/tools/kmeans_wide_fit_time.py [--out profiles/kmeans_wide_fit_time.json] [--reps 5]

Both legs get the same samples and the same `random_state`; the tool records whether they produced the same labels and iteration counts (faster and
different is not faster).  Every timed run is a whole call ended by a device synchronise; one warm-up run per leg first (code objects, allocator, BLAS
threads), then the median of `reps` runs with min and max.  The entry-point times are device time between events around each call of one fit, summed
per entry point.  The host leg uses the threads the environment gives it (OMP_NUM_THREADS; recorded, not changed).
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

K, R, SEED, SPREAD = 50, 256, 7, 1.0
SAMPLE_COUNTS = (2048, 20032)
EM = dict(covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=100, n_init=1)


def samples(N):
    """N fp32 samples of a K-component mixture in R dimensions, from a seed (the generator of profiles/tools/emgmm_wide_fit_time.py)."""
    rng = np.random.default_rng(11)
    c, A = rng.normal(0, SPREAD, (K, R)), 0.5 * np.eye(R)[None] + rng.normal(0, 0.5 / np.sqrt(R), (K, R, R))
    i = rng.integers(0, K, N)
    out = np.empty((N, R), np.float32)
    for k in range(K):                                                               # (component by component: no [N, R, R] gather)
        sel = np.flatnonzero(i == k)
        out[sel] = c[k] + rng.normal(size=(len(sel), R)) @ A[k].T
    return out


def timed(fn, reps, warmup=1):
    secs, out = [], None
    for r in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if r >= warmup:
            secs.append(time.perf_counter() - t0)
    secs.sort()
    return dict(ms_median=round(1e3 * statistics.median(secs), 3), ms_min=round(1e3 * secs[0], 3), ms_max=round(1e3 * secs[-1], 3)), out


def verdict(row):
    """The requirement: the device leg's median below the host leg's minimum."""
    row["sklearn_over_hip_wide"] = round(row["sklearn"]["ms_median"] / row["hip_wide"]["ms_median"], 2)
    row["device_median_below_host_min"] = row["hip_wide"]["ms_median"] < row["sklearn"]["ms_min"]


def kmeans_row(Xd, reps):
    from sklearn.cluster import KMeans
    from ladder_latent_data_distribution_modelling_amd.codes.kmeans import DeviceKMeans
    fits = {}

    def host():                                                                      # what mixture_fit.initial_labels_for does around the labeller
        fits["sk"] = KMeans(n_clusters=K, n_init=1, random_state=np.random.RandomState(SEED)).fit(Xd.cpu().numpy().astype(np.float64))
        return torch.as_tensor(fits["sk"].labels_.astype(np.int32)).to(Xd.device)

    def dev():
        return DeviceKMeans(n_clusters=K, random_state=np.random.RandomState(SEED), device=Xd.device).fit(Xd)

    row = dict(kmeans_alone=True, n_samples=Xd.shape[0], R=R, K=K)
    row["sklearn"], lab = timed(host, reps)
    row["hip_wide"], km = timed(dev, reps)
    row["sklearn"]["n_iter"], row["hip_wide"]["n_iter"] = int(fits["sk"].n_iter_), km.n_iter_
    row["label_mismatches"] = int((lab != km.labels_dev).sum())
    row["same_n_iter"] = int(fits["sk"].n_iter_) == km.n_iter_
    verdict(row)
    row["entry_points_ms"] = entry_point_times(Xd, km.n_iter_)
    return row


def mixture_row(Xd, reps):
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.codes.mixture_fit import OneRank
    row = dict(fit="DeviceGaussianMixture, cold", n_samples=Xd.shape[0], R=R, K=K)
    fits, labels = {}, {}
    for backend in ("sklearn", "hip_wide"):
        make = lambda: DeviceGaussianMixture(n_components=K, random_state=SEED, kmeans_backend=backend, **EM)
        row[backend], fits[backend] = timed(lambda: make().fit(Xd), reps)
        row[backend]["n_iter"], row[backend]["converged"] = fits[backend].n_iter_, bool(fits[backend].converged_)
        labels[backend] = make()._initial_labels(Xd, OneRank(), np.random.RandomState(SEED))
    a, b = fits["sklearn"], fits["hip_wide"]
    row["label_mismatches"] = int((labels["sklearn"] != labels["hip_wide"]).sum())
    row["same_n_iter"] = a.n_iter_ == b.n_iter_
    row["covariance_max_rel_difference"] = float(np.abs(a.covariances_ - b.covariances_).max() / np.abs(a.covariances_).max())
    verdict(row)
    return row


def entry_point_times(Xd, n_iter):
    """One fit with an event pair around every entry-point call: device ms per entry point (sum over the fit) and per call."""
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.codes.mixture_fit import kmeans_draws
    lib = L.load()
    Nn = Xd.shape[0]
    st = torch.cuda.current_stream().cuda_stream
    state = torch.zeros(lib.ladder_kmeans_wide_state_doubles(K, R), dtype=torch.float64, device=Xd.device)
    ws = torch.empty(lib.ladder_kmeans_wide_workspace_bytes(Nn, K, R), dtype=torch.uint8, device=Xd.device)
    labels = torch.empty(Nn, dtype=torch.int32, device=Xd.device)
    first, u = kmeans_draws(np.random.RandomState(SEED), Nn, K)
    draws = torch.as_tensor(np.concatenate([[float(first)], u.ravel()])).to(Xd.device)
    spans = []

    def span(what, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        assert fn() == 0
        b.record()
        spans.append((what, a, b))

    span("seed", lambda: lib.ladder_kmeans_wide_seed(Xd.data_ptr(), Nn, K, R, draws.data_ptr(), state.data_ptr(), ws.data_ptr(), ws.numel(), st))
    for it in range(1, n_iter + 2):
        span("assign", lambda: lib.ladder_kmeans_wide_assign(Xd.data_ptr(), Nn, K, R, it, state.data_ptr(), labels.data_ptr(), ws.data_ptr(),
                                                             ws.numel(), st))
        span("update", lambda: lib.ladder_kmeans_wide_update(Xd.data_ptr(), Nn, K, R, labels.data_ptr(), state.data_ptr(), 1e-4, 300, it,
                                                             ws.data_ptr(), ws.numel(), st))
    torch.cuda.synchronize()
    out = {}
    for what in ("seed", "assign", "update"):
        ms = [a.elapsed_time(b) for w, a, b in spans if w == what]
        out[what] = dict(calls=len(ms), total=round(sum(ms), 3), per_call_median=round(statistics.median(ms), 4))
    total = sum(out[w]["total"] for w in ("seed", "assign", "update"))
    for what in ("seed", "assign", "update"):
        out[what]["share"] = round(out[what]["total"] / total, 3)
    out["n_iter_of_this_fit"] = int(state[-3].item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_wide_fit_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kmeans_wide_fit_time.py measures on the GPU: none found")
    warnings.simplefilter("ignore")
    rows = []
    for N in SAMPLE_COUNTS:
        Xd = torch.as_tensor(samples(N)).cuda()
        for make_row in (kmeans_row, mixture_row):
            rows.append(make_row(Xd, a.reps))
            print(json.dumps(rows[-1]), flush=True)
    import sklearn
    doc = dict(what="k-means alone and cold EM fits of the GMM prior on a wide code, host k-means (sklearn) vs device k-means (hip_wide): wall ms per "
                    "call, median of %d runs after one warm-up" % a.reps,
               reps=a.reps, spread=SPREAD, device_name=torch.cuda.get_device_name(0), torch=torch.__version__, sklearn=sklearn.__version__,
               host_threads=os.environ.get("OMP_NUM_THREADS"), rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
