"""Wall time of a COLD mixture fit with the k-means labels from the host (kmeans_backend="sklearn": gather, device -> host copy, sklearn.cluster.KMeans,
labels back -- what every cold fit did before csrc/kmeans.hip) against the device k-means (kmeans_backend="hip"), at the shapes of the accurate fits:
DeviceGaussianMixture on 20 096 x 64, K = 50 and DeviceBayesianGaussianMixture on 20 096 x 8, K = 50; then the k-means portion alone and the time of its
entry points ("K-means on the device").

    python profiles/tools/kmeans_fit_time.py [--out profiles/kmeans_fit_time.json] [--reps 5]

Both legs get the same samples and the same `random_state`; the tool records whether they produced the same labels and iteration counts (faster and
different is not faster).  Every timed run is a whole call ended by a device synchronise; one warm-up run per leg first (code objects, allocator, BLAS
threads), then the median of `reps` runs with min and max.  The entry-point times are device time between events around each call of one fit, summed per
entry point.  The host leg uses the threads the environment gives it (OMP_NUM_THREADS; recorded).
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

N, K, SEED = 20096, 50, 7


def samples(R, centres, spread, seed):
    rng = np.random.default_rng(seed)
    c, A = rng.normal(0, spread, (centres, R)), 0.5 * np.eye(R)[None] + rng.normal(0, 0.5 / np.sqrt(R), (centres, R, R))
    i = rng.integers(0, centres, N)
    return (c[i] + np.einsum("nij,nj->ni", A[i], rng.normal(size=(N, R)))).astype(np.float32)


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


def mixture_rows(name, make, Xd, reps):
    row = dict(fit=name, n_samples=N, R=Xd.shape[1], K=K)
    fits = {}
    for backend in ("sklearn", "hip"):
        row[backend], fits[backend] = timed(lambda: make(backend).fit(Xd), reps)
        row[backend]["n_iter"] = fits[backend].n_iter_
    a, b = fits["sklearn"], fits["hip"]
    row["same_n_iter"] = a.n_iter_ == b.n_iter_
    row["covariance_max_rel_difference"] = float(np.abs(a.covariances_ - b.covariances_).max() / np.abs(a.covariances_).max())
    row["sklearn_over_hip"] = round(row["sklearn"]["ms_median"] / row["hip"]["ms_median"], 2)
    return row


def kmeans_rows(Xd, reps):
    from sklearn.cluster import KMeans
    from ladder_latent_data_distribution_modelling_amd.codes.kmeans import DeviceKMeans

    def host():                                                                      # what mixture_fit.initial_labels_for does around the labeller
        lab = KMeans(n_clusters=K, n_init=1, random_state=np.random.RandomState(SEED)).fit(Xd.cpu().numpy().astype(np.float64)).labels_
        return torch.as_tensor(lab.astype(np.int32)).to(Xd.device)

    def dev():
        return DeviceKMeans(n_clusters=K, random_state=np.random.RandomState(SEED), device=Xd.device).fit(Xd)

    row = dict(kmeans_alone=True, n_samples=N, R=Xd.shape[1], K=K)
    row["sklearn"], lab = timed(host, reps)
    row["hip"], km = timed(dev, reps)
    row["hip"]["n_iter"] = km.n_iter_
    row["label_mismatches"] = int((lab != km.labels_dev).sum())
    row["sklearn_over_hip"] = round(row["sklearn"]["ms_median"] / row["hip"]["ms_median"], 2)
    row["entry_points_ms"] = entry_point_times(Xd, km.n_iter_)
    return row


def entry_point_times(Xd, n_iter):
    """One fit with an event pair around every entry-point call: device ms per entry point (sum over the fit) and per call."""
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.codes.mixture_fit import kmeans_draws
    lib = L.load()
    Nn, R = Xd.shape
    st = torch.cuda.current_stream().cuda_stream
    state = torch.zeros(lib.ladder_kmeans_state_doubles(K, R), dtype=torch.float64, device=Xd.device)
    ws = torch.empty(lib.ladder_kmeans_workspace_bytes(Nn, K, R), dtype=torch.uint8, device=Xd.device)
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

    span("seed", lambda: lib.ladder_kmeans_seed(Xd.data_ptr(), Nn, K, R, draws.data_ptr(), state.data_ptr(), ws.data_ptr(), ws.numel(), st))
    for it in range(1, n_iter + 2):
        span("assign", lambda: lib.ladder_kmeans_assign(Xd.data_ptr(), Nn, K, R, it, state.data_ptr(), labels.data_ptr(), ws.data_ptr(), ws.numel(), st))
        span("update", lambda: lib.ladder_kmeans_update(Xd.data_ptr(), Nn, K, R, labels.data_ptr(), state.data_ptr(), 1e-4, 300, it, ws.data_ptr(),
                                                        ws.numel(), st))
    torch.cuda.synchronize()
    out = {}
    for what in ("seed", "assign", "update"):
        ms = [a.elapsed_time(b) for w, a, b in spans if w == what]
        out[what] = dict(calls=len(ms), total=round(sum(ms), 3), per_call_median=round(statistics.median(ms), 4))
    out["n_iter_of_this_fit"] = int(state[-3].item())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_fit_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kmeans_fit_time.py measures on the GPU: none found")
    warnings.simplefilter("ignore")
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.codes.vbgmm import DeviceBayesianGaussianMixture
    X64, X8 = torch.as_tensor(samples(64, 50, 0.3, 11)).cuda(), torch.as_tensor(samples(8, 50, 1.0, 12)).cuda()
    rows = []
    rows.append(mixture_rows("DeviceGaussianMixture", lambda be: DeviceGaussianMixture(
        n_components=K, max_iter=2000, n_init=1, random_state=SEED, kmeans_backend=be), X64, a.reps))
    print(json.dumps(rows[-1]), flush=True)
    rows.append(mixture_rows("DeviceBayesianGaussianMixture", lambda be: DeviceBayesianGaussianMixture(
        n_components=K, max_iter=2000, n_init=1, weight_concentration_prior_type="dirichlet_process", weight_concentration_prior=0.1,
        random_state=SEED, kmeans_backend=be), X8, a.reps))
    print(json.dumps(rows[-1]), flush=True)
    for Xd in (X64, X8):
        rows.append(kmeans_rows(Xd, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    import sklearn
    doc = dict(what="cold mixture fits and k-means alone, host k-means (sklearn) vs device k-means (hip): wall ms per call, median of %d runs" % a.reps,
               reps=a.reps, device_name=torch.cuda.get_device_name(0), sklearn=sklearn.__version__, host_threads=os.environ.get("OMP_NUM_THREADS"),
               rows=rows)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
