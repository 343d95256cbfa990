"""Time of the wide mixture term and the wide sampler ("The wide form of the mixture"; csrc/mixture_wide.hip, csrc/chol_wide.h, csrc/sample.hip).

    python profiles/tools/gmm_wide_time.py [--out profiles/gmm_wide_time.json] [--reps 5] [--calls 20]

term: ladder_gmm_wide_logprob_fwd_bwd, forward only (dmu = dsd = NULL) and the training call, at (L, B, K, R) = (100, 64, 50, 256), (100, 128, 50, 256)
and (100, 128, 30, 128), on two kinds of input: "separated" -- the synthetic mixture and posteriors of tests/test_gpu_gmm_wide.py, whose
responsibilities are one-hot, so that the backward kernel skips every component but one per 16-sample tile -- and "overlapping" -- K components that
share one covariance with means 0.05 apart, where every responsibility is non-zero and nothing is skipped.  Beside each, in the same process, ONE
ladder_dense_fwd of [S, R] x [R, K*R]: the whitening product of the GEMM form alone, with none of its passes over Y.  The targets: forward only no
slower than that GEMM, the training call no slower than two.
prepare / sampler: ladder_gmm_wide_prepare, ladder_mixture_sample_wide_prepare and 50 000 Philox samples at K = 50, R = 256.
HIP events around `calls` back-to-back calls, one warm-up run, the median of `reps` runs.  One JSON document.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if not any(os.path.isdir(os.path.join(p, "ladder_latent_data_distribution_modelling_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)

SHAPES = [(100, 64, 50, 256), (100, 128, 50, 256), (100, 128, 30, 128)]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def timed(fn, calls, reps):
    """-> microseconds per call: median / min / max over `reps` runs of `calls` calls, after one warm-up run"""
    us = []
    for r in range(1 + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        if r:
            us.append(a.elapsed_time(b) * 1e3 / calls)
    return dict(us_median=round(statistics.median(us), 1), us_min=round(min(us), 1), us_max=round(max(us), 1))


def inputs(kind, L_, B, K, R):
    from oracle import ladder_oracle as O
    rng = np.random.default_rng(K * 7 + R)
    if kind == "separated":
        gm = O.synthetic_gm(dict(n_mixtures=K, representation_size=R), rng)
        mu, sd = rng.standard_normal((B, R)) * 1.5, 0.05 + rng.random((B, R))
    else:
        one = O.synthetic_gm(dict(n_mixtures=1, representation_size=R), rng)
        m0 = one["means"][0]
        gm = dict(weights=rng.dirichlet(np.ones(K)), means=m0 + 0.05 * rng.standard_normal((K, R)), covs=np.repeat(one["covs"], K, 0))
        mu, sd = m0 + 0.05 * rng.standard_normal((B, R)), 0.05 + 0.2 * rng.random((B, R))
    eps = rng.standard_normal((L_, B, R))
    return gm, mu, sd, eps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gmm_wide_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gmm_wide_time.py measures on the GPU: none found")
    from oracle import ladder_oracle as O
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.engine import Ctx
    st = Ctx("cuda:0").stream
    rows = []
    for L_, B, K, R in SHAPES:
        S = L_ * B
        # the whitening GEMM of the dense form on its own: T [S, R] x Bmat [R, K*R] -> Y [S, K*R]
        T, Bm, bias, Y = torch.randn(S, R, device="cuda"), torch.randn(R, K * R, device="cuda"), torch.zeros(K * R, device="cuda"), torch.empty(S, K * R, device="cuda")
        gws = torch.empty(max(L.query("ladder_igemm_fwd_workspace_bytes", S, R, K * R), 256), dtype=torch.uint8, device="cuda")
        gemm = timed(lambda: L.call("ladder_dense_fwd", p(T), p(Bm), p(bias), p(Y), S, R, K * R, 0, p(gws), gws.numel(), st), a.calls, a.reps)
        del T, Bm, bias, Y, gws
        for kind in ("separated", "overlapping"):
            gm, mu, sd, eps = inputs(kind, L_, B, K, R)
            params = torch.zeros(L.query("ladder_gmm_wide_param_bytes", K, R), dtype=torch.uint8, device="cuda")
            pws = torch.empty(L.query("ladder_gmm_wide_prepare_workspace_bytes", K, R), dtype=torch.uint8, device="cuda")
            wd, md, cd = dev(gm["weights"]), dev(gm["means"]), dev(gm["covs"])
            L.call("ladder_gmm_wide_prepare", p(wd), p(md), p(cd), K, R, p(params), p(pws), pws.numel(), st)
            assert int(params[:4].view(torch.int32).item()) == -1
            mud, sdd, epsd = dev(mu), dev(sd), dev(eps)
            out, dmu, dsd = torch.empty(1, device="cuda"), torch.empty(B, R, device="cuda"), torch.empty(B, R, device="cuda")
            ws = torch.empty(L.query("ladder_gmm_wide_workspace_bytes", L_, B, R, K), dtype=torch.uint8, device="cuda")
            call = lambda g: L.call("ladder_gmm_wide_logprob_fwd_bwd", p(mud), p(sdd), p(epsd), p(params), L_, B, R, K, p(out), p(dmu) if g else None,
                                    p(dsd) if g else None, p(ws), ws.numel(), st)
            fwd, train = timed(lambda: call(False), a.calls, a.reps), timed(lambda: call(True), a.calls, a.reps)
            nb = R // 16
            row = dict(L=L_, B=B, K=K, R=R, S=S, inputs=kind, sum_logp=out.item(), forward_only=fwd, training=train, whitening_gemm=gemm,
                       forward_over_gemm=round(fwd["us_median"] / gemm["us_median"], 3), training_over_two_gemms=round(train["us_median"] / (2 * gemm["us_median"]), 3),
                       forward_tflops=round(2.0 * S * K * (nb * (nb + 1) // 2) * 256 / fwd["us_median"] * 1e-6, 2),
                       gemm_tflops=round(2.0 * S * K * R * R / gemm["us_median"] * 1e-6, 2),
                       workspace_bytes=ws.numel(), whitened_product_bytes=4 * S * K * R)
            rows.append(row)
            print(json.dumps(row), flush=True)
    # prepare and sampler at the shipped K and R
    K, R, n = 50, 256, 50000
    gm = O.synthetic_gm(dict(n_mixtures=K, representation_size=R), np.random.default_rng(K * 7 + R))
    wd, md, cd = dev(gm["weights"]), dev(gm["means"]), dev(gm["covs"])
    params = torch.zeros(L.query("ladder_gmm_wide_param_bytes", K, R), dtype=torch.uint8, device="cuda")
    pws = torch.empty(L.query("ladder_gmm_wide_prepare_workspace_bytes", K, R), dtype=torch.uint8, device="cuda")
    prep = timed(lambda: L.call("ladder_gmm_wide_prepare", p(wd), p(md), p(cd), K, R, p(params), p(pws), pws.numel(), st), 2, a.reps)
    sparams = torch.zeros(L.query("ladder_mixture_sample_wide_param_bytes", K, R), dtype=torch.uint8, device="cuda")
    sws = torch.empty(L.query("ladder_mixture_sample_wide_prepare_workspace_bytes", K, R), dtype=torch.uint8, device="cuda")
    sprep = timed(lambda: L.call("ladder_mixture_sample_wide_prepare", p(wd), p(md), p(cd), K, R, p(sparams), p(sws), sws.numel(), st), 2, a.reps)
    assert int(sparams[:4].view(torch.int32).item()) == -1
    lat, comp = torch.empty(n, R, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    samp = timed(lambda: L.call("ladder_mixture_sample_wide", p(sparams), K, R, n, 0, None, None, 7, 0, p(lat), p(comp), st), 4, a.reps)
    once = dict(K=K, R=R, mixture_prepare=prep, sampler_prepare=sprep, samples=n, sampler=samp,
                sampler_gb_per_s=round(n * (R * (R + 1) // 2) * 4 / samp["us_median"] * 1e-3, 1))
    print(json.dumps(once), flush=True)
    doc = dict(what="the wide mixture term (forward only / training call) beside one strict-fp32 ladder_dense_fwd of [S, R] x [R, K*R], and the prepare / "
                    "sampler calls at K = 50, R = 256: HIP events around %d back-to-back calls (prepare: 2, sampler: 4), one warm-up run, median of %d runs"
                    % (a.calls, a.reps),
               calls=a.calls, reps=a.reps, device_name=torch.cuda.get_device_name(0), term=rows, once_per_fit=once)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
