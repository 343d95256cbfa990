"""Every output of the mixture entry points on fixed seeded inputs, written to one .npz -- for whichever library LADDER_HIP_LIB names.

    LADDER_HIP_LIB=/path/to/libladder_hip.so python profiles/mixture_outputs.py out.npz
    python profiles/mixture_outputs.py --compare a.npz b.npz        # table of np.array_equal per array (NaN positions must match too)

Run it once per library, each in a fresh process, and compare: two builds whose mixture kernels compute the same thing give equal arrays
bit for bit.  The shapes reach every code path at its smallest size: K = 64 / 65 straddles the register-kernel boundary, L is no multiple
of the 4 wavefronts, K = 130 gives three component chunks, n = 7 is no multiple of the 4 points of a workgroup, and the K = 130, R = 8
mixture (5 850 floats) does not fit the 4 096-float LDS budget of ladder_slp_optimise.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PACKED = [(5, 1, 7, 3), (30, 2, 9, 5), (64, 8, 5, 4), (65, 3, 5, 4), (130, 8, 6, 2)]       # (K, R, L, B)
N_ROWS = 7
# the diagonal mixture (VampPrior).  Wide term (L, B, Z, K): S = 15 under one workgroup with lanes 20..63 off; two component chunks of 16, the second
# padded; two chunks of 64 components (Kp = 80); an odd L.  Rows (n, Z, K): rows padded to 8; a second workgroup with one live row and two component
# chunks; one row, one component, the widest code; ld = 252 and three chunks.
DIAG_WIDE = [(3, 5, 80, 1), (5, 7, 80, 17), (2, 9, 256, 65), (7, 3, 96, 50)]
DIAG_ROWS = [(7, 5, 3), (17, 40, 65), (1, 256, 1), (5, 250, 130)]


def mixture(K, R, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 0.3, (K, R, R))
    return rng.dirichlet(np.ones(K)), rng.normal(0, 1.5, (K, R)), A @ A.transpose(0, 2, 1) / R + 0.05 * np.eye(R)


def compare(a, b):
    a, b = np.load(a), np.load(b)
    assert sorted(a.files) == sorted(b.files), (sorted(set(a.files) ^ set(b.files)))
    bad = 0
    print("| array | shape | NaNs | equal |\n|---|---|---|---|")
    for k in sorted(set(a.files) - {"library"}):
        eq = a[k].shape == b[k].shape and np.array_equal(a[k], b[k], equal_nan=True)
        bad += not eq
        print("| %s | %s | %d | %s |" % (k, "x".join(map(str, a[k].shape)) or "scalar", int(np.isnan(a[k].astype(np.float64)).sum()), "yes" if eq else "NO"))
    print("%d arrays, %d differ (%s vs %s)" % (len(a.files) - 1, bad, a["library"], b["library"]))
    return 1 if bad else 0


def main(out_path):
    import torch
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.engine import Ctx, LadderEngine
    from ladder_latent_data_distribution_modelling_amd.codes.interpolation import SLPInterpolator
    from ladder_latent_data_distribution_modelling_amd.demo.demo_tools import MixturePrior
    from ladder_latent_data_distribution_modelling_amd.mixture import DeviceMixture
    ctx = Ctx("cuda:0")
    st = ctx.stream
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    p = lambda t: None if t is None else t.data_ptr()
    host = lambda t: t.cpu().numpy()
    out = {"library": np.array(os.environ.get("LADDER_HIP_LIB", L.LIB_PATH))}

    def inputs(K, R, Lmc, B, n, seed):
        rng = np.random.default_rng(seed)
        return (dev(rng.standard_normal((B, R)) * 2), dev(0.05 + rng.random((B, R))), dev(rng.standard_normal((Lmc, B, R))),
                dev(rng.standard_normal((n, R)) * 2))

    # ---- packed form: prepare, fwd_bwd, rows
    packed = {}
    for K, R, Lmc, B in PACKED:
        tag = "packed_K%d_R%d" % (K, R)
        w, m, c = (dev(a) for a in mixture(K, R, 100 + K))
        buf = torch.empty(K * L.query("ladder_gmm_packed_stride", R), device="cuda")
        L.call("ladder_gmm_prepare", p(w), p(m), p(c), K, R, p(buf), st)
        mu, sd, eps, t = inputs(K, R, Lmc, B, N_ROWS, 200 + K)
        s, dmu, dsd, lp = torch.empty(1, device="cuda"), torch.empty(B, R, device="cuda"), torch.empty(B, R, device="cuda"), torch.empty(N_ROWS, device="cuda")
        ws = torch.empty(L.query("ladder_gmm_workspace_bytes", Lmc, B), dtype=torch.uint8, device="cuda")
        L.call("ladder_gmm_logprob_fwd_bwd", p(mu), p(sd), p(eps), p(buf), Lmc, B, R, K, p(s), p(dmu), p(dsd), p(ws), ws.numel(), st)
        L.call("ladder_gmm_logprob_rows", p(t), p(buf), N_ROWS, R, K, p(lp), st)
        torch.cuda.synchronize()
        out.update({tag + "_prepared": host(buf), tag + "_sum": host(s), tag + "_dmu": host(dmu), tag + "_dsd": host(dsd), tag + "_rows": host(lp)})
        packed[(K, R)] = buf

    # ---- ladder_slp_optimise: one launch of 12 iterations, and 6 + 6 chained through the state
    for K, R, n_step in ((30, 2, 5), (130, 8, 6)):
        P, n_iter = 3, 12
        rng = np.random.default_rng(300 + K)
        s_d, e_d = dev(rng.normal(0, 1.5, (P, R))), dev(rng.normal(0, 1.5, (P, R)))
        init = np.stack([np.linspace(a, b, n_step + 1, endpoint=False)[1:] for a, b in zip(host(s_d), host(e_d))])
        for mode, cuts in (("once", (12,)), ("chained", (6, 6))):
            pts = dev(init)
            state = torch.empty(L.query("ladder_slp_state_bytes", P, n_step, R) // 8, dtype=torch.float64, device="cuda")
            recs, t0 = [], 0
            for k in cuts:
                rec = torch.empty(P, k, 4, dtype=torch.float64, device="cuda")
                L.call("ladder_slp_optimise", p(s_d), p(e_d), p(pts), p(packed[(K, R)]), K, R, P, n_step, k, t0, 1e-2, 0.9, 0.95, 1e-8, 1.0, 10.0, 100.0,
                       p(state), p(rec), st)
                recs.append(rec)
                t0 += k
            torch.cuda.synchronize()
            tag = "slp_K%d_R%d_%s" % (K, R, mode)
            out.update({tag + "_pts": host(pts), tag + "_state": host(state), tag + "_record": host(torch.cat(recs, 1))})
            assert t0 == n_iter

    # ---- dense form (file move + Python dispatch)
    K, R, Lmc, B = 7, 12, 3, 5
    w, m, c = (dev(a) for a in mixture(K, R, 107))
    buf = torch.empty(L.query("ladder_gmm_dense_param_floats", K, R), device="cuda")
    L.call("ladder_gmm_prepare_dense", p(w), p(m), p(c), K, R, p(buf), st)
    mu, sd, eps, t = inputs(K, R, Lmc, B, N_ROWS, 207)
    s, s2, dmu, dsd, lp = (torch.empty(1, device="cuda"), torch.empty(1, device="cuda"), torch.empty(B, R, device="cuda"), torch.empty(B, R, device="cuda"),
                           torch.empty(N_ROWS, device="cuda"))
    ws = torch.empty(max(L.query("ladder_gmm_dense_workspace_bytes", Lmc, B, R, K), L.query("ladder_gmm_dense_workspace_bytes", 1, N_ROWS, R, K)),
                     dtype=torch.uint8, device="cuda")
    L.call("ladder_gmm_dense_logprob_fwd_bwd", p(mu), p(sd), p(eps), p(buf), Lmc, B, R, K, p(s), p(dmu), p(dsd), p(ws), ws.numel(), st)
    L.call("ladder_gmm_dense_logprob_fwd_bwd", p(mu), p(sd), p(eps), p(buf), Lmc, B, R, K, p(s2), None, None, p(ws), ws.numel(), st)
    L.call("ladder_gmm_dense_logprob_rows", p(t), p(buf), N_ROWS, R, K, p(lp), p(ws), ws.numel(), st)
    torch.cuda.synchronize()
    out.update(dense_prepared=host(buf), dense_sum=host(s), dense_sum_fwd_only=host(s2), dense_dmu=host(dmu), dense_dsd=host(dsd), dense_rows=host(lp))

    # ---- VampPrior term (file move)
    K, Z, Lmc, B = 10, 8, 7, 5
    rng = np.random.default_rng(400)
    a = [dev(v) for v in (rng.standard_normal((B, Z)) * 1.2, 0.1 + rng.random((B, Z)), rng.standard_normal((Lmc, B, Z)), rng.standard_normal((K, Z)),
                          0.3 + rng.random((K, Z)))]
    s, dmu, dsd, dcm, dcs = (torch.empty(1, device="cuda"), torch.empty(B, Z, device="cuda"), torch.empty(B, Z, device="cuda"),
                             torch.empty(K, Z, device="cuda"), torch.empty(K, Z, device="cuda"))
    ws = torch.empty(L.query("ladder_diag_mixture_workspace_bytes", B, Z, K), dtype=torch.uint8, device="cuda")
    L.call("ladder_diag_mixture_fwd_bwd", *(p(v) for v in a), Lmc, B, Z, K, p(s), p(dmu), p(dsd), p(dcm), p(dcs), p(ws), ws.numel(), st)
    torch.cuda.synchronize()
    out.update(diag_sum=host(s), diag_dmu=host(dmu), diag_dsd=host(dsd), diag_dcm=host(dcm), diag_dcs=host(dcs))

    # ---- the same term on a wide code, and the per-row log-density (csrc/diag_mixture.hip)
    for Lmc, B, Z, K in DIAG_WIDE:
        rng = np.random.default_rng(410 + K)
        a = [dev(v) for v in (rng.standard_normal((B, Z)) * 1.2, 0.1 + rng.random((B, Z)), rng.standard_normal((Lmc, B, Z)), rng.standard_normal((K, Z)),
                              0.3 + rng.random((K, Z)))]
        s, dmu, dsd, dcm, dcs = (torch.empty(1, device="cuda"), torch.empty(B, Z, device="cuda"), torch.empty(B, Z, device="cuda"),
                                 torch.empty(K, Z, device="cuda"), torch.empty(K, Z, device="cuda"))
        ws = torch.empty(L.query("ladder_diag_mixture_wide_workspace_bytes", Lmc, B, Z, K), dtype=torch.uint8, device="cuda")
        L.call("ladder_diag_mixture_wide_fwd_bwd", *(p(v) for v in a), Lmc, B, Z, K, p(s), p(dmu), p(dsd), p(dcm), p(dcs), p(ws), ws.numel(), st)
        torch.cuda.synchronize()
        tag = "diag_wide_L%d_B%d_Z%d_K%d" % (Lmc, B, Z, K)
        out.update({tag + "_sum": host(s), tag + "_dmu": host(dmu), tag + "_dsd": host(dsd), tag + "_dcm": host(dcm), tag + "_dcs": host(dcs)})
    for n, Z, K in DIAG_ROWS:
        rng = np.random.default_rng(420 + K)
        z, cm, cs = dev(rng.standard_normal((n, Z)) * 1.5), dev(rng.standard_normal((K, Z))), dev(0.3 + rng.random((K, Z)))
        lp = torch.empty(n, device="cuda")
        ws = torch.empty(L.query("ladder_diag_mixture_logprob_rows_workspace_bytes", n, Z, K), dtype=torch.uint8, device="cuda")
        L.call("ladder_diag_mixture_logprob_rows", p(z), p(cm), p(cs), n, Z, K, p(lp), p(ws), ws.numel(), st)
        torch.cuda.synchronize()
        out["diag_rows_n%d_Z%d_K%d" % (n, Z, K)] = host(lp)

    # ---- the wide form of the full-covariance term (its sum of the partials is the kernel every term shares)
    K, R, Lmc, B = 3, 80, 3, 5
    mix = DeviceMixture(ctx, K, R)
    mix.set(*mixture(K, R, 113))
    mu, sd, eps, t = inputs(K, R, Lmc, B, N_ROWS, 213)
    s = torch.empty(1, device="cuda")
    dmu, dsd = mix.fwd_bwd(mu, sd, eps, s)
    lp = mix.log_prob_rows(t)
    torch.cuda.synchronize()
    out.update(wide_sum=host(s), wide_dmu=host(dmu), wide_dsd=host(dsd), wide_rows=host(lp))

    # ---- through Python
    d = np.load(os.path.join(ROOT, "tests", "golden", "oracle_mnist_digit.npz"))
    cfg = json.loads(str(d["config"]))
    eng = LadderEngine(cfg, "cuda:0", seed=1)
    for K, R in ((30, 2), (7, 12)):
        prior = MixturePrior(eng, *mixture(K, R, 100 + K))
        pts = np.random.default_rng(500 + K).standard_normal((N_ROWS, R)) * 2
        out["py_log_prob_K%d_R%d" % (K, R)] = np.asarray(prior.log_prob(pts).thunk())
    slp = SLPInterpolator(eng, *mixture(30, 2, 130))
    nll, g = slp.neg_log_likelihood(np.random.default_rng(530).standard_normal((5, 2)) * 2)
    out.update(py_slp_nll=np.float64(nll), py_slp_grad=g)

    def engine_run(cfg, tag):
        eng = LadderEngine(cfg, "cuda:0", seed=1)
        K, R, Z, Lmc, B = eng.K, eng.R, eng.Z, eng.Lmc, 4
        rng = np.random.default_rng(600)
        noise = dict(eps_z=rng.standard_normal((B, Z)), eps_t=rng.standard_normal((B, R)), eps_mc=rng.standard_normal((Lmc, B, R)))
        x = d["x"][:B]
        if not eng.vamp:
            eng.set_mixture(*mixture(K, R, 601))
            ptr = eng.mixture.buf.data_ptr()
            eng.set_mixture(*mixture(K, R, 602))                     # the second mixture must be the one in force, in the same buffer
            out[tag + "_buffer_kept"] = np.array(eng.mixture.buf.data_ptr() == ptr)
        for run, lr in ((eng.run_ae, cfg["learning_rate_ae"]), (eng.run_prior, cfg["learning_rate_prior"])):
            run(x, lr, noise, use_sg=False, use_mask=False)
            f = eng.fetch([n for n in L.S_NAMES if not n.startswith("_")])
            out["%s_%s" % (tag, run.__name__)] = np.array([f[k] for k in sorted(f)])
        return eng

    engine_run(cfg, "engine_ours")
    vcfg = dict(cfg, prior="vampPrior", n_mixtures=7)
    eng = engine_run(vcfg, "engine_vamp")
    rng = np.random.default_rng(700)
    code, latent, comp = eng.prior_sampler("vampPrior").sample(8, noise=dict(u=rng.random(8), eps=rng.standard_normal((8, eng.Z))))
    out.update(vamp_sample_code=host(code), vamp_sample_latent=host(latent), vamp_sample_comp=host(comp))

    np.savez(out_path, **out)
    print("wrote %d arrays to %s (library: %s)" % (len(out), out_path, out["library"]))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
