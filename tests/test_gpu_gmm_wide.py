"""The wide form of the fitted mixture (csrc/mixture_wide.hip, csrc/chol_wide.h; 64 < R <= 256) through the C ABI and DeviceMixture against the float64
oracle: the term and its gradients at the bars of test_gpu_kernels.py::test_gmm_dense_logprob, overlapping components (responsibilities that are not
one-hot), the per-row log-prob, and the status word of a component without a factor."""
import numpy as np
import pytest
import torch

from oracle import ladder_oracle as O

pytestmark = pytest.mark.gpu
GUARD = 64


def _lib():
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    return L


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def close(got, ref, rtol, what=""):
    """the helper of tests/test_gpu_kernels.py: max |got - ref| relative to max |ref|"""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    ref = ref.detach().numpy().astype(np.float64) if isinstance(ref, torch.Tensor) else np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref).max() / scale
    print("%s: rel err %.3e (tol %.1e)" % (what, err, rtol))
    assert np.isfinite(got).all() and err < rtol, "%s: rel err %.3e (tol %.1e)" % (what, err, rtol)


def prepare(st, gm, K, R):
    """-> (prepared buffer, status word)"""
    L = _lib()
    params = torch.zeros(L.query("ladder_gmm_wide_param_bytes", K, R), dtype=torch.uint8, device="cuda")
    ws = torch.empty(L.query("ladder_gmm_wide_prepare_workspace_bytes", K, R), dtype=torch.uint8, device="cuda")
    wd, md, cd = dev(gm["weights"]), dev(gm["means"]), dev(gm["covs"])
    L.call("ladder_gmm_wide_prepare", p(wd), p(md), p(cd), K, R, p(params), p(ws), ws.numel(), st)
    return params, int(params[:4].view(torch.int32).item())           # (synchronises: the temporaries outlive the kernels)


def nan_workspace(nbytes):
    return torch.full(((nbytes + 3) // 4,), float("nan"), device="cuda")


def reference(gm, mu, sd, eps):
    """float64: (sum of log-probs, d/dmu, d/dsd, responsibilities [L*B, K])"""
    mut, sdt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (mu, sd))
    t = mut.unsqueeze(0) + sdt.unsqueeze(0) * torch.tensor(eps, dtype=torch.float64)
    w, m, c = (torch.tensor(gm[k], dtype=torch.float64) for k in ("weights", "means", "covs"))
    lp = O.gmm_log_prob(t, w, m, c)
    lp.sum().backward()
    with torch.no_grad():
        comp = torch.stack([O.gmm_log_prob(t, torch.ones(1, dtype=torch.float64), m[k:k + 1], c[k:k + 1]) for k in range(len(w))], -1)
        resp = torch.softmax(comp + torch.log(w / w.sum()), -1).reshape(-1, len(w)).numpy()
    return lp.sum().item(), mut.grad, sdt.grad, resp


def run_term(st, params, mu, sd, eps, K, R):
    """training call, forward-only call, training call again -> the three sums, (dmu, dsd) of both training calls; guards and bit-equality asserted"""
    L = _lib()
    Lmc, B = eps.shape[:2]
    nws = L.query("ladder_gmm_wide_workspace_bytes", Lmc, B, R, K)
    assert nws > 0
    mud, sdd, epsd = dev(mu), dev(sd), dev(eps)
    res = []
    for train in (True, False, True):
        ws = nan_workspace(nws)
        out = torch.full((1 + GUARD,), 7.0, device="cuda")
        dmu, dsd = torch.full((B * R + GUARD,), 7.0, device="cuda"), torch.full((B * R + GUARD,), 7.0, device="cuda")
        L.call("ladder_gmm_wide_logprob_fwd_bwd", p(mud), p(sdd), p(epsd), p(params), Lmc, B, R, K, p(out), p(dmu) if train else None,
               p(dsd) if train else None, p(ws), 4 * ws.numel(), st)
        torch.cuda.synchronize()
        assert (out[1:] == 7.0).all() and (dmu[B * R:] == 7.0).all() and (dsd[B * R:] == 7.0).all(), "guard floats were written"
        if not train:
            assert (dmu == 7.0).all() and (dsd == 7.0).all()
        res.append((out[:1].cpu(), dmu[:B * R].reshape(B, R).cpu(), dsd[:B * R].reshape(B, R).cpu()))
    bits = lambda t: t.numpy().view(np.uint32)
    assert np.array_equal(bits(res[0][0]), bits(res[1][0])), "forward-only sum differs from the training call's"
    for a, b in zip(res[0], res[2]):
        assert np.array_equal(bits(a), bits(b)), "two training calls differ"
    return res[0]


def check_term(st, gm, mu, sd, eps, K, R, ref):
    params, status = prepare(st, gm, K, R)
    assert status == -1
    out, dmu, dsd = run_term(st, params, mu, sd, eps, K, R)
    print("K=%d R=%d S=%d: sum %.6f ref %.6f" % (K, R, eps.shape[0] * eps.shape[1], out.item(), ref[0]))
    assert abs(out.item() - ref[0]) < 3e-5 * abs(ref[0]) + 1e-3
    close(dmu, ref[1], 1e-4, "dmu")
    close(dsd, ref[2], 1e-4, "dsd")


def synthetic_inputs(K, R, Lmc, B):
    """as test_gmm_dense_logprob builds them"""
    rng = np.random.default_rng(K * 7 + R)
    gm = {k: v.astype(np.float32) for k, v in O.synthetic_gm(dict(n_mixtures=K, representation_size=R), rng).items()}
    mu = (rng.standard_normal((B, R)) * 1.5).astype(np.float32)
    sd = (0.05 + rng.random((B, R))).astype(np.float32)
    eps = rng.standard_normal((Lmc, B, R)).astype(np.float32)
    return gm, mu, sd, eps


@pytest.mark.parametrize("K,R,Lmc,B", [(1, 80, 3, 5),        # one component, S under a tile, R not a multiple of 64
                                       (7, 128, 7, 19),      # S = 133: a tile tail
                                       (50, 256, 10, 64),    # the shipped K and R
                                       (3, 256, 1, 1),       # one sample
                                       (6, 96, 100, 4)])     # long L reduction
def test_gmm_wide_logprob(gpu_ctx, K, R, Lmc, B):
    gm, mu, sd, eps = synthetic_inputs(K, R, Lmc, B)
    check_term(gpu_ctx.stream, gm, mu, sd, eps, K, R, reference(gm, mu, sd, eps))


def soft_inputs(R, seed=0, K=5, Lmc=6, B=8):
    """K components that share one covariance of the synthetic recipe, their means 0.05 apart: the responsibilities are not one-hot"""
    rng = np.random.default_rng(seed)
    one = O.synthetic_gm(dict(n_mixtures=1, representation_size=R), rng)
    m0 = one["means"][0]
    gm = dict(weights=rng.dirichlet(np.ones(K)).astype(np.float32), means=(m0 + 0.05 * rng.standard_normal((K, R))).astype(np.float32),
              covs=np.repeat(one["covs"], K, 0).astype(np.float32))
    mu = (m0 + 0.05 * rng.standard_normal((B, R))).astype(np.float32)
    sd = (0.05 + 0.2 * rng.random((B, R))).astype(np.float32)
    eps = rng.standard_normal((Lmc, B, R)).astype(np.float32)
    return gm, mu, sd, eps


@pytest.mark.parametrize("R", [80, 256])
def test_gmm_wide_soft_responsibilities(gpu_ctx, R):
    """With the recipe of test_gmm_wide_logprob the components never overlap at these widths; here the logsumexp and the mixed backward are exercised."""
    K = 5
    gm, mu, sd, eps = soft_inputs(R)
    ref = reference(gm, mu, sd, eps)
    share = float((ref[3].max(-1) < 0.9).mean())
    print("R=%d: share of samples with max responsibility < 0.9: %.2f" % (R, share))
    assert share >= 0.5
    check_term(gpu_ctx.stream, gm, mu, sd, eps, K, R, ref)


@pytest.mark.parametrize("n", [1, 130])
def test_gmm_wide_logprob_rows(gpu_ctx, n):
    L, st = _lib(), gpu_ctx.stream
    K, R = 7, 128
    gm, mu, sd, eps = synthetic_inputs(K, R, 1, n)
    t = (mu + sd * eps[0]).astype(np.float32)
    ref = O.gmm_log_prob(torch.tensor(t, dtype=torch.float64), *(torch.tensor(gm[k], dtype=torch.float64) for k in ("weights", "means", "covs"))).numpy()
    params, status = prepare(st, gm, K, R)
    assert status == -1
    nws = L.query("ladder_gmm_wide_workspace_bytes", 1, n, R, K)
    ws = nan_workspace(nws)
    out = torch.full((n + GUARD,), 7.0, device="cuda")
    td = dev(t)
    L.call("ladder_gmm_wide_logprob_rows", p(td), p(params), n, R, K, p(out), p(ws), 4 * ws.numel(), st)
    got = out.cpu().numpy().astype(np.float64)
    assert (got[n:] == 7.0).all()
    err = np.abs(got[:n] - ref)
    print("rows n=%d: max err %.3e, max |ref| %.3e" % (n, err.max(), np.abs(ref).max()))
    assert np.isfinite(got[:n]).all() and (err < 3e-5 * np.abs(ref) + 1e-3).all()
    # the owner's path gives the same values
    from ladder_latent_data_distribution_modelling_amd.mixture import DeviceMixture
    mix = DeviceMixture(gpu_ctx, K, R)
    assert mix.wide and not mix.dense
    mix.set(gm["weights"], gm["means"], gm["covs"])
    assert np.array_equal(mix.log_prob_rows(td).cpu().numpy(), out[:n].cpu().numpy())


def test_gmm_wide_status_and_foreign_buffer(gpu_ctx):
    from ladder_latent_data_distribution_modelling_amd.mixture import DeviceMixture
    L, st = _lib(), gpu_ctx.stream
    K, R, Lmc, B = 4, 128, 3, 5
    gm, mu, sd, eps = synthetic_inputs(K, R, Lmc, B)
    good, status = prepare(st, gm, K, R)
    assert status == -1
    val, vec = np.linalg.eigh(gm["covs"][2].astype(np.float64))
    val[5] = -val[5]                                                    # one eigenvalue flipped: indefinite
    bad = dict(gm, covs=gm["covs"].copy())
    bad["covs"][2] = ((vec * val) @ vec.T).astype(np.float32)
    params, status = prepare(st, bad, K, R)
    assert status == 2
    mix = DeviceMixture(gpu_ctx, K, R)
    with pytest.raises(ValueError, match="component 2"):
        mix.set(bad["weights"], bad["means"], bad["covs"])
    with pytest.raises(ValueError, match="positive finite sum"):
        mix.set(np.zeros(K, np.float32), bad["means"], gm["covs"])
    mix.set(gm["weights"], gm["means"], gm["covs"])                    # the same buffer, rewritten in place, is usable again
    with pytest.raises(ValueError, match="256"):
        DeviceMixture(gpu_ctx, K, 72)

    def term(buf, K_, R_, train):
        ws = nan_workspace(L.query("ladder_gmm_wide_workspace_bytes", Lmc, B, R_, K_))
        out, dmu, dsd = torch.zeros(1, device="cuda"), torch.zeros(B, R_, device="cuda"), torch.zeros(B, R_, device="cuda")
        mud, sdd, epsd = dev(mu[:, :R_]), dev(sd[:, :R_]), dev(eps[:, :, :R_])
        L.call("ladder_gmm_wide_logprob_fwd_bwd", p(mud), p(sdd), p(epsd), p(buf), Lmc, B, R_, K_, p(out), p(dmu) if train else None,
               p(dsd) if train else None, p(ws), 4 * ws.numel(), st)
        return out.item(), dmu.cpu().numpy()

    assert np.isfinite(term(good, K, R, False)[0])
    for train in (False, True):
        s, g = term(params, K, R, train)                               # a component without a factor
        assert np.isnan(s) and (not train or np.isnan(g).all())
        s, g = term(good, K, 112, train)                               # prepared for (4, 128), called with (4, 112)
        assert np.isnan(s) and (not train or np.isnan(g).all())
