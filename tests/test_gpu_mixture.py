"""DeviceMixture (mixture.py), the one Python owner of the prepared mixture, against the raw exports of csrc/mixture.hip it wraps, and the
zero-weight component in ladder_gmm_logprob_rows (the guarded online log-sum-exp of csrc/gmm_packed.h)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _mixture(K, R, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(0, 0.3, (K, R, R))
    return rng.dirichlet(np.ones(K)), rng.normal(0, 1.5, (K, R)), A @ A.transpose(0, 2, 1) / R + 0.05 * np.eye(R)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _raw_prepare(L, st, K, R, gm):
    w, m, c = (_dev(a) for a in gm)
    dense = R > 8
    buf = torch.empty(L.query("ladder_gmm_dense_param_floats", K, R) if dense else K * L.query("ladder_gmm_packed_stride", R), device="cuda")
    L.call("ladder_gmm_prepare_dense" if dense else "ladder_gmm_prepare", w.data_ptr(), m.data_ptr(), c.data_ptr(), K, R, buf.data_ptr(), st)
    torch.cuda.synchronize()                                   # (w, m, c live until here)
    return buf


def _raw_fwd_bwd(L, st, buf, K, R, mu, sd, eps, grad=True):
    Lmc, B = eps.shape[0], mu.shape[0]
    out, dmu, dsd = torch.empty(1, device="cuda"), torch.empty(B, R, device="cuda"), torch.empty(B, R, device="cuda")
    name = "ladder_gmm_dense_logprob_fwd_bwd" if R > 8 else "ladder_gmm_logprob_fwd_bwd"
    nbytes = L.query("ladder_gmm_dense_workspace_bytes", Lmc, B, R, K) if R > 8 else L.query("ladder_gmm_workspace_bytes", Lmc, B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    L.call(name, mu.data_ptr(), sd.data_ptr(), eps.data_ptr(), buf.data_ptr(), Lmc, B, R, K, out.data_ptr(), dmu.data_ptr() if grad else None,
           dsd.data_ptr() if grad else None, ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    return out, dmu, dsd


def _raw_rows(L, st, buf, K, R, t):
    n = t.shape[0]
    lp = torch.empty(n, device="cuda")
    if R > 8:
        ws = torch.empty(L.query("ladder_gmm_dense_workspace_bytes", 1, n, R, K), dtype=torch.uint8, device="cuda")
        L.call("ladder_gmm_dense_logprob_rows", t.data_ptr(), buf.data_ptr(), n, R, K, lp.data_ptr(), ws.data_ptr(), ws.numel(), st)
    else:
        L.call("ladder_gmm_logprob_rows", t.data_ptr(), buf.data_ptr(), n, R, K, lp.data_ptr(), st)
    torch.cuda.synchronize()
    return lp


def _eq(a, b):
    return np.array_equal(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("K,R", [(30, 2), (7, 12)])
def test_device_mixture_equals_the_raw_exports(gpu_ctx, K, R):
    """Both forms (packed R <= 8, dense R > 8): the prepared buffer, fwd_bwd (sum, dmu, dsd) and log_prob_rows are bit for bit what the
    exports give when called directly on the same device inputs; the dense form without gradients returns (None, None) and the same sum."""
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.mixture import DeviceMixture
    st, gm = gpu_ctx.stream, _mixture(K, R, K)
    mix = DeviceMixture(gpu_ctx, K, R)
    mix.set(*gm)
    assert mix.dense == (R > 8)
    raw = _raw_prepare(L, st, K, R, gm)
    assert _eq(mix.buf, raw)
    rng = np.random.default_rng(R)
    Lmc, B, n = 5, 3, 7
    mu, sd, eps, t = _dev(rng.standard_normal((B, R)) * 2), _dev(0.05 + rng.random((B, R))), _dev(rng.standard_normal((Lmc, B, R))), _dev(rng.standard_normal((n, R)) * 2)
    out = torch.empty(1, device="cuda")
    dmu, dsd = mix.fwd_bwd(mu, sd, eps, out)
    r_out, r_dmu, r_dsd = _raw_fwd_bwd(L, st, raw, K, R, mu, sd, eps)
    assert _eq(out, r_out) and _eq(dmu, r_dmu) and _eq(dsd, r_dsd) and np.isfinite(out.item())
    out2 = torch.empty(1, device="cuda")
    g = mix.fwd_bwd(mu, sd, eps, out2, need_grad=False)
    assert _eq(out2, _raw_fwd_bwd(L, st, raw, K, R, mu, sd, eps, grad=R <= 8)[0])
    assert g == (None, None) if mix.dense else _eq(g[0], r_dmu) and _eq(g[1], r_dsd)
    lp = mix.log_prob_rows(t)
    assert lp.shape == (n,) and _eq(lp, _raw_rows(L, st, raw, K, R, t)) and np.isfinite(lp.cpu().numpy()).all()


def test_set_rewrites_the_same_buffer(gpu_ctx):
    """set() twice: the address captured graphs and the run cache hold never changes, and the second mixture is the one in force."""
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.mixture import DeviceMixture
    K, R = 30, 2
    mix = DeviceMixture(gpu_ctx, K, R)
    ptr = mix.buf.data_ptr()
    first, second = _mixture(K, R, 1), _mixture(K, R, 2)
    mix.set(*first)
    a = mix.buf.clone()
    mix.set(*second)
    assert mix.buf.data_ptr() == ptr and not _eq(mix.buf, a)
    assert _eq(mix.buf, _raw_prepare(L, gpu_ctx.stream, K, R, second))
    t = _dev(np.random.default_rng(3).standard_normal((7, R)))
    assert _eq(mix.log_prob_rows(t), _raw_rows(L, gpu_ctx.stream, mix.buf, K, R, t))


def test_wrong_shapes_raise_before_any_launch(gpu_ctx):
    from ladder_latent_data_distribution_modelling_amd.mixture import DeviceMixture
    K, R = 5, 2
    mix = DeviceMixture(gpu_ctx, K, R)
    w, m, c = _mixture(K, R, 0)
    mix.set(w, m, c)
    before = mix.buf.clone()
    for bad in ((w[:4], m, c), (w, m[:, :1], c), (w, m, c[:, :, :1]), (w, m.T, c), (w, m, c[:4]), (w[None], m, c)):
        with pytest.raises(ValueError, match="do not fit K = 5, R = 2"):
            mix.set(*bad)
    assert _eq(mix.buf, before)                                # nothing was written


def test_zero_weight_component_ahead_of_a_live_one(gpu_ctx):
    """K = 65, weights[0] = 0: lane 0 of ladder_gmm_logprob_rows owns components 0 and 64 and meets c_0 = -inf while its running maximum
    is still -inf.  The result must be finite and agree with float64 logsumexp over the 64 live components (tolerance of
    test_gpu_kernels.test_gmm_logprob: 2e-5 relative + 1e-3); so must the K > 64 two-pass kernel of ladder_gmm_logprob_fwd_bwd."""
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    K, R, n = 65, 2, 5
    w, m, c = _mixture(K, R, 65)
    w[0] = 0.0
    t = np.random.default_rng(66).standard_normal((n, R)) * 2
    w32, m32, c32, t32 = (np.asarray(a, np.float32).astype(np.float64) for a in (w, m, c, t))      # the fp32 values the device sees
    d = t32[:, None, :] - m32[None, 1:, :]
    maha = np.einsum("nki,kij,nkj->nk", d, np.linalg.inv(c32[1:]), d)
    lp = np.log(w32[1:] / w32.sum()) - 0.5 * np.linalg.slogdet(c32[1:])[1] - 0.5 * R * np.log(2 * np.pi) - 0.5 * maha
    ref = lp.max(1) + np.log(np.exp(lp - lp.max(1, keepdims=True)).sum(1))
    assert np.isfinite(ref).all()
    st = gpu_ctx.stream
    buf = _raw_prepare(L, st, K, R, (w, m, c))
    assert buf[0].item() == -np.inf                            # c_0 = log 0: the case under test is really reached
    td = _dev(t)
    rows = _raw_rows(L, st, buf, K, R, td).cpu().numpy().astype(np.float64)
    assert np.isfinite(rows).all() and (np.abs(rows - ref) < 2e-5 * np.abs(ref) + 1e-3).all()
    out, dmu, _ = _raw_fwd_bwd(L, st, buf, K, R, td, torch.ones_like(td), torch.zeros(1, n, R, device="cuda"))
    assert abs(out.item() - ref.sum()) < 2e-5 * abs(ref.sum()) + 1e-3 and np.isfinite(dmu.cpu().numpy()).all()
