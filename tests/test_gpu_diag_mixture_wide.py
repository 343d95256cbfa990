"""The VampPrior term on a wide code (csrc/diag_mixture.hip; 80 <= Z <= 256, Z % 16 == 0) through the C ABI against float64 autograd of the formula
in codes/base.py:244-254, 361-370, written as tests/test_gpu_kernels.py::test_diag_mixture_vamp writes it, at that test's bars:

    |sum - ref| < 3e-5 |ref| + 1e-3,   each of the four gradients within 1e-4 of the reference's largest magnitude.

Where the formula itself is worse conditioned than that in float32 the gradient bar is max(1e-4 * scale, 5 * cond), cond = max |f32 - f64| of the same
formula restated in float32 torch on the CPU (the rule of test_gmm_prior_wide_code_vs_oracle); every check prints error, scale and cond.
Measured on an MI355X: over the six shapes and both data sets of test_parity the largest gradient error is 1.5e-5 of the scale (dcomp_sd at K 50, Z 256,
clustered: err 8.2e-5, scale 5.48, cond 7.6e-5), the far-sample case 1.4e-7 of the scale, the largest sum error 1.0e-7 of the reference: 1e-4 * scale
was the larger term of the bar in every check, so no shape needed more than the narrow test's bars."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
E_SHAPE, E_WORKSPACE = -1, -3
GUARD = 64

# (K, Z, L, B)
CASES = [(5, 80, 6, 3),        # five 16-blocks: neither a multiple of 64 nor of the 256-thread block
         (50, 256, 7, 5),      # the limit width, the reference's K
         (70, 144, 3, 4),      # more components than one wavefront of owners, a tail chunk of 6
         (1, 96, 1, 1),        # every degenerate end
         (130, 80, 2, 2),      # more components than any one chunk: three owner passes, nine accumulate chunks
         (7, 208, 9, 130)]     # B above 128, L not a multiple of any L-split


def _lib():
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    return L


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def inputs(kind, K, Z, Lmc, B):
    """fp32 (mu, sd, eps, comp_mean, comp_sd).  "scattered": as test_diag_mixture_vamp draws them, responsibilities one-hot for nearly every sample;
    "clustered": components and posteriors around one point, so that the log-sum-exp and the responsibility weights matter."""
    rng = np.random.default_rng(K + Z)
    if kind == "scattered":
        mu = rng.standard_normal((B, Z)) * 1.2
        sd = 0.1 + rng.random((B, Z))
        eps = rng.standard_normal((Lmc, B, Z))
        cm = rng.standard_normal((K, Z))
        cs = 0.3 + rng.random((K, Z))
    else:
        base = rng.standard_normal(Z)
        cm = base + 0.05 * rng.standard_normal((K, Z))
        cs = 0.8 * (1 + 0.02 * rng.standard_normal((K, Z)))
        mu = base + 0.3 * rng.standard_normal((B, Z))
        sd = 0.1 + rng.random((B, Z))
        eps = rng.standard_normal((Lmc, B, Z))
    return tuple(np.ascontiguousarray(a, np.float32) for a in (mu, sd, eps, cm, cs))


def formula(arrs, dtype):
    """-> (sum of log-probs, [dmu, dsd, dcomp_mean, dcomp_sd], responsibilities [L*B, K]) by torch autograd in `dtype` on the CPU"""
    mu, sd, eps, cm, cs = arrs
    K, Z = cm.shape
    mut, sdt, cmt, cst = (torch.tensor(a, dtype=dtype, requires_grad=True) for a in (mu, sd, cm, cs))
    z = (mut.unsqueeze(0) + sdt.unsqueeze(0) * torch.tensor(eps, dtype=dtype)).unsqueeze(2)
    u = (z - cmt) / cst
    lp = -0.5 * (u ** 2).sum(-1) - torch.log(cst).sum(-1) - 0.5 * Z * np.log(2 * np.pi) - np.log(K)
    tot = torch.logsumexp(lp, dim=-1).sum()
    tot.backward()
    resp = torch.softmax(lp.detach(), -1).reshape(-1, K).numpy()
    return tot.item(), [t.grad.numpy().astype(np.float64) for t in (mut, sdt, cmt, cst)], resp


@functools.lru_cache(maxsize=None)
def reference(kind, K, Z, Lmc, B):
    """computed once per (data set, shape) and shared: (inputs, float64 results, float32 results)"""
    arrs = inputs(kind, K, Z, Lmc, B)
    return arrs, formula(arrs, torch.float64), formula(arrs, torch.float32)


def run(st, arrs, ws=None, ws_offset=0):
    """one call -> (sum [1], dmu, dsd, dcomp_mean, dcomp_sd) on the host; guard floats behind every output asserted untouched"""
    L = _lib()
    mu, sd, eps, cm, cs = arrs
    (Lmc, B, Z), K = eps.shape, cm.shape[0]
    nws = L.query("ladder_diag_mixture_wide_workspace_bytes", Lmc, B, Z, K)
    assert nws > 0
    if ws is None:
        ws = torch.empty(nws + ws_offset, dtype=torch.uint8, device="cuda")
    sizes = (1, B * Z, B * Z, K * Z, K * Z)
    outs = [torch.full((n + GUARD,), 7.0, device="cuda") for n in sizes]
    a = [dev(v) for v in arrs]
    L.call("ladder_diag_mixture_wide_fwd_bwd", *(p(t) for t in a), Lmc, B, Z, K, *(p(o) for o in outs), p(ws) + ws_offset, nws, st)
    torch.cuda.synchronize()
    for o, n in zip(outs, sizes):
        assert (o[n:] == 7.0).all(), "guard floats were written"
    shapes = ((1,), (B, Z), (B, Z), (K, Z), (K, Z))
    return [o[:n].reshape(s).cpu().numpy() for o, n, s in zip(outs, sizes, shapes)]


def check(got, ref64, ref32, what):
    tot, grads, _ = ref64
    err = abs(float(got[0][0]) - tot)
    print("%s sum: %.6f ref %.6f err %.3e (bar %.3e)" % (what, float(got[0][0]), tot, err, 3e-5 * abs(tot) + 1e-3))
    assert np.isfinite(got[0]).all() and err < 3e-5 * abs(tot) + 1e-3, (what, float(got[0][0]), tot)
    for name, g, r64, r32 in zip(("dmu", "dsd", "dcomp_mean", "dcomp_sd"), got[1:], grads, ref32[1]):
        scale = max(np.abs(r64).max(), 1e-30)
        cond = np.abs(r32 - r64).max()
        err = np.abs(g.astype(np.float64) - r64).max()
        print("%s %s: err %.3e scale %.3e cond %.3e (err/scale %.2e)" % (what, name, err, scale, cond, err / scale))
        assert np.isfinite(g).all() and err < max(1e-4 * scale, 5 * cond), (what, name, err, scale, cond)


@pytest.mark.parametrize("kind", ["scattered", "clustered"])
@pytest.mark.parametrize("K,Z,Lmc,B", CASES)
def test_parity(gpu_ctx, K, Z, Lmc, B, kind):
    arrs, ref64, ref32 = reference(kind, K, Z, Lmc, B)
    if kind == "clustered" and K > 1:
        top = ref64[2].max(-1)
        assert (top < 0.9).mean() >= 0.5, "the clustered set is meant to have soft responsibilities: %.2f of the samples below 0.9" % (top < 0.9).mean()
    check(run(gpu_ctx.stream, arrs), ref64, ref32, "%s K=%d Z=%d L=%d B=%d" % (kind, K, Z, Lmc, B))


def test_far_samples_stay_finite(gpu_ctx):
    """mu shifted by 60 in every dimension: every log-prob is below -1e4, the max-subtracted log-sum-exp keeps every output finite and within the bars"""
    mu, sd, eps, cm, cs = inputs("scattered", 50, 256, 7, 5)
    arrs = ((mu + 60.0).astype(np.float32), sd, eps, cm, cs)
    ref64, ref32 = formula(arrs, torch.float64), formula(arrs, torch.float32)
    assert ref64[0] / (7 * 5) < -1e4
    check(run(gpu_ctx.stream, arrs), ref64, ref32, "far")


def test_duplicate_and_dead_components(gpu_ctx):
    """Identical components (in one chunk of 16, in two chunks, in two passes of 64 owners) get the same gradient rows bit for bit; a component whose
    responsibility is exactly 0 on every sample in float64 gets an exactly zero dcomp_mean row (and a zero dcomp_sd row)."""
    mu, sd, eps, cm, cs = (a.copy() for a in inputs("clustered", 130, 80, 2, 2))
    for a, b in ((0, 1), (3, 20), (5, 100)):
        cm[b], cs[b] = cm[a], cs[a]
    cm[77] = cm[77] + 200.0
    cs[77] = 0.3
    arrs = (mu, sd, eps, cm, cs)
    ref64 = formula(arrs, torch.float64)
    assert (ref64[2][:, 77] == 0.0).all() and (ref64[1][2][77] == 0.0).all()
    got = run(gpu_ctx.stream, arrs)
    check(got, ref64, formula(arrs, torch.float32), "duplicates")
    bits = lambda x: x.view(np.uint32)
    for a, b in ((0, 1), (3, 20), (5, 100)):
        assert np.array_equal(bits(got[3][a]), bits(got[3][b])) and np.array_equal(bits(got[4][a]), bits(got[4][b])), (a, b)
        assert np.abs(got[3][a]).max() > 0
    assert (got[3][77] == 0.0).all() and (got[4][77] == 0.0).all()


@pytest.mark.parametrize("Z", [80, 256])
def test_agrees_with_the_full_covariance_wide_term(gpu_ctx, Z):
    """covs_k = diag(s_k^2), weights 1/K: ladder_gmm_wide_logprob_fwd_bwd on the same (mu, sd, eps) gives the same sum_logp, dmu and dsd, within the sum
    of both kernels' bars (tests/test_gpu_gmm_wide.py holds that one to the same bars as this file)."""
    L, st = _lib(), gpu_ctx.stream
    K, Lmc, B = 7, 6, 5
    arrs, ref64, _ = reference("clustered", K, Z, Lmc, B)
    mu, sd, eps, cm, cs = arrs
    got = run(st, arrs)
    covs = np.zeros((K, Z, Z), np.float32)
    covs[:, np.arange(Z), np.arange(Z)] = cs.astype(np.float32) ** 2
    params = torch.zeros(L.query("ladder_gmm_wide_param_bytes", K, Z), dtype=torch.uint8, device="cuda")
    pws = torch.empty(L.query("ladder_gmm_wide_prepare_workspace_bytes", K, Z), dtype=torch.uint8, device="cuda")
    wd, md, cd = dev(np.full(K, 1.0 / K)), dev(cm), dev(covs)
    L.call("ladder_gmm_wide_prepare", p(wd), p(md), p(cd), K, Z, p(params), p(pws), pws.numel(), st)
    assert int(params[:4].view(torch.int32).item()) == -1
    ws = torch.empty(L.query("ladder_gmm_wide_workspace_bytes", Lmc, B, Z, K), dtype=torch.uint8, device="cuda")
    out, dmu, dsd = torch.empty(1, device="cuda"), torch.empty(B, Z, device="cuda"), torch.empty(B, Z, device="cuda")
    a = [dev(v) for v in (mu, sd, eps)]
    L.call("ladder_gmm_wide_logprob_fwd_bwd", *(p(t) for t in a), p(params), Lmc, B, Z, K, p(out), p(dmu), p(dsd), p(ws), ws.numel(), st)
    torch.cuda.synchronize()
    tot = ref64[0]
    print("Z=%d sum: diagonal %.6f full %.6f ref %.6f" % (Z, float(got[0][0]), out.item(), tot))
    assert abs(float(got[0][0]) - out.item()) < 2 * (3e-5 * abs(tot) + 1e-3)
    for name, g, full, r64 in (("dmu", got[1], dmu, ref64[1][0]), ("dsd", got[2], dsd, ref64[1][1])):
        scale = np.abs(r64).max()
        err = np.abs(g.astype(np.float64) - full.cpu().numpy().astype(np.float64)).max()
        print("Z=%d %s: |diagonal - full| %.3e scale %.3e" % (Z, name, err, scale))
        assert err < 2e-4 * scale, (name, err, scale)


def test_same_bits_whatever_the_workspace_held(gpu_ctx):
    """The same call twice, once more on a workspace filled with NaN, once more with the workspace pointer 4 bytes off (the entry aligns it itself):
    all five outputs equal bit for bit."""
    L, st = _lib(), gpu_ctx.stream
    K, Z, Lmc, B = 50, 256, 7, 5
    arrs = inputs("clustered", K, Z, Lmc, B)
    nws = L.query("ladder_diag_mixture_wide_workspace_bytes", Lmc, B, Z, K)
    ws = torch.zeros(nws + 8, dtype=torch.uint8, device="cuda")
    first = run(st, arrs, ws)
    again = run(st, arrs, ws)
    ws.view(torch.float32).fill_(float("nan"))
    poisoned = run(st, arrs, ws)
    ws.view(torch.float32).fill_(float("nan"))
    shifted = run(st, arrs, ws, ws_offset=4)
    for other in (again, poisoned, shifted):
        for a, b in zip(first, other):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_abi(gpu_ctx):
    L, st = _lib(), gpu_ctx.stream
    x = torch.ones(4 * 1024 * 272, device="cuda")
    outs = [torch.full((1024 * 272,), 7.0, device="cuda") for _ in range(5)]
    ws = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
    wide = lambda Lmc, B, Z, K, wsp=p(ws), n=ws.numel(): L.query("ladder_diag_mixture_wide_fwd_bwd", *([p(x)] * 5), Lmc, B, Z, K, *(p(o) for o in outs), wsp, n, st)
    for Z in (64, 72, 88, 272):
        assert wide(3, 2, Z, 4) == E_SHAPE, Z
    for K in (0, 1025):
        assert wide(3, 2, 80, K) == E_SHAPE, K
    assert wide(0, 2, 80, 4) == E_SHAPE and wide(3, 0, 80, 4) == E_SHAPE
    need = L.query("ladder_diag_mixture_wide_workspace_bytes", 3, 2, 80, 4)
    assert 0 < need <= ws.numel()
    assert wide(3, 2, 80, 4, None, need) == E_WORKSPACE and wide(3, 2, 80, 4, p(ws), need - 1) == E_WORKSPACE
    torch.cuda.synchronize()
    assert all((o == 7.0).all() for o in outs), "a refused call wrote to an output"
    # the narrow entry keeps its rule
    assert L.query("ladder_diag_mixture_fwd_bwd", *([p(x)] * 5), 3, 2, 80, 4, *(p(o) for o in outs), p(ws), ws.numel(), st) == E_SHAPE
    torch.cuda.synchronize()
    assert all((o == 7.0).all() for o in outs)
    # the largest component count at the smallest width, two samples
    arrs = inputs("scattered", 1024, 80, 1, 2)
    got = run(st, arrs)
    assert all(np.isfinite(g).all() for g in got)
    assert wide(3, 2, 80, 4, p(ws), need) == 0
