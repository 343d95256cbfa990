"""The wide sampler (ladder_mixture_sample_wide*, csrc/sample.hip with the factorisation of csrc/chol_wide.h; 64 < R <= 256) against the float64
restatement of tests/test_gpu_generate.py: component = searchsorted(cdf, u, side="right") clamped, value = m_k + cholesky(cov_k) @ eps, every
element within (R + 3) 2^-23 (|m_k| + sum_j |L_ij| |eps_j|)."""
import json
import os

import numpy as np
import pytest
import torch

from oracle import ladder_oracle as O

pytestmark = pytest.mark.gpu
N = 1024


def _L():
    from ladder_latent_data_distribution_modelling_amd import _lib
    _lib.load()
    return _lib


def dev(a, dt=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dt)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def cdf64(w32):
    run = np.cumsum(np.maximum(np.asarray(w32, np.float32).astype(np.float64), 0.0))       # sequential, index order
    return run / run[-1]


def restate(w32, m32, chol64, u32, eps32):
    """the rule of tests/test_gpu_generate.py -> (component [n], value float64 [n, R], elementwise bound)"""
    cdf = cdf64(w32)
    K, R = m32.shape
    k = np.minimum(np.searchsorted(cdf, u32.astype(np.float64), side="right"), K - 1)
    m, e = m32.astype(np.float64), eps32.astype(np.float64)
    t = m[k] + np.einsum("nij,nj->ni", chol64[k], e)
    bound = (R + 3) * 2.0 ** -23 * (np.abs(m[k]) + np.einsum("nij,nj->ni", np.abs(chol64[k]), np.abs(e)))
    return k, t, bound


def prepare(st, w32, m32, c32=None, sd32=None):
    L = _L()
    K, R = m32.shape
    nb = L.query("ladder_mixture_sample_wide_param_bytes", K, R)
    assert nb > 0
    params = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    md = dev(m32)
    if c32 is not None:
        wd, cd = dev(w32), dev(c32)
        ws = torch.empty(L.query("ladder_mixture_sample_wide_prepare_workspace_bytes", K, R), dtype=torch.uint8, device="cuda")
        L.call("ladder_mixture_sample_wide_prepare", p(wd), p(md), p(cd), K, R, p(params), p(ws), ws.numel(), st)
    else:
        sd = dev(sd32)
        L.call("ladder_mixture_sample_wide_prepare_diag", p(md), p(sd), K, R, p(params), st)
    status = int(params[:4].view(torch.int32).item())          # (synchronises: the temporaries outlive the kernels)
    return params, status


def draw(st, params, K, R, n, first=0, u=None, eps=None, seed=0, offset=0):
    L = _L()
    out = torch.full((n, R), float("nan"), device="cuda")
    comp = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ud, ed = (dev(u), dev(eps)) if u is not None else (None, None)
    L.call("ladder_mixture_sample_wide", p(params), K, R, n, first, p(ud), p(ed), seed, offset, p(out), p(comp), st)
    return out.cpu().numpy(), comp.cpu().numpy()


def check_parity(st, w32, m32, c32=None, sd32=None, seed=0):
    K, R = m32.shape
    rng = np.random.default_rng(1000 + seed)
    u = rng.random(N).astype(np.float32)
    eps = rng.standard_normal((N, R)).astype(np.float32)
    params, status = prepare(st, w32, m32, c32, sd32)
    assert status == -1
    got, comp = draw(st, params, K, R, N, u=u, eps=eps)
    if c32 is not None:
        chol = np.linalg.cholesky(c32.astype(np.float64))
    else:
        chol = np.stack([np.diag(s) for s in sd32.astype(np.float64)])
        w32 = np.ones(K, np.float32)
    k, t, bound = restate(w32, m32, chol, u, eps)
    assert np.array_equal(comp, k), "component indices differ in %d of %d samples" % (int((comp != k).sum()), N)
    err = np.abs(got.astype(np.float64) - t)
    worst = float((err / np.maximum(bound, 1e-300)).max())
    print("K=%d R=%d: max |t - t_ref| / bound = %.3f" % (K, R, worst))
    assert (err <= bound).all(), worst


def synthetic(K, R):
    gm = O.synthetic_gm(dict(n_mixtures=K, representation_size=R), np.random.default_rng(K * 7 + R))
    return tuple(gm[k].astype(np.float32) for k in ("weights", "means", "covs"))


# ------------------------------------------------------------------------------------------------ 1. explicit-noise parity
@pytest.mark.parametrize("K,R", [(1, 80), (20, 128), (50, 256)])
def test_wide_sampler_parity_full_covariance(gpu_ctx, K, R):
    w, m, c = synthetic(K, R)
    check_parity(gpu_ctx.stream, w, m, c, seed=K + R)


def test_wide_sampler_parity_diagonal(gpu_ctx):
    K, R = 5, 256
    rng = np.random.default_rng(K * R)
    m = rng.normal(0, 1.5, (K, R)).astype(np.float32)
    sd = (0.05 + rng.random((K, R))).astype(np.float32)
    check_parity(gpu_ctx.stream, None, m, sd32=sd, seed=K)


def test_wide_sampler_one_component_standard_normal(gpu_ctx):
    """N(0, I_256) as the one-component mixture with zero mean and identity factor: the draw IS eps, bit for bit."""
    st, R = gpu_ctx.stream, 256
    params, status = prepare(st, None, np.zeros((1, R), np.float32), sd32=np.ones((1, R), np.float32))
    assert status == -1
    rng = np.random.default_rng(R)
    u, eps = rng.random(N).astype(np.float32), rng.standard_normal((N, R)).astype(np.float32)
    got, comp = draw(st, params, 1, R, N, u=u, eps=eps)
    assert (comp == 0).all() and np.array_equal(got, eps)


# ------------------------------------------------------------------------------------------------ 2. Philox mode
def test_wide_philox_chunks_seed_and_offset(gpu_ctx):
    st = gpu_ctx.stream
    w, m, c = synthetic(6, 256)
    K, R = m.shape
    params, status = prepare(st, w, m, c)
    assert status == -1
    seed, off = 77, 5
    one = draw(st, params, K, R, 300, seed=seed, offset=off)
    a, b = draw(st, params, K, R, 100, first=0, seed=seed, offset=off), draw(st, params, K, R, 200, first=100, seed=seed, offset=off)
    out, comp = np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]])
    assert np.array_equal(out.view(np.uint32), one[0].view(np.uint32)) and np.array_equal(comp, one[1])
    assert np.isfinite(one[0]).all() and (one[1] >= 0).all()
    for kw in (dict(seed=seed + 1, offset=off), dict(seed=seed, offset=off + 1)):
        other = draw(st, params, K, R, 300, **kw)
        assert (other[0] != one[0]).any(1).all(), kw                                   # every row changes


def test_wide_philox_statistics(gpu_ctx):
    """4 096 standard-normal draws at R = 256: every column mean within 5 standard errors; the generator blocks 2 .. 65 all deliver."""
    st, R, n = gpu_ctx.stream, 256, 4096
    params, status = prepare(st, None, np.zeros((1, R), np.float32), sd32=np.ones((1, R), np.float32))
    assert status == -1
    t, comp = draw(st, params, 1, R, n, seed=20240607)
    assert (comp == 0).all() and np.isfinite(t).all()
    z = np.abs(t.astype(np.float64).mean(0)) * np.sqrt(n)
    print("column means: max %.2f standard errors; column sd in [%.3f, %.3f]" % (z.max(), t.std(0).min(), t.std(0).max()))
    assert (z <= 5).all()
    assert len(np.unique(t[0])) == R                                                   # no block is delivered twice


# ------------------------------------------------------------------------------------------------ 3. refusals
def test_wide_sampler_refuses_foreign_and_unusable_buffers(gpu_ctx, golden_dir):
    st = gpu_ctx.stream
    w, m, c = synthetic(4, 128)
    params, status = prepare(st, w, m, c)
    assert status == -1
    good, comp = draw(st, params, 4, 128, 50, seed=1)
    assert np.isfinite(good).all() and (comp >= 0).all()
    for K2, R2 in ((3, 128), (4, 112)):
        out, comp = draw(st, params, K2, R2, 50, seed=1)
        assert np.isnan(out).all() and (comp == -1).all(), (K2, R2)
    val, vec = np.linalg.eigh(c[2].astype(np.float64))
    val[7] = -val[7]
    bad = c.copy()
    bad[2] = ((vec * val) @ vec.T).astype(np.float32)
    params, status = prepare(st, w, m, bad)
    assert status == 2
    out, comp = draw(st, params, 4, 128, 50, seed=1)
    assert np.isnan(out).all() and (comp == -1).all()
    from ladder_latent_data_distribution_modelling_amd.engine import LadderEngine
    d = np.load(os.path.join(golden_dir, "oracle_mnist_fashion.npz"))
    cfg = dict(json.loads(str(d["config"])), prior="GMM", code_size=128, n_mixtures=4)
    eng = LadderEngine(cfg, "cuda:0", seed=2)
    with pytest.raises(ValueError, match="component 2"):
        eng.prior_sampler("GMM", (w, m, bad))
    assert eng.prior_sampler("GMM", (w, m, c)).R == 128
