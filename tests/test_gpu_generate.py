"""Generation from the prior on the device (csrc/sample.hip, LadderEngine.prior_sampler / generate, the trainer's
generate_samples_from_prior_by_method / generate_images, `model.psedeu_prior`, generate.py) against float64 numpy restatements written
here and the oracle's decoder sub-graphs.

The restatement of the sampler: cumulative distribution in float64 with both sums formed sequentially in index order (the running sum's
last entry is the total -- `w64.sum()` would be numpy's PAIRWISE sum, which can differ from the sequential one in the last bit and is
therefore not used), component = searchsorted(cdf, u, side="right") clamped, value = m_k + cholesky(cov_k) @ eps.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ladder_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ALIGN = -2
N = 4096


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
    """-> (component [n], value float64 [n, R], elementwise bound of the issue: (R+3) 2^-23 (|m_k| + sum_j |L_k,ij| |eps_j|))."""
    cdf = cdf64(w32)
    K, R = m32.shape
    k = np.minimum(np.searchsorted(cdf, u32.astype(np.float64), side="right"), K - 1)
    m, e = m32.astype(np.float64), eps32.astype(np.float64)
    t = m[k] + np.einsum("nij,nj->ni", chol64[k], e)
    bound = (R + 3) * 2.0 ** -23 * (np.abs(m[k]) + np.einsum("nij,nj->ni", np.abs(chol64[k]), np.abs(e)))
    return k, t, bound


def prepare(st, w32, m32, c32=None, sd32=None):
    """Prepared parameter buffer + its status word.  Full covariances `c32`, or diagonal components `sd32` (equal weights)."""
    L = _L()
    K, R = m32.shape
    nb = L.query("ladder_mixture_sample_param_bytes", K, R)
    assert nb > 0
    params = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    md = dev(m32)
    if c32 is not None:
        wd, cd = dev(w32), dev(c32)
        L.call("ladder_mixture_sample_prepare", p(wd), p(md), p(cd), K, R, p(params), st)
    else:
        sd = dev(sd32)
        L.call("ladder_mixture_sample_prepare_diag", p(md), p(sd), K, R, p(params), st)
    status = int(params[:4].view(torch.int32).item())          # (synchronises: the temporaries outlive the kernels)
    return params, status


def draw(st, params, K, R, n, first=0, u=None, eps=None, seed=0, offset=0):
    L = _L()
    out = torch.full((n, R), float("nan"), device="cuda")
    comp = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    ud, ed = (dev(u), dev(eps)) if u is not None else (None, None)
    L.call("ladder_mixture_sample", p(params), K, R, n, first, p(ud), p(ed), seed, offset, p(out), p(comp), st)
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


def fixture_mixture(golden_dir, which):
    fix = np.load(os.path.join(golden_dir, "GM_prior_info.npz"))
    return tuple(fix["%s_%s" % (a, which)].astype(np.float32) for a in ("w", "m", "K"))


# ------------------------------------------------------------------------------------------------ 1. explicit-noise parity
@pytest.mark.parametrize("which", ["full", "active"])
def test_sampler_parity_reference_mixture(gpu_ctx, golden_dir, which):
    w, m, c = fixture_mixture(golden_dir, which)
    assert m.shape == ((50, 2) if which == "full" else (27, 2))
    assert np.linalg.cond(c.astype(np.float64)).max() <= 16
    check_parity(gpu_ctx.stream, w, m, c, seed=len(w))


@pytest.mark.parametrize("K,R,dense", [(5, 1, False), (50, 8, False), (70, 3, False), (30, 64, True), (20, 16, True)])
def test_sampler_parity_synthetic(gpu_ctx, golden_dir, K, R, dense):
    """Mixtures built as test_gmm_logprob (R <= 8) and test_gmm_dense_logprob (wide latent) build theirs."""
    cfg = dict(n_mixtures=K, representation_size=R)
    if dense:
        gm = O.synthetic_gm(cfg, np.random.default_rng(K * 7 + R))
    else:
        fix = np.load(os.path.join(golden_dir, "GM_prior_info.npz"))
        gm = O.synthetic_gm(cfg, np.random.default_rng(K + R), fix if K <= 50 else None)
    w, m, c = (gm[k].astype(np.float32) for k in ("weights", "means", "covs"))
    check_parity(gpu_ctx.stream, w, m, c, seed=K + R)


def test_sampler_parity_parameters_beyond_lds(gpu_ctx):
    """R <= 8 with a parameter buffer over 48 KB: the one-thread-per-sample kernel reads it in place instead of staging it in LDS."""
    K, R = 300, 8
    assert _L().query("ladder_mixture_sample_param_bytes", K, R) > 48 * 1024
    gm = O.synthetic_gm(dict(n_mixtures=K, representation_size=R), np.random.default_rng(K + R))
    w, m, c = (gm[k].astype(np.float32) for k in ("weights", "means", "covs"))
    check_parity(gpu_ctx.stream, w, m, c, seed=K + R)


@pytest.mark.parametrize("R", [2, 16])
def test_sampler_refuses_a_buffer_of_another_shape(gpu_ctx, R):
    """K and R of the call are compared with the prepared header on the device: a mismatch, or a buffer whose status is not "usable",
    gives NaN / -1 for every sample and reads nothing through a wrong layout (both kernel shapes)."""
    st = gpu_ctx.stream
    gm = O.synthetic_gm(dict(n_mixtures=20, representation_size=R), np.random.default_rng(R))
    w, m, c = (gm[k].astype(np.float32) for k in ("weights", "means", "covs"))
    params, status = prepare(st, w, m, c)
    assert status == -1
    good, comp = draw(st, params, 20, R, 300, seed=1)
    assert np.isfinite(good).all() and (comp >= 0).all()
    for K2, R2 in ((19, R), (20, R - 1)):                    # (smaller shapes: the output buffers of draw() fit either way)
        out, comp = draw(st, params, K2, R2, 300, seed=1)
        assert np.isnan(out).all() and (comp == -1).all(), (K2, R2)
    bad = c.copy()
    bad[3] = -np.eye(R, dtype=np.float32)
    params, status = prepare(st, w, m, bad)
    assert status == 3
    out, comp = draw(st, params, 20, R, 300, seed=1)
    assert np.isnan(out).all() and (comp == -1).all()


@pytest.mark.parametrize("K,R", [(10, 8), (7, 13), (12, 64)])
def test_sampler_parity_diagonal(gpu_ctx, K, R):
    """The VampPrior's mixture: K equally weighted diagonal components (both kernel shapes; R = 13: a ragged last generator block)."""
    rng = np.random.default_rng(K * R)
    m = rng.normal(0, 1.5, (K, R)).astype(np.float32)
    sd = (0.05 + rng.random((K, R))).astype(np.float32)
    check_parity(gpu_ctx.stream, None, m, sd32=sd, seed=K)


@pytest.mark.parametrize("R", [2, 8, 64])
def test_sampler_parity_one_component_standard_normal(gpu_ctx, R):
    """N(0, I_R) as the one-component mixture with zero mean and identity factor: the draw IS eps, bit for bit."""
    st = gpu_ctx.stream
    params, status = prepare(st, None, np.zeros((1, R), np.float32), sd32=np.ones((1, R), np.float32))
    assert status == -1
    rng = np.random.default_rng(R)
    u, eps = rng.random(N).astype(np.float32), rng.standard_normal((N, R)).astype(np.float32)
    got, comp = draw(st, params, 1, R, N, u=u, eps=eps)
    assert (comp == 0).all() and np.array_equal(got, eps)
    check_parity(st, np.ones(1, np.float32), np.zeros((1, R), np.float32), np.eye(R, dtype=np.float32)[None], seed=R)


def test_sampler_zero_weights_and_boundaries(gpu_ctx, golden_dir):
    st = gpu_ctx.stream
    w, m, c = fixture_mixture(golden_dir, "full")
    w = w.copy()
    zero = np.array([0, 1, 7, 20, 21, 48, 49])
    w[zero] = 0.0
    K, R = m.shape
    params, status = prepare(st, w, m, c)
    assert status == -1
    pos = np.flatnonzero(w > 0)
    rng = np.random.default_rng(5)
    cdf = cdf64(w)
    # uniform draws + the float32 neighbours of every cdf step (where an off-by-one in the search would land on a zero-weight component)
    edges = cdf.astype(np.float32)
    u = np.concatenate([rng.random(N - 3 * K).astype(np.float32), edges, np.nextafter(edges, np.float32(0)), np.nextafter(edges, np.float32(2))])
    u = np.clip(u, 0, np.nextafter(np.float32(1), np.float32(0))).astype(np.float32)
    eps = rng.standard_normal((N, R)).astype(np.float32)
    _, comp = draw(st, params, K, R, N, u=u, eps=eps)
    k, _, _ = restate(w, m, np.linalg.cholesky(c.astype(np.float64)), u, eps)
    assert np.array_equal(comp, k) and not np.isin(comp, zero).any()
    # boundaries: u = 0 -> first component of positive weight; u just below 1 -> last component of positive weight
    ub = np.array([0.0, np.nextafter(np.float32(1), np.float32(0))] * 8, np.float32)
    _, cb = draw(st, params, K, R, 16, u=ub, eps=eps[:16])
    assert (cb[0::2] == pos[0]).all() and (cb[1::2] == pos[-1]).all() and pos[0] == 2 and pos[-1] == 47
    # Philox mode never selects them either
    _, cp = draw(st, params, K, R, 1 << 16, seed=3)
    assert not np.isin(cp, zero).any() and set(np.unique(cp)) <= set(pos)


def test_non_positive_definite_covariance_raises(gpu_ctx, golden_dir):
    from ladder_latent_data_distribution_modelling_amd.engine import LadderEngine
    w, m, c = fixture_mixture(golden_dir, "full")
    bad = c.copy()
    bad[17] = np.array([[1.0, 2.0], [2.0, 1.0]], np.float32)             # indefinite
    bad[31] = 0.0
    _, status = prepare(gpu_ctx.stream, w, m, bad)
    assert status == 17                                                   # the FIRST broken component
    d = np.load(os.path.join(golden_dir, "oracle_mnist_digit.npz"))
    eng = LadderEngine(json.loads(str(d["config"])), "cuda:0", seed=2)
    with pytest.raises(ValueError, match="component 17"):
        eng.prior_sampler("ours", (w, m, bad))
    with pytest.raises(ValueError, match="positive"):
        eng.prior_sampler("ours", (np.zeros_like(w), m, c))
    assert eng.prior_sampler("ours", (w, m, c)).K == 50


# ------------------------------------------------------------------------------------------------ 2. Philox mode
@pytest.mark.parametrize("case", ["full", "wide"])
def test_philox_chunk_independence_seed_and_offset(gpu_ctx, golden_dir, case):
    st = gpu_ctx.stream
    if case == "full":
        w, m, c = fixture_mixture(golden_dir, "full")
    else:
        gm = O.synthetic_gm(dict(n_mixtures=20, representation_size=16), np.random.default_rng(156))
        w, m, c = (gm[k].astype(np.float32) for k in ("weights", "means", "covs"))
    K, R = m.shape
    params, status = prepare(st, w, m, c)
    assert status == -1
    n, first, seed, off = 1000, 12345, 77, 5
    one = draw(st, params, K, R, n, first=first, seed=seed, offset=off)
    for chunk in (128, 500):
        parts = [draw(st, params, K, R, min(chunk, n - lo), first=first + lo, seed=seed, offset=off) for lo in range(0, n, chunk)]
        out, comp = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
        assert np.array_equal(out.view(np.uint32), one[0].view(np.uint32)) and np.array_equal(comp, one[1]), chunk
    again = draw(st, params, K, R, n, first=first, seed=seed, offset=off)
    assert np.array_equal(again[0].view(np.uint32), one[0].view(np.uint32)) and np.array_equal(again[1], one[1])
    other = draw(st, params, K, R, n, first=first, seed=seed, offset=off + 1)
    assert not np.array_equal(other[0], one[0]) and not np.array_equal(other[1], one[1])
    other = draw(st, params, K, R, n, first=first, seed=seed + 1, offset=off)
    assert not np.array_equal(other[0], one[0])
    assert np.isfinite(one[0]).all() and len(np.unique(one[0][:, 0])) > 990                  # distinct draws per sample index


def test_philox_statistics(gpu_ctx, golden_dir):
    st = gpu_ctx.stream
    w, m, c = fixture_mixture(golden_dir, "full")
    K, R = m.shape
    params, status = prepare(st, w, m, c)
    assert status == -1
    n = 1 << 20
    t, comp = draw(st, params, K, R, n, seed=20240607)
    cdf = cdf64(w)
    wk = np.diff(np.concatenate([[0.0], cdf]))
    freq = np.bincount(comp, minlength=K) / n
    live = wk > 0
    assert live.any() and (freq[~live] == 0).all()                       # a zero-weight component is never drawn (and has no sigma)
    z = np.abs(freq[live] - wk[live]) / np.sqrt(wk[live] * (1 - wk[live]) / n)
    print("component frequencies: max %.2f sigma" % z.max())
    assert (z <= 5).all(), z.max()
    chol = np.linalg.cholesky(c.astype(np.float64))
    worst_mean = worst_cov = 0.0
    for k in range(K):
        sel = comp == k
        nk = int(sel.sum())
        if nk < 1000:
            continue
        y = np.linalg.solve(chol[k], (t[sel].astype(np.float64) - m[k].astype(np.float64)).T).T
        dm = np.abs(y.mean(0)).max() * np.sqrt(nk)
        dc = np.abs(np.cov(y.T, bias=True) - np.eye(R)).max() * np.sqrt(nk)
        worst_mean, worst_cov = max(worst_mean, dm), max(worst_cov, dc)
        assert dm <= 5 and dc <= 8, (k, nk, dm, dc)
    print("whitened per-component: mean %.2f / sqrt(n_k), covariance %.2f / sqrt(n_k)" % (worst_mean, worst_cov))


# ------------------------------------------------------------------------------------------------ 3. byte packing
def test_images_to_u8_exact(gpu_ctx):
    L = _L()
    st = gpu_ctx.stream
    n = 128 * 128 * 3 * 5 + 3
    rng = np.random.default_rng(9)
    x = rng.uniform(-0.3, 1.3, n).astype(np.float32)
    ties = ((np.arange(0, 255, dtype=np.float32) + np.float32(0.5)) / np.float32(255)).astype(np.float32)
    ties = ties[(ties * np.float32(255)) % 1 == 0.5]                    # those whose fp32 product IS an exact .5
    assert len(ties) > 50
    x[100:100 + len(ties)] = ties
    x[5000:5006] = [np.nan, np.inf, -np.inf, -0.0, 1.0, 0.0]
    x[-3:] = [0.5, np.nan, 2.0]                                          # the ragged tail
    x[16 * 777 + 3] = np.nan
    finite = np.where(np.isnan(x), np.float32(0), x)                     # NaN -> 0 (stated; a NaN -> uint8 cast is undefined in numpy)
    want = np.rint(np.clip(finite, 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8)
    xd = dev(x)
    out = torch.full((n + 16,), 99, dtype=torch.uint8, device="cuda")
    L.call("ladder_images_to_u8", p(xd), p(out), n, st)
    got = out.cpu().numpy()
    assert np.array_equal(got[:n], want), int((got[:n] != want).sum())
    assert (got[n:] == 99).all()                                         # nothing written past n
    assert set(want[100:100 + len(ties)] % 2) == {0}                     # ties went to even
    assert L.query("ladder_images_to_u8", p(xd) + 4, p(out), 64, st) == E_ALIGN
    assert L.query("ladder_images_to_u8", p(xd), p(out) + 1, 64, st) == E_ALIGN
    assert (out.cpu().numpy()[n:] == 99).all()


# ------------------------------------------------------------------------------------------------ 4. end to end against the oracle
def _tp(P):
    return {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in P.items()}


def _close(a, b, tol=2e-4):
    b = b.numpy() if isinstance(b, torch.Tensor) else np.asarray(b, np.float64)
    err = np.abs(np.asarray(a, np.float64) - b).max()
    return err <= tol * max(1.0, float(np.abs(b).max()))


@pytest.mark.parametrize("exp", ["mnist_digit", "celeba"])
@pytest.mark.parametrize("prior", ["ours", "hierarchical", "GMM", "standard_gaussian", "vampPrior"])
def test_generation_end_to_end_vs_oracle(golden_dir, exp, prior):
    from ladder_latent_data_distribution_modelling_amd.codes import models as M
    from ladder_latent_data_distribution_modelling_amd.codes.base import BaseTrain_joint
    from ladder_latent_data_distribution_modelling_amd.codes.session import Session
    d = np.load(os.path.join(golden_dir, "oracle_%s.npz" % exp))
    cfg = json.loads(str(d["config"]))
    cfg.update(checkpoint_dir="/tmp/", result_dir="/tmp/res/", prior=prior)
    P = O.init_params(cfg, seed=5)
    Pt = _tp(P)
    Model = {"mnist_digit": M.MNISTModel_digit, "celeba": M.CelebAModel_densenet}[exp]
    model = Model(cfg, device="cuda:0", values=P)
    sess = Session()
    tr = BaseTrain_joint(sess, model, None, cfg)
    tr.cur_epoch = 3
    Z, Rt, K = int(cfg["code_size"]), int(cfg["representation_size"]), int(cfg["n_mixtures"])
    n_sample = 6
    n = n_sample ** 2
    rng = np.random.default_rng(11)
    td = lambda a: torch.as_tensor(np.asarray(a, np.float64))

    if prior in ("ours", "GMM"):
        with pytest.raises(RuntimeError, match="not been fitted"):
            tr.generate_samples_from_prior_by_method(mode="crude-GM", n_sample=n_sample)
        R = Rt if prior == "ours" else Z
        if prior == "ours":
            crude = tuple(np.asarray(d[k], np.float32) for k in ("gm_w", "gm_m", "gm_c"))
        else:
            gm = O.synthetic_gm(dict(n_mixtures=K, representation_size=Z), np.random.default_rng(2))
            crude = tuple(gm[k].astype(np.float32) for k in ("weights", "means", "covs"))
        final = (crude[0][::-1].copy(), (crude[1][::-1] + np.float32(0.25)).copy(), crude[2][::-1].copy())      # a different mixture
        tr.gm_params = crude
        with pytest.raises(RuntimeError, match="not been fitted"):
            tr.generate_samples_from_prior_by_method(mode="accurate-GM", n_sample=n_sample)
        tr.gm_final_params = final
        modes = [("crude-GM", crude, "/tmp/res/generated_samples_prior_3_crude-GM.pdf"),
                 ("accurate-GM", final, "/tmp/res/generated_samples_prior_3_accurate-GM.pdf")]
    else:
        R = Rt if prior == "hierarchical" else Z
        modes = [("crude-GM", None, "/tmp/res/generated_samples_prior_3.pdf"), ("accurate-GM", None, "/tmp/res/generated_samples_prior_3.pdf")]
    u = rng.random(n).astype(np.float32)
    eps = rng.standard_normal((n, R)).astype(np.float32)

    for mode, mix, fname in modes:
        code, got_name = tr.generate_samples_from_prior_by_method(mode=mode, n_sample=n_sample, noise={"u": u, "eps": eps})
        assert got_name == fname and code.shape == (n, Z) and code.dtype == np.float32
        if prior in ("ours", "GMM"):
            _, lat, _ = restate(mix[0], mix[1], np.linalg.cholesky(mix[2].astype(np.float64)), u, eps)
        elif prior == "vampPrior":
            ps_in = sess.run(model.psedeu_input)
            cm, cs = sess.run([model.code_mean, model.code_std_dev], feed_dict={model.original_signal: ps_in, model.is_code_input: False,
                                                                               model.code_input: np.zeros((1, Z))})
            assert cm.shape == (K, Z)
            _, lat, _ = restate(np.ones(K, np.float32), cm, np.stack([np.diag(s) for s in cs.astype(np.float64)]), u, eps)
            o_m, o_s = O.encoder(cfg, Pt, td(ps_in))                      # ... and those components are the oracle's
            assert _close(cm, o_m) and _close(cs, o_s)
        else:
            lat = eps.astype(np.float64)
        ref = O.inner_decoder(cfg, Pt, td(lat)).numpy() if prior in ("ours", "hierarchical") else lat
        assert _close(code, ref), np.abs(code - ref).max()
        if prior == "hierarchical":                                        # reference semantics: inner_decoder(t), NOT a plain N(0, I_Z) draw
            assert R < Z and np.abs(code[:, :R] - eps).max() > 1e-2

    # the bulk path on the SAME draws: the sampler's own stream with a fixed seed gives the codes, generate_images decodes them
    code, _ = tr.generate_samples_from_prior_by_method(mode="accurate-GM", n_sample=n_sample, seed=42)
    code2, _ = tr.generate_samples_from_prior_by_method(mode="accurate-GM", n_sample=n_sample, seed=42)
    code3, _ = tr.generate_samples_from_prior_by_method(mode="accurate-GM", n_sample=n_sample)               # no seed: fresh draws per call
    code4, _ = tr.generate_samples_from_prior_by_method(mode="accurate-GM", n_sample=n_sample)
    assert np.array_equal(code, code2) and not np.array_equal(code, code3) and not np.array_equal(code3, code4) and np.isfinite(code).all()
    imgs = tr.generate_images(n, mode="accurate-GM", chunk=16, seed=42)
    assert imgs.shape == (n, cfg["dim_input_x"], cfg["dim_input_y"], cfg["dim_input_channel"]) and imgs.dtype == np.float32
    assert _close(imgs, O.decoder(cfg, Pt, td(code)))

    if prior == "vampPrior":
        s = sess.run(model.psedeu_prior.sample(64))
        assert s.shape == (64, Z) and s.dtype == np.float32 and np.isfinite(s).all()
        assert not np.array_equal(s, sess.run(model.psedeu_prior.sample(64)))                               # fresh draws every run
        u2, eps2 = rng.random(64).astype(np.float32), rng.standard_normal((64, Z)).astype(np.float32)
        fed = sess.run(model.psedeu_prior.sample(64, noise={"u": u2, "eps": eps2}))
        _, lat, bound = restate(np.ones(K, np.float32), cm, np.stack([np.diag(s_) for s_ in cs.astype(np.float64)]), u2, eps2)
        assert _close(fed, lat)
    else:
        assert not hasattr(model, "psedeu_prior")


# ------------------------------------------------------------------------------------------------ 5. bulk path
def test_generate_chunking_bytes_and_restore(golden_dir):
    from ladder_latent_data_distribution_modelling_amd.engine import LadderEngine
    d = np.load(os.path.join(golden_dir, "oracle_celeba.npz"))
    cfg = json.loads(str(d["config"]))
    eng = LadderEngine(cfg, "cuda:0", seed=3)
    sampler = eng.prior_sampler("ours", fixture_mixture(golden_dir, "full"), seed=9)
    drawn = []                                                             # the codes generate() itself decoded, call by call
    sample = sampler.sample

    def recording(n, first=0, **kw):
        r = sample(n, first=first, **kw)
        drawn.append(r[0].cpu().numpy())
        return r

    sampler.sample = recording
    a = eng.generate(300, sampler, chunk=128)
    za, drawn = np.concatenate(drawn), []
    b = eng.generate(300, sampler, chunk=300)
    zb, drawn = np.concatenate(drawn), []
    assert a.shape == b.shape == (300, 128, 128, 3) and a.dtype == np.float32
    assert za.shape == (300, eng.Z) and np.array_equal(za.view(np.uint32), zb.view(np.uint32))
    assert np.array_equal(zb, sample(300)[0].cpu().numpy())
    assert np.abs(a - b).max() <= 2e-4 * max(1.0, float(np.abs(b).max()))
    q = eng.generate(300, sampler, chunk=128, as_uint8=True)
    assert q.dtype == np.uint8 and np.array_equal(q, np.rint(np.clip(a, 0, 1).astype(np.float32) * np.float32(255)).astype(np.uint8))
    assert len(np.unique(q)) > 20                                           # real images, not a constant
    # `first` continues the same stream: samples 100 .. 299 of the run above
    drawn.clear()
    c = eng.generate(200, sampler, chunk=128, first=100)
    assert np.array_equal(np.concatenate(drawn), za[100:])                # `first` continues the same stream
    assert np.abs(c - a[100:]).max() <= 2e-4 * max(1.0, float(np.abs(a).max()))
    assert eng.generate(0, sampler).shape == (0, 128, 128, 3)
    assert eng.ctx.keep_activations is True
    with pytest.raises(ValueError):
        eng.generate(4, sampler, chunk=0)
    assert eng.ctx.keep_activations is True


@pytest.mark.parametrize("flags,dtype", [((), np.float32), (("--uint8",), np.uint8)])
def test_generate_cli_writes_sampled_images(tmp_path, golden_dir, flags, dtype):
    """generate.py as a fresh child process, the way a user runs it (no checkpoint in the scratch directory: the freshly initialised model)."""
    cfg = json.load(open(os.path.join(ROOT, "codes", "mnist_digit_config.json")))
    cfg.update(num_hidden_units=64, num_hidden_units_inner_VAE=32, n_layers_inner_VAE=2, batch_size=64)
    cpath = str(tmp_path / "mnist_digit_config.json")
    json.dump(cfg, open(cpath, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    outp = str(tmp_path / "gen.npz")
    cmd = [sys.executable, os.path.join(ROOT, "generate.py"), "--config", cpath, "--n", "70", "--chunk", "32", "--out", outp, "--seed", "4",
           "--gm", os.path.join(golden_dir, "GM_prior_info.npz")] + list(flags)
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = np.load(outp)
    assert r.files == ["sampled_images"]
    imgs = r["sampled_images"]
    assert imgs.shape == (70, 28, 28, 1) and imgs.dtype == dtype and np.isfinite(imgs.astype(np.float64)).all()
    assert len(np.unique(imgs[0])) > 1 and not np.array_equal(imgs[0], imgs[1])
    # without a mixture archive the command says what is missing
    if not flags:
        miss = subprocess.run(cmd[:-2], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
        assert miss.returncode != 0 and "no fitted mixture" in miss.stderr


# ------------------------------------------------------------------------------------------------ 6. training is untouched
def test_generation_leaves_training_bit_identical(golden_dir):
    from ladder_latent_data_distribution_modelling_amd.engine import LadderEngine
    d = np.load(os.path.join(golden_dir, "oracle_mnist_digit.npz"))
    cfg = json.loads(str(d["config"]))
    P = O.init_params(cfg, seed=5)
    x = d["x"]
    gm = (d["gm_w"], d["gm_m"], d["gm_c"])

    def iteration(eng):
        got = []
        for kind, lr in (("ae", 3e-4), ("sigma", 5e-4), ("prior", 2e-4), ("inner_sigma", 1e-4)):
            getattr(eng, "run_" + kind)(x, lr, None, False, False)
            got.append(eng.fetch())
        return got

    a, b = (LadderEngine(cfg, "cuda:0", values=P, noise_seed=99) for _ in range(2))
    for eng in (a, b):
        eng.set_mixture(*gm)
    fa = iteration(a) + iteration(a)
    fb = iteration(b)
    counter = int(b.rng_counter.item())
    imgs = b.generate(256, b.prior_sampler("ours", fixture_mixture(golden_dir, "full"), seed=1), chunk=100)
    assert imgs.shape == (256, 28, 28, 1) and np.isfinite(imgs).all()
    assert int(b.rng_counter.item()) == counter
    fb += iteration(b)
    for ra, rb in zip(fa, fb):
        assert ra.keys() == rb.keys()
        for k in ra:
            assert ra[k] == rb[k] or (np.isnan(ra[k]) and np.isnan(rb[k])), k
    pa, pb = a.ps.to_dict(), b.ps.to_dict()
    assert pa.keys() == pb.keys() and all(np.array_equal(pa[k], pb[k]) for k in pa)
