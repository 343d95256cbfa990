"""oracle/elbo_ref.py against what it must not drift from: the published Philox known answers and `ladder_oracle.forward`.

tests/test_gpu_elbo_kernels.py checks the ELBO-side kernels against oracle/elbo_ref.py; this file is what keeps that reference
from being a restatement of the kernels.
"""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import elbo_ref as E
from oracle import ladder_oracle as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))


# Known-answer vectors of Random123 (its kat_vectors file, lines "philox4x32 10": counter words, key words, expected words).
PHILOX_KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", PHILOX_KAT, ids=["zero", "ones", "pi"])
def test_philox_known_answer(ctr, key, want):
    got = E.philox4x32_10(np.array(ctr, np.uint64), key[0] | (key[1] << 32))
    assert tuple(int(w) for w in got) == want
    # the vectorised form (a leading axis of counters) gives the same words
    both = E.philox4x32_10(np.array([ctr, PHILOX_KAT[0][0]], np.uint64), key[0] | (key[1] << 32))
    assert tuple(int(w) for w in both[0]) == want


def test_randn_ref_layout_and_rounding():
    """Block q gives values 4q .. 4q+3, a prefix does not depend on n, and the offset's high word is part of the counter."""
    a = E.randn_ref(64, 42, 0)
    assert np.array_equal(E.randn_ref(13, 42, 0), a[:13])
    w = E.philox4x32_10(np.array([3, 0, 5, 1], np.uint64), 42)
    u1, u2 = E._unit_open(w[0:1]), E._unit_open(w[1:2])
    r = np.sqrt(-2.0 * np.log(np.float64(u1[0])))
    b = E.randn_ref(16, 42, 5 + 2 ** 32)
    assert b[12] == r * np.cos(np.float64(np.float32(6.2831855) * u2[0]))
    assert not np.array_equal(b, E.randn_ref(16, 42, 5))
    # a word >= 2^31: (w >> 8) + 0.5 is not representable in fp32 and rounds to even
    assert E._unit_open(np.array([0xFFFFFFFF], np.uint64))[0] == np.float32(1.0)
    assert E._unit_open(np.array([0x80000100], np.uint64))[0] == np.float32((2 ** 23 + 2) * 2.0 ** -24)
    assert E._unit_open(np.array([0], np.uint64))[0] == np.float32(2.0 ** -25)
    x = E.randn_ref(1 << 16, 7, 0)
    assert abs(x.mean()) < 0.02 and abs(x.var() - 1) < 0.03


def test_adam_lr_t_rounds_the_decay_rates():
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.95))
    assert E.adam_lr_t(3e-4, 0.9, 0.95, 3) == 3e-4 * np.sqrt(1 - b2 ** 3) / (1 - b1 ** 3)
    assert E.adam_lr_t(3e-4, 0.9, 0.95, 3) != 3e-4 * np.sqrt(1 - 0.95 ** 3) / (1 - 0.9 ** 3)


def _rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


def _f(t):
    return float(t.detach())


CASES = [(prior, use_sg, use_mask, sigma0)
         for prior in ("ours", "hierarchical") for use_sg in (True, False)
         for use_mask in ((False, True) if prior == "ours" else (False,))
         for sigma0 in (0.5, 0.01)]


@pytest.mark.parametrize("prior,use_sg,use_mask,sigma0", CASES)
def test_elbo_scalars_agree_with_oracle_forward(golden_dir, prior, use_sg, use_mask, sigma0):
    """Partials formed from ladder_oracle.forward's own tensors, fed to elbo_scalars: every scalar to 1e-12 relative, the four
    backward coefficients to 1e-10 against autograd through forward itself.  sigma0 = 0.5 / 0.01 puts sigma on either side of the
    mean pixel error; the configuration's inner sigma sits exactly on its upper clamp bound."""
    from make_golden import tiny_config
    cfg = tiny_config("mnist_digit")
    cfg.update(prior=prior, sigma=sigma0)
    if prior == "hierarchical":
        cfg.update(representation_size=3)
    B, Z, R, L = 4, int(cfg["code_size"]), int(cfg["representation_size"]), int(cfg["n_MC_samples"])
    D = 28 * 28
    rng = np.random.default_rng(11)
    x = torch.tensor(rng.random((B, 28, 28, 1)), dtype=torch.float64)
    params = O.init_params(cfg, seed=5)
    params["encoder/code_std_dev/bias"] = params["encoder/code_std_dev/bias"] + np.float32(1.0)   # sd_z on both sides of the mask's 1
    st = O.OracleState(cfg, params, np.float64)
    P = st.torch_params(("ae", "prior", "sigma", "inner_sigma"))
    nz = {k: torch.tensor(v) for k, v in O.make_noise(cfg, B, rng).items()}
    gm = None
    if prior == "ours":
        fix = np.load(os.path.join(golden_dir, "GM_prior_info.npz"))
        gm = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in O.synthetic_gm(cfg, fixture=fix).items()}
    out = O.forward(cfg, P, x, nz["eps_z"], nz["eps_t"], nz["eps_mc"], gm, use_sg=use_sg, use_mask=use_mask)

    mu_z, sd_z, z, xhat = out["code_mean"], out["code_std_dev"], out["code_sample"], out["decoded"]
    mu_t, sd_t, zhat = out["representation_mean"], out["representation_std_dev"], out["decoded_code"]
    masked = use_mask and prior == "ours"
    if masked:
        assert bool((sd_z > 1).any()) and bool((sd_z <= 1).any())
    err = (z - zhat) ** 2
    if masked:
        err = torch.where(sd_z > 1.0, torch.zeros_like(err), err)
    Pv = np.zeros(E.P_FIXED)
    Pv[E.P_PIX_ABS] = _f((x - xhat).abs().sum())
    Pv[E.P_PIX_SQ] = _f(((x - xhat) ** 2).sum())
    Pv[E.P_LOG_SDZ] = _f(torch.log(sd_z).sum())
    Pv[E.P_MU2SD2_Z] = _f((mu_z ** 2 + sd_z ** 2).sum())
    Pv[E.P_CODE_ERR] = _f(err.sum())
    Pv[E.P_CODE_SQRT] = _f(torch.sqrt(err).sum())
    Pv[E.P_CODE_ABS] = _f((z - zhat).abs().sum())
    Pv[E.P_LOG_SDT] = _f(torch.log(sd_t).sum())
    Pv[E.P_MU2SD2_T] = _f((mu_t ** 2 + sd_t ** 2).sum())
    if prior == "ours":
        t_mc = mu_t.unsqueeze(0) + sd_t.unsqueeze(0) * nz["eps_mc"]
        Pv[E.P_LOGP] = _f(O.gmm_log_prob(t_mc, gm["weights"], gm["means"], gm["covs"]).sum())
    ecfg = dict(B_global=B, D=D, Z=Z, R=R, L=L, sigma_uses_mpe=1, has_inner=1, use_sg=int(use_sg),
                clamp_inner_sigma=int(cfg["TRAIN_inner_sigma"]), inner_sigma_lb=cfg["inner_sigma_lb"], inner_sigma_ub=cfg["inner_sigma_ub"],
                hierarchical=int(prior == "hierarchical"), prior_gmm=0)
    S = E.elbo_scalars(Pv, _f(P["sigma/Variable"]), _f(P["inner_sigma/Variable"]), ecfg)

    assert set(S) == set(range(26))
    for slot, key in E.S_ORACLE_KEY.items():
        assert _rel(S[slot], _f(out[key])) <= 1e-12, (key, S[slot], _f(out[key]))
    assert (S[E.S_SIGMA] == _f(out["mean_pixel_error"])) == (sigma0 == 0.01)       # both sides of the maximum are visited
    assert S[E.S_INV_B] == 1.0 / B and S[E.S_INV_LB] == 1.0 / (L * B)

    def tol(a, b):
        return abs(a - b) <= 1e-10 * max(1.0, abs(b))
    g_sig, g_xhat = torch.autograd.grad(out["loss_ae"], [P["sigma/Variable"], xhat], retain_graph=True)
    g_isv, g_zhat = torch.autograd.grad(out["loss_prior"], [P["inner_sigma/Variable"], zhat], retain_graph=True)
    assert tol(S[E.S_G_SIGMA_VAR], _f(g_sig))
    assert tol(S[E.S_G_INNER_SIGMA_VAR], _f(g_isv))
    assert (_f(g_sig) == 0.0) == (sigma0 == 0.01) and _f(g_isv) != 0.0
    sgn = torch.sign(xhat - x)
    count = _f((sgn != 0).sum())
    assert tol(S[E.S_G_PIX], _f((g_xhat * sgn).sum()) / count)
    assert _f((g_xhat - S[E.S_G_PIX] * sgn).abs().max()) <= 1e-10 * abs(S[E.S_G_PIX])
    # d loss_prior / d zhat = -2 G_CODE (z - zhat) mask
    d = (z - zhat) * (err != 0)
    assert tol(S[E.S_G_CODE], _f((g_zhat * -d).sum()) / _f(2.0 * (d * d).sum()))
    _, dzhat = E.code_grad_ref(z.detach().numpy(), zhat.detach().numpy(), sd_z.detach().numpy(), masked, S[E.S_G_CODE])
    assert np.abs(dzhat - g_zhat.detach().numpy()).max() <= 1e-10 * max(1.0, np.abs(dzhat).max())
    cp = E.code_partials_ref(z.detach().numpy(), zhat.detach().numpy(), sd_z.detach().numpy(), masked)
    assert _rel(cp[0], Pv[E.P_CODE_ERR]) <= 1e-12 and _rel(cp[2], Pv[E.P_CODE_ABS]) <= 1e-12


def test_elbo_scalars_without_inner_vae():
    """standard_gaussian and the mixture-on-z route: no inner slots, crossEntropy_prior routed as ladder_oracle.forward does."""
    Pv = np.arange(1.0, 17.0)
    base = dict(B_global=5, D=12, Z=4, R=2, L=9, sigma_uses_mpe=0, has_inner=0, use_sg=1, clamp_inner_sigma=0, inner_sigma_lb=0.0,
                inner_sigma_ub=0.0, hierarchical=0, prior_gmm=0)
    S = E.elbo_scalars(Pv, -0.7, None, base)
    assert set(S) == set(range(11)) | set(range(20, 26))
    assert S[E.S_XENT_PRIOR] == S[E.S_XENT_SG] and S[E.S_G_CODE] == 0.0 and S[E.S_G_INNER_SIGMA_VAR] == 0.0
    assert S[E.S_SIGMA] == 0.7 and S[E.S_G_SIGMA_VAR] != 0.0
    # sigma = |v|: the derivative w.r.t. a negative variable has the opposite sign of the one w.r.t. its mirror image
    assert S[E.S_G_SIGMA_VAR] == -E.elbo_scalars(Pv, 0.7, None, base)[E.S_G_SIGMA_VAR]
    G = E.elbo_scalars(Pv, -0.7, None, dict(base, prior_gmm=1))
    assert G[E.S_XENT_PRIOR] == Pv[E.P_LOGP] / (9 * 5) and G[E.S_XENT_SG] == S[E.S_XENT_SG]


def test_latent_refs_against_autograd():
    """latent_bwd_terms is the autograd gradient of the three terms a latent block feeds: a downstream loss through the sample, the
    entropy term -sum log sd / B (mode bit 0) and the standard-Gaussian cross-entropy 0.5 sum (mu^2 + sd^2) / B (mode bit 1)."""
    rng = np.random.default_rng(0)
    B, Z, lvp = 3, 5, 2.0 ** -10
    mu, sd_raw, eps, g, em, es = (rng.standard_normal((B, Z)).astype(np.float32) for _ in range(6))
    sd_raw[0, 0] = 0.0
    f = E.latent_fwd_ref(mu, np.maximum(sd_raw, 0), eps, lvp)
    assert f["sd"].dtype == np.float32 and np.array_equal(f["sd"], np.maximum(sd_raw, 0) + np.float32(lvp))
    inv_B, inv_LB = 1.0 / 6, 1.0 / 42
    for mode in range(4):
        mt = torch.tensor(mu, dtype=torch.float64, requires_grad=True)
        rt = torch.tensor(sd_raw, dtype=torch.float64, requires_grad=True)
        sd = torch.where(rt > 0, rt, torch.zeros_like(rt)) + lvp          # tf.nn.relu: no gradient at exactly 0
        zz = mt + sd * torch.tensor(eps, dtype=torch.float64)
        loss = (zz * torch.tensor(g, dtype=torch.float64)).sum()
        if mode & 1:
            loss = loss - torch.log(sd).sum() * inv_B
        if mode & 2:
            loss = loss + 0.5 * (mt ** 2 + sd ** 2).sum() * inv_B
        loss = loss - inv_LB * ((mt * torch.tensor(em, dtype=torch.float64)).sum() + (sd * torch.tensor(es, dtype=torch.float64)).sum())
        loss.backward()
        dmu, dsd_raw, am, asd = E.latent_bwd_terms(g, mu, sd.detach().numpy(), sd_raw, eps, em, es, -1.0, inv_B, inv_LB, mode)
        assert np.abs(dmu - mt.grad.numpy()).max() < 1e-13 and np.abs(dsd_raw - rt.grad.numpy()).max() < 1e-11
        assert dsd_raw[0, 0] == 0.0 and (am >= np.abs(dmu) - 1e-15).all() and (asd >= np.abs(dsd_raw) - 1e-12).all()
