"""Float64 references for the kernels between the encoder output and the optimiser step.  TEST INFRASTRUCTURE ONLY.

What is here restates, in plain numpy / torch-CPU float64, the operations that `csrc/elbo.hip` runs on the device: the scalar
algebra of define_loss on a vector of partial sums, the latent block and its gradient, the code terms, the Philox4x32-10 normal
generator and the device-side Adam learning rate.  It is written from `oracle/ladder_oracle.py:forward` (the sigma block, the
prior routing and the ELBO terms, lines 520-601) and from the slot definitions of `include/ladder_hip.h`, never from the kernels;
`tests/test_elbo_ref_cpu.py` ties `elbo_scalars` back to `ladder_oracle.forward` and the generator to a published known answer,
so that the GPU tests that use this module do not compare the kernels with a copy of themselves.

Nothing here imports the HIP library or its binding.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from oracle import ladder_oracle as O

# partial-sum and scalar slots: include/ladder_hip.h (LADDER_P_*, LADDER_S_*)
P_PIX_ABS, P_PIX_SQ, P_LOG_SDZ, P_MU2SD2_Z, P_CODE_ERR, P_CODE_SQRT, P_CODE_ABS, P_LOG_SDT, P_MU2SD2_T, P_LOGP = range(10)
P_FIXED = 16
(S_SIGMA, S_MPE, S_ENTROPY_Z, S_XENT_SG, S_XENT_PRIOR, S_L1, S_L2, S_RECON_LL, S_SIGMA_REG, S_ELBO, S_LOSS_AE,
 S_INNER_SIGMA, S_MEAN_CODE_ERROR, S_CODE_LL, S_CODE_L1, S_REP_REG, S_ENTROPY_T, S_XENT_T, S_ELBO_PRIOR, S_LOSS_PRIOR,
 S_G_PIX, S_G_SIGMA_VAR, S_G_CODE, S_G_INNER_SIGMA_VAR, S_INV_B, S_INV_LB) = range(26)
S_COUNT = 32

# scalar slot -> key of the dict ladder_oracle.forward returns
S_ORACLE_KEY = {
    S_SIGMA: "sigma", S_MPE: "mean_pixel_error", S_ENTROPY_Z: "entropy_z", S_XENT_SG: "crossEntropy_prior_sg",
    S_XENT_PRIOR: "crossEntropy_prior", S_L1: "l1_reconstruction_error", S_L2: "l2_reconstruction_error",
    S_RECON_LL: "reconstruction_likelihood", S_SIGMA_REG: "sigma_regularisor", S_ELBO: "elbo", S_LOSS_AE: "loss_ae",
    S_INNER_SIGMA: "inner_sigma", S_MEAN_CODE_ERROR: "mean_code_error", S_CODE_LL: "code_reconstruction_likelihood",
    S_CODE_L1: "code_l1_reconstruction_error", S_REP_REG: "representation_regularisor", S_ENTROPY_T: "entropy_t",
    S_XENT_T: "crossEntropy_representation", S_ELBO_PRIOR: "elbo_prior", S_LOSS_PRIOR: "loss_prior",
}

_DT = torch.float64


def _grad(y, x):
    """d y / d x by autograd; 0 where y does not depend on x."""
    if not y.requires_grad:
        return torch.zeros_like(x)
    g, = torch.autograd.grad(y, x, retain_graph=True, allow_unused=True)
    return torch.zeros_like(x) if g is None else g


def elbo_scalars(P, sigma_var, inner_sigma_var, cfg):
    """The scalars of one step from the GLOBAL partial sums `P` ([LADDER_P_*] slots, any float type: used as float64), the two
    trainable scales and `cfg`, a mapping with the fields of LadderElboCfg (B_global, D, Z, R, L, sigma_uses_mpe, has_inner, use_sg,
    clamp_inner_sigma, inner_sigma_lb, inner_sigma_ub, hierarchical, prior_gmm).  Returns {slot: float64} with only the slots the
    chosen branch defines: the inner-VAE scalars (slots 11-19) are absent without an inner VAE.

    Every batch mean is over B_global samples (ladder_oracle.forward's `Bg`); per-sample constants therefore enter once.
    The four backward coefficients are autograd derivatives of the two losses:
      G_PIX = d loss_ae / d P[PIX_ABS]  (so that d loss_ae / d xhat = G_PIX * sign(xhat - x)),
      G_SIGMA_VAR = d loss_ae / d sigma_var,  G_CODE = d loss_prior / d P[CODE_ERR],  G_INNER_SIGMA_VAR = d loss_prior / d inner_sigma_var;
    without an inner VAE there is no loss_prior term here and the last two are the derivative of nothing: 0.
    INV_B = 1 / B_global and INV_LB = 1 / (L * B_global)."""
    B, D, Z, R, L = (float(cfg[k]) for k in ("B_global", "D", "Z", "R", "L"))
    has_inner, hier, gmm_z = bool(cfg["has_inner"]), bool(cfg["hierarchical"]), bool(cfg["prior_gmm"])
    assert not (has_inner and gmm_z), "the mixture sits either on t (inner VAE) or on z, never both"
    Pt = torch.tensor(np.asarray(P, np.float64), dtype=_DT, requires_grad=True)
    sv = torch.tensor(float(sigma_var), dtype=_DT, requires_grad=True)
    out = {}

    # sigma block (forward:520-527)
    sigma = torch.abs(sv)                                      # sqrt(v * v)
    mpe = Pt[P_PIX_ABS] / (B * D)
    if cfg["sigma_uses_mpe"]:
        sigma = O.tf_maximum(sigma, mpe)
    out[S_SIGMA], out[S_MPE] = sigma, mpe

    # (forward:530-532) sum_b [-Z/2 log 2pi - Z/2 - sum_j log sd] / B and the closed-form cross-entropy against N(0, I)
    out[S_ENTROPY_Z] = -0.5 * Z * O.LOG_2PI - 0.5 * Z - Pt[P_LOG_SDZ] / B
    out[S_XENT_SG] = -0.5 * Z * O.LOG_2PI - 0.5 * Pt[P_MU2SD2_Z] / B

    iv = None
    if gmm_z:                                                  # (forward:549-553; the VampPrior's mixture term takes the same route)
        out[S_XENT_PRIOR] = Pt[P_LOGP] / (L * B)
    elif has_inner:                                            # (forward:554-588)
        iv = torch.tensor(float(inner_sigma_var), dtype=_DT, requires_grad=True)
        inner_sigma = torch.abs(iv)
        if cfg["clamp_inner_sigma"]:
            inner_sigma = O.tf_minimum(O.tf_maximum(inner_sigma, O.f32c(cfg["inner_sigma_lb"], _DT)),
                                       O.f32c(cfg["inner_sigma_ub"], _DT))
        out[S_INNER_SIGMA] = inner_sigma
        out[S_MEAN_CODE_ERROR] = Pt[P_CODE_ABS] / (B * Z)
        out[S_CODE_LL] = -(Pt[P_CODE_ERR] / (2.0 * inner_sigma ** 2)) / B
        out[S_CODE_L1] = Pt[P_CODE_SQRT] / B
        out[S_REP_REG] = -Z * torch.log(inner_sigma) - 0.5 * Z * O.LOG_2PI
        Re = 2.0 if hier else R
        out[S_ENTROPY_T] = -0.5 * Re * O.LOG_2PI - 0.5 * Re - Pt[P_LOG_SDT] / B
        if hier:
            out[S_XENT_T] = -0.5 * R * O.LOG_2PI - 0.5 * Pt[P_MU2SD2_T] / B
        else:
            out[S_XENT_T] = Pt[P_LOGP] / (L * B)
        out[S_ELBO_PRIOR] = out[S_CODE_LL] + out[S_REP_REG] - out[S_ENTROPY_T] + out[S_XENT_T]
        out[S_XENT_PRIOR] = out[S_XENT_SG] if cfg["use_sg"] else out[S_ELBO_PRIOR]
        out[S_LOSS_PRIOR] = -out[S_ELBO_PRIOR]
    else:                                                      # (forward:535-536)
        out[S_XENT_PRIOR] = out[S_XENT_SG]

    # (forward:592-599)
    out[S_L2] = Pt[P_PIX_SQ] / B
    out[S_L1] = Pt[P_PIX_ABS] / B
    out[S_RECON_LL] = -(Pt[P_PIX_ABS] / B) / sigma
    out[S_SIGMA_REG] = -D * torch.log(2.0 * sigma)
    out[S_ELBO] = out[S_RECON_LL] + out[S_SIGMA_REG] - out[S_ENTROPY_Z] + out[S_XENT_PRIOR]
    out[S_LOSS_AE] = -out[S_ELBO]

    res = {k: float(v.detach()) for k, v in out.items()}
    res[S_G_PIX] = float(_grad(out[S_LOSS_AE], Pt)[P_PIX_ABS])
    res[S_G_SIGMA_VAR] = float(_grad(out[S_LOSS_AE], sv))
    if has_inner:
        res[S_G_CODE] = float(_grad(out[S_LOSS_PRIOR], Pt)[P_CODE_ERR])
        res[S_G_INNER_SIGMA_VAR] = float(_grad(out[S_LOSS_PRIOR], iv))
    else:
        res[S_G_CODE] = res[S_G_INNER_SIGMA_VAR] = 0.0
    res[S_INV_B] = 1.0 / B
    res[S_INV_LB] = 1.0 / (L * B)
    return res


# ---------------------------------------------------------------------------------------------- latent block, code terms
def latent_fwd_ref(mu, sd_raw, eps, lvp):
    """The latent block on fp32 heads (models.py:95-103): sd = sd_raw + lvp is an fp32 TENSOR of the graph (one fp32 addition of the
    fp32 constant), everything after it is evaluated in float64 on that tensor.  Returns dict(sd [fp32], z, p_log, p_mu2sd2, p_sdsum)."""
    mu, sd_raw, eps = (np.asarray(a, np.float32) for a in (mu, sd_raw, eps))
    sd = sd_raw + np.float32(lvp)
    assert sd.dtype == np.float32
    s64, m64 = sd.astype(np.float64), mu.astype(np.float64)
    return dict(sd=sd, z=m64 + s64 * eps.astype(np.float64), p_log=np.log(s64).sum(), p_mu2sd2=(m64 * m64 + s64 * s64).sum(),
                p_sdsum=s64.sum(0))


def latent_bwd_terms(g_sample, mu, sd, sd_raw, eps, extra_mu, extra_sd, extra_sign, inv_B, inv_LB, mode):
    """The gradient of a reparameterised latent block w.r.t. its heads, term by term (include/ladder_hip.h, ladder_latent_bwd):
      dmu = g_sample [+ mu * INV_B if mode & 2] + extra_sign * INV_LB * extra_mu
      dsd = g_sample * eps [- INV_B / sd if mode & 1] [+ sd * INV_B if mode & 2] + extra_sign * INV_LB * extra_sd
      dsd_raw = dsd * (sd_raw > 0)
    Returns (dmu, dsd_raw, sum |term| of dmu, sum |term| of dsd), all float64; absent inputs are None."""
    f = lambda a: None if a is None else np.asarray(a, np.float64)
    g_sample, mu, sd, sd_raw, eps, extra_mu, extra_sd = map(f, (g_sample, mu, sd, sd_raw, eps, extra_mu, extra_sd))
    tm, ts = [], []
    if g_sample is not None:
        tm.append(g_sample)
        ts.append(g_sample * eps)
    if mode & 1:
        ts.append(-inv_B / sd)
    if mode & 2:
        tm.append(mu * inv_B)
        ts.append(sd * inv_B)
    if extra_mu is not None:
        tm.append(extra_sign * inv_LB * extra_mu)
        ts.append(extra_sign * inv_LB * extra_sd)
    zero = np.zeros_like(mu)
    dmu, dsd = sum(tm, zero), sum(ts, zero)
    return dmu, np.where(sd_raw > 0, dsd, 0.0), sum((np.abs(t) for t in tm), zero), sum((np.abs(t) for t in ts), zero)


def _code_err(z, zhat, sd_z, use_mask):
    err = (z - zhat) ** 2                                       # (forward:569-571)
    if use_mask:
        err = torch.where(sd_z > 1.0, torch.zeros_like(err), err)
    return err


def code_partials_ref(z, zhat, sd_z, use_mask):
    """(sum err, sum sqrt(err), sum |z - zhat|) with err = (z - zhat)^2, 0 where use_mask and sd_z > 1; the last ignores the mask."""
    z, zhat, sd_z = (torch.tensor(np.asarray(a, np.float64)) for a in (z, zhat, sd_z))
    err = _code_err(z, zhat, sd_z, use_mask)
    return float(err.sum()), float(torch.sqrt(err).sum()), float((zhat - z).abs().sum())


def code_grad_ref(z, zhat, sd_z, use_mask, g_code):
    """(d/dz, d/dzhat) of g_code * sum err, by autograd."""
    z, zhat, sd_z = (torch.tensor(np.asarray(a, np.float64)) for a in (z, zhat, sd_z))
    z.requires_grad_(True)
    zhat.requires_grad_(True)
    (float(g_code) * _code_err(z, zhat, sd_z, use_mask).sum()).backward()
    return z.grad.numpy(), zhat.grad.numpy()


# ---------------------------------------------------------------------------------------------- Philox4x32-10 normals
_M32 = np.uint64(0xFFFFFFFF)
_PHILOX_M0, _PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)      # Salmon et al., "Parallel random numbers: as easy as 1, 2, 3" (SC'11)
_PHILOX_W0, _PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)      # key increments: golden ratio, sqrt(3) - 1


def philox4x32_10(counter4, seed):
    """Philox4x32 with ten rounds.  counter4: [..., 4] words (low word first); seed: the 64-bit key {low, high}.  Returns [..., 4] uint64
    holding 32-bit values."""
    c = np.asarray(counter4, np.uint64) & _M32
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    seed = int(seed)
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = _PHILOX_M0 * c0, _PHILOX_M1 * c2                          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + _PHILOX_W0) & _M32, (k1 + _PHILOX_W1) & _M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def _unit_open(w):
    """A 32-bit word -> (0, 1]: (float32(w >> 8) + 0.5) * 2^-24 evaluated in fp32, so that the addition rounds (to even) for words
    >= 2^31 exactly as an fp32 implementation's does."""
    a = (w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)
    u = a * np.float32(2.0 ** -24)
    assert u.dtype == np.float32
    return u


def randn_ref(n, seed, offset, with_radius=False):
    """n standard normals of the stream (seed, offset): block q uses the counter {q low, q high, offset low, offset high} and gives four
    values: words (0, 1) and (2, 3) each make r = sqrt(-2 log u1), angle = float32(2 pi) * u2 -> (r cos, r sin).  The uniforms and the angle are
    fp32 quantities (the argument roundings are part of the definition); log, sqrt, sin, cos are float64."""
    n, offset = int(n), int(offset)
    nq = (n + 3) // 4
    q = np.arange(nq, dtype=np.uint64)
    ctr = np.stack([q & _M32, q >> np.uint64(32), np.full(nq, offset & 0xFFFFFFFF, np.uint64),
                    np.full(nq, (offset >> 32) & 0xFFFFFFFF, np.uint64)], axis=-1)
    w = philox4x32_10(ctr, seed)
    out, rad = np.empty((nq, 4), np.float64), np.empty((nq, 4), np.float64)
    for p in range(2):
        u1, u2 = _unit_open(w[:, 2 * p]), _unit_open(w[:, 2 * p + 1])
        ang = np.float32(6.2831855) * u2
        assert ang.dtype == np.float32
        r = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
        a64 = ang.astype(np.float64)
        out[:, 2 * p], out[:, 2 * p + 1] = r * np.cos(a64), r * np.sin(a64)
        rad[:, 2 * p] = rad[:, 2 * p + 1] = r
    out, rad = out.reshape(-1)[:n], rad.reshape(-1)[:n]
    return (out, rad) if with_radius else out


# ---------------------------------------------------------------------------------------------- Adam
def adam_lr_t(lr, b1, b2, t):
    """TF-form step size lr * sqrt(1 - b2^t) / (1 - b1^t) with the decay rates as the C ABI carries them: rounded to float32."""
    b1, b2 = float(np.float32(b1)), float(np.float32(b2))
    return float(lr) * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def adam_step_ref(theta, g, m, v, lr_t, b1, b2, eps, clip):
    """One clip + Adam step (ladder_oracle.adam_tf) in float64 from the given state; b1, b2, eps, clip rounded to float32 as the C ABI
    carries them.  Returns (theta', m', v') and the two terms of m' (for error bounds)."""
    theta, g, m, v = (np.asarray(a, np.float64) for a in (theta, g, m, v))
    b1, b2, eps, clip = (float(np.float32(a)) for a in (b1, b2, eps, clip))
    g = np.clip(g, -clip, clip)
    t1, t2 = b1 * m, (1.0 - b1) * g
    m1 = t1 + t2
    v1 = b2 * v + (1.0 - b2) * g * g
    return theta - lr_t * m1 / (np.sqrt(v1) + eps), m1, v1, (t1, t2)
