"""Float64 reference of the importance-weighted log-likelihood (DESIGN.md "Importance-weighted log-likelihood"), composed from the oracle's networks:
`encoder`, `decoder`, `inner_encoder`, `inner_decoder`, `gmm_log_prob` of oracle/ladder_oracle.py.  Restates the definition, and the VampPrior row
density as O.forward writes it.

A batch of B images is encoded once (batch statistics of that batch); sample s of image b is z = mu_z[b] + sd_z[b] * eps_z[s, b] and

    standard_gaussian, GMM, vampPrior   log w = log p(x|z) + log p(z) - log q(z|x)
    ours, hierarchical                  t = mu_t(z) + sd_t(z) * eps_t[s, b]
                                        log w = log p(x|z) + log N(z; inner_decoder(t), inner_sigma^2 I) + log p(t) - log q(z|x) - log q(t|z)

    log p(x|z) = -sum_d |x_d - xhat_d| / sigma - D log(2 sigma), sigma a fixed number.
"""
import math

import numpy as np
import torch

from oracle import ladder_oracle as O

LOG_2PI = math.log(2.0 * math.pi)
SIGNS = {"log_px_z": 1.0, "log_pz": 1.0, "log_pt": 1.0, "log_qz": -1.0, "log_qt": -1.0}


def _normal_logpdf(a, b, s):
    """log N(a; b, s^2 I) over the last axis."""
    W = a.shape[-1]
    return -((a - b) ** 2).sum(-1) / (2.0 * s * s) - W * math.log(s) - 0.5 * W * LOG_2PI


def _logq(eps, sd):
    """log-density of mu + sd * eps under N(mu, diag sd^2)."""
    W = eps.shape[-1]
    return -0.5 * (eps ** 2).sum(-1) - torch.log(sd).sum(-1) - 0.5 * W * LOG_2PI


def inner_sigma(cfg, P):
    s = abs(float(np.asarray(P["inner_sigma/Variable"], np.float64).reshape(-1)[0]))
    if int(cfg["TRAIN_inner_sigma"]) == 1:
        s = min(max(s, float(np.float32(cfg["inner_sigma_lb"]))), float(np.float32(cfg["inner_sigma_ub"])))
    return s


def terms(cfg, params, x, eps_z, eps_t=None, gm=None, sigma=None):
    """-> dict of float64 arrays [B, S]: the term vectors present for cfg["prior"], "logw", and "z" [B, S, Z].  eps_z [S, B, Z], eps_t [S, B, R]."""
    dt = torch.float64
    P = {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in params.items()}
    x = torch.as_tensor(np.asarray(x, np.float64))
    eps_z = torch.as_tensor(np.asarray(eps_z, np.float64)).permute(1, 0, 2)             # [B, S, Z]
    B, S, Z = eps_z.shape
    D = int(np.prod(x.shape[1:]))
    sigma = abs(float(np.asarray(params["sigma/Variable"], np.float64).reshape(-1)[0])) if sigma is None else float(sigma)
    prior = cfg["prior"]
    with torch.no_grad():
        mu, sd = O.encoder(cfg, P, x)
        z = mu[:, None, :] + sd[:, None, :] * eps_z
        zr = z.reshape(B * S, Z)
        xhat = O.decoder(cfg, P, zr).reshape(B, S, D)
        out = {"z": z.numpy()}
        out["log_px_z"] = -(x.reshape(B, 1, D) - xhat).abs().sum(-1) / sigma - D * math.log(2.0 * sigma)
        out["log_qz"] = _logq(eps_z, sd[:, None, :])
        if prior == "standard_gaussian":
            out["log_pz"] = _normal_logpdf(z, torch.zeros((), dtype=dt), 1.0)
        elif prior == "GMM":
            out["log_pz"] = O.gmm_log_prob(zr, *(torch.as_tensor(np.asarray(gm[k], np.float64)) for k in ("weights", "means", "covs"))).reshape(B, S)
        elif prior == "vampPrior":                                                      # O.forward: the components the encoder gives at the pseudo-inputs
            mu_p, sd_p = O.encoder(cfg, P, P["prior/Variable"])
            K = mu_p.shape[0]
            u = (zr[:, None, :] - mu_p) / sd_p
            lp = -0.5 * (u ** 2).sum(-1) - torch.log(sd_p).sum(-1) - 0.5 * Z * LOG_2PI - math.log(K)
            out["log_pz"] = torch.logsumexp(lp, dim=-1).reshape(B, S)
        elif prior in ("ours", "hierarchical"):
            et = torch.as_tensor(np.asarray(eps_t, np.float64)).permute(1, 0, 2).reshape(B * S, -1)
            mu_t, sd_t = O.inner_encoder(cfg, P, zr)
            t = mu_t + sd_t * et
            out["log_pz"] = _normal_logpdf(zr, O.inner_decoder(cfg, P, t), inner_sigma(cfg, params)).reshape(B, S)
            out["log_qt"] = _logq(et, sd_t).reshape(B, S)
            if prior == "ours":
                out["log_pt"] = O.gmm_log_prob(t, *(torch.as_tensor(np.asarray(gm[k], np.float64)) for k in ("weights", "means", "covs"))).reshape(B, S)
            else:                                                                       # N(0, I_R) with the true R
                out["log_pt"] = _normal_logpdf(t, torch.zeros((), dtype=dt), 1.0).reshape(B, S)
        else:
            raise NotImplementedError(prior)
    out = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}
    out["logw"] = sum(SIGNS[k] * out[k] for k in SIGNS if k in out)
    return out


def finish(logw):
    """logw [B, S] -> [B, 4]: log_px = logsumexp_s - log S, elbo_1 = mean_s, ess = (sum w)^2 / sum w^2, S.  An image whose weights are all 0: -inf, ess 0."""
    logw = np.asarray(logw, np.float64)
    B, S = logw.shape
    out = np.empty((B, 4))
    for b in range(B):
        M = logw[b].max()
        if M == -np.inf:
            out[b] = (-np.inf, -np.inf, 0.0, S)
            continue
        e = np.exp(logw[b] - M)
        out[b] = (M + math.log(e.sum()) - math.log(S), logw[b].sum() / S, e.sum() ** 2 / (e ** 2).sum(), S)
    return out
