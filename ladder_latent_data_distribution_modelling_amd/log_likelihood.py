"""Importance-weighted estimate of the marginal log-likelihood, log p(x) ~ log (1/S) sum_s w_s, for every prior (DESIGN.md "Importance-weighted
log-likelihood"; kernels: csrc/iwll.hip, and csrc/diag_mixture.hip for log p(z) of the vampPrior).

A batch of B images is encoded once, as `test_step` encodes it (batch-norm statistics of that batch) -> mu_z, sd_z.  Sample s of image b is
z = mu_z[b] + sd_z[b] * eps_z and its log-weight

    standard_gaussian, GMM, vampPrior   log w = log p(x|z) + log p(z) - log q(z|x)
    ours, hierarchical                  t = mu_t(z) + sd_t(z) * eps_t,
                                        log w = log p(x|z) + log N(z; inner_decoder(t), inner_sigma^2 I) + log p(t) - log q(z|x) - log q(t|z)

with log p(x|z) = -sum_d |x_d - xhat_d| / sigma - D log(2 sigma), the Laplace likelihood of define_loss (reference codes/base.py:383-396).
sigma is ONE fixed number per estimator (default |sigma/Variable|, read once), never test_step's batch-dependent max(., mean_pixel_error); there is no mask.
The S x decoder passes run in chunks of C = max(1, rows // B) samples of every image of the batch; the log-weights exist one chunk [B * C] at a
time and enter a streaming log-sum-exp on the device.  The host sees one copy [B, 4] per image batch.
"""
import numpy as np
import torch

from . import _lib as L
from .layers import _p
from .mixture import DeviceMixture

FULL_MIXTURE_PRIORS = ("ours", "GMM")
TERMS = ("log_px_z", "log_pz", "log_pt", "log_qz", "log_qt")       # + "logw" and the code samples "z" with return_terms


def mixture_missing(prior, mode):
    """The RuntimeError of a trainer call that needs a mixture `mode` names before it was fitted (the wording of interpolate_paths)."""
    crude = mode == "crude-GM"
    return RuntimeError("log-likelihood estimation with prior %r, mode %r needs the %s mixture, which has not been fitted yet (fit_GMM_VI(mode=%r))"
                        % (prior, mode, "per-epoch" if crude else "accurate", "fast" if crude else "accurate"))


def check_counts(n_samples, rows):
    n_samples, rows = int(n_samples), int(rows)
    if n_samples < 1 or rows < 1:
        raise ValueError("log-likelihood estimation takes n_samples >= 1 and rows >= 1 (got %d, %d)" % (n_samples, rows))
    return n_samples, rows


class ImportanceEstimator:
    """log p(x) of images under the model of `engine`, by importance sampling from its encoder.

    `mixture` = (weights, means, covs): the fitted full-covariance mixture of the priors "ours" (on t) and "GMM" (on z); the "vampPrior" components are
    those the encoder gives at the pseudo-inputs when the estimator is built.  `sigma`: the scale of the pixel likelihood, a fixed number for every call
    of this estimator (default: |sigma/Variable| as it is now -- NOT the batch-dependent max(|sigma/Variable|, mean_pixel_error) of the ELBO fetches).
    `seed` keys the estimator's own Philox stream: sample s of image i (its index in the data handed to `estimate`, or first + b) draws the same numbers
    whatever `rows` and the batch size are."""

    def __init__(self, engine, mixture=None, sigma=None, seed=0):
        eng = self.eng = engine
        cfg, ctx = eng.cfg, eng.ctx
        self.prior = cfg["prior"]
        self.seed = int(seed)
        self.Z, self.D = eng.Z, eng.D
        self.R = int(cfg["representation_size"]) if eng.has_inner else 0
        eng._join_aux()
        self.sigma = abs(float(eng.ps.w["sigma/Variable"].reshape(-1)[0])) if sigma is None else float(sigma)
        if not (self.sigma > 0.0 and np.isfinite(self.sigma)):
            raise ValueError("sigma must be a finite positive number (got %r)" % self.sigma)
        self.inner_sigma = None
        if eng.has_inner:                                         # the value `forward` computes (reference codes/base.py:210-212)
            s = abs(float(eng.ps.w["inner_sigma/Variable"].reshape(-1)[0]))
            if int(cfg["TRAIN_inner_sigma"]) == 1:
                s = min(max(s, float(np.float32(cfg["inner_sigma_lb"]))), float(np.float32(cfg["inner_sigma_ub"])))
            self.inner_sigma = s
        self.mixture = None
        if self.prior in FULL_MIXTURE_PRIORS:
            if mixture is None:
                raise ValueError("prior %r is evaluated under a fitted mixture: pass mixture=(weights, means, covs)" % self.prior)
            w, m, c = mixture
            self.mixture = DeviceMixture(ctx, int(np.shape(w)[0]), self.R if self.prior == "ours" else self.Z)
            self.mixture.set(w, m, c)
        self.vamp = None
        if self.prior == "vampPrior":
            keep, ctx.keep_activations = ctx.keep_activations, False
            try:
                self.vamp = eng._vamp_components()[:2]
            finally:
                ctx.keep_activations = keep

    # ------------------------------------------------------------------------------------------ row terms
    def _f64(self, n):
        return torch.empty(n, dtype=torch.float64, device=self.eng.ctx.device)

    def _sd(self, sd_raw):
        """The standard deviations of a head: relu output + latent_variance_precision, by the kernel of the training path."""
        ctx, eng = self.eng.ctx, self.eng
        n, W = int(sd_raw.shape[0]), int(sd_raw.shape[1])
        sd, scratch = ctx.empty(n, W), ctx.empty(2)
        L.call("ladder_latent_fwd", _p(sd_raw), _p(sd_raw), None, eng.lvp, None, _p(sd), _p(scratch), _p(scratch[1:]), None, n, W, ctx.stream)
        return sd

    def _eps(self, noise, key, level, s0, c, B, W, first):
        """Noise rows [B * c, W], image-major, of samples s0 .. s0 + c - 1."""
        ctx = self.eng.ctx
        if noise is not None:
            return noise[key][s0:s0 + c].permute(1, 0, 2).reshape(B * c, W).contiguous()
        eps = ctx.empty(B * c, W)
        L.call("ladder_iw_randn_rows", _p(eps), B, c, W, int(first), int(s0), self.seed, level, ctx.stream)
        return eps

    def _sample(self, mu, sd, eps, per):
        n, W = int(eps.shape[0]), int(eps.shape[1])
        out, logq = self.eng.ctx.empty(n, W), self._f64(n)
        L.call("ladder_iw_sample_rows", _p(mu), _p(sd), _p(eps), n, per, W, _p(out), _p(logq), self.eng.ctx.stream)
        return out, logq

    def _gauss(self, a, b, s):
        n, W = int(a.shape[0]), int(a.shape[1])
        out = self._f64(n)
        L.call("ladder_iw_gauss_rows", _p(a), _p(b), float(s), n, W, _p(out), self.eng.ctx.stream)
        return out

    def _laplace(self, x, xhat, per):
        ctx, n = self.eng.ctx, int(xhat.shape[0])
        out = self._f64(n)
        wsp, wsn = ctx.ws(L.query("ladder_iw_laplace_rows_workspace_bytes", n, self.D) or None)
        L.call("ladder_iw_laplace_rows", _p(x), _p(xhat), n, per, self.D, self.sigma, _p(out), wsp, wsn, ctx.stream)
        return out

    def _chunk_terms(self, x, mu, sd, noise, s0, c, first):
        """The term vectors [B * c] of samples s0 .. s0 + c - 1 of every image of the batch -> ({name: (tensor, sign)}, z rows)."""
        eng, B = self.eng, int(mu.shape[0])
        n = B * c
        z, logq_z = self._sample(mu, sd, self._eps(noise, "eps_z", 0, s0, c, B, self.Z, first), c)
        xhat = eng.decoder.forward(z)
        terms = {"log_px_z": (self._laplace(x, xhat.reshape(n, self.D), c), 1.0), "log_qz": (logq_z, -1.0)}
        if self.prior == "standard_gaussian":
            terms["log_pz"] = (self._gauss(z, None, 1.0), 1.0)
        elif self.prior == "GMM":
            terms["log_pz"] = (self.mixture.log_prob_rows(z), 1.0)
        elif self.prior == "vampPrior":
            terms["log_pz"] = (eng.vamp_mixture.log_prob_rows(z, *self.vamp), 1.0)
        else:
            mu_t, sdraw_t = eng.inner.encode(z)
            t, logq_t = self._sample(mu_t, self._sd(sdraw_t), self._eps(noise, "eps_t", 1, s0, c, B, self.R, first), 1)
            terms["log_pz"] = (self._gauss(z, eng.inner.decode(t), self.inner_sigma), 1.0)
            terms["log_pt"] = (self.mixture.log_prob_rows(t) if self.prior == "ours" else self._gauss(t, None, 1.0), 1.0)
            terms["log_qt"] = (logq_t, -1.0)
        return terms, z

    def _logw(self, terms):
        st, logw = self.eng.ctx.stream, None
        for v, sign in terms.values():
            init = logw is None
            if init:
                logw = self._f64(int(v.shape[0]))
            L.call("ladder_iw_add_term", _p(v), int(v.dtype == torch.float32), sign, int(v.shape[0]), int(init), _p(logw), st)
        return logw

    # ------------------------------------------------------------------------------------------ one image batch
    def estimate_batch(self, x, n_samples, rows=128, first=0, noise=None, return_terms=False):
        """x [B, H, W, C] -> float64 array [B, 4]: log_px = logsumexp_s(log w) - log S, elbo_1 = mean_s log w, ess = (sum w)^2 / sum w^2, S.
        `first`: the index of x[0] in the data set (keys the device noise).  `noise` = dict(eps_z [S, B, Z], eps_t [S, B, R]) feeds the draws instead.
        With `return_terms` also a dict of float64 arrays [B, S] (TERMS present for the prior, "logw") and "z" [B, S, Z] float32."""
        eng = self.eng
        ctx, st = eng.ctx, eng.ctx.stream
        S, rows = check_counts(n_samples, rows)
        eng._join_aux()
        x = eng._dev(x)
        B = int(x.shape[0])
        if noise is not None:
            noise = {k: eng._dev(v) for k, v in noise.items() if v is not None}
            for key, W in (("eps_z", self.Z),) + ((("eps_t", self.R),) if eng.has_inner else ()):
                if key not in noise or tuple(noise[key].shape) != (S, B, W):
                    raise ValueError("noise[%r] must be [%d, %d, %d]" % (key, S, B, W))
        C = max(1, rows // B)
        state = torch.zeros(B, 5, dtype=torch.float64, device=ctx.device)
        out = torch.empty(B, 4, dtype=torch.float64, device=ctx.device)
        kept = {}
        keep_acts, ctx.keep_activations = ctx.keep_activations, False
        eng._enc_cache = None                                    # the encoder's layers now hold another batch
        try:
            mu, sd_raw = eng.encoder.forward(x)
            sd = self._sd(sd_raw)
            for s0 in range(0, S, C):
                c = min(C, S - s0)
                terms, z = self._chunk_terms(x, mu, sd, noise, s0, c, first)
                logw = self._logw(terms)
                L.call("ladder_iw_accumulate", _p(logw), B, c, _p(state), st)
                if return_terms:
                    for k, (v, _) in terms.items():
                        kept.setdefault(k, []).append(v.double().reshape(B, c))
                    kept.setdefault("logw", []).append(logw.reshape(B, c))
                    kept.setdefault("z", []).append(z.reshape(B, c, self.Z))
            L.call("ladder_iw_finish", _p(state), B, _p(out), st)
        finally:
            ctx.keep_activations = keep_acts
        res = out.cpu().numpy()
        if return_terms:
            return res, {k: torch.cat(v, dim=1).cpu().numpy() for k, v in kept.items()}
        return res

    # ------------------------------------------------------------------------------------------ a data set
    def estimate(self, data, n_samples=5000, rows=128, batch_size=None, max_images=None):
        """`data`: an array [N, H, W, C], or an iterator whose next() gives [B, H, W, C] batches (then `max_images` is required).  -> dict of the per-image
        arrays log_px, elbo_1, ess, their means, n_samples, n_images and stderr_log_px, the standard error of mean(log_px)."""
        S, rows = check_counts(n_samples, rows)
        per_image = []
        if hasattr(data, "next"):
            if max_images is None or int(max_images) < 1:
                raise ValueError("estimate: an iterator has no end, pass max_images >= 1")
            done = 0
            while done < int(max_images):
                x = data.next()[:int(max_images) - done]
                per_image.append(self.estimate_batch(x, S, rows, first=done))
                done += int(x.shape[0])
        else:
            n = int(data.shape[0]) if max_images is None else min(int(data.shape[0]), int(max_images))
            bs = int(batch_size or self.eng.cfg["batch_size"])
            if n < 1 or bs < 1:
                raise ValueError("estimate: no image to evaluate (N = %d, batch_size = %d)" % (n, bs))
            for lo in range(0, n, bs):
                per_image.append(self.estimate_batch(data[lo:min(lo + bs, n)], S, rows, first=lo))
        return summarise(np.concatenate(per_image, axis=0), self.sigma)


def summarise(per_image, sigma):
    """[N, 4] rows of estimate_batch -> the result dict."""
    log_px, elbo_1, ess = per_image[:, 0].copy(), per_image[:, 1].copy(), per_image[:, 2].copy()
    n = int(log_px.shape[0])
    return dict(log_px=log_px, elbo_1=elbo_1, ess=ess, n_samples=int(per_image[0, 3]), n_images=n, sigma=float(sigma),
                mean_log_px=float(log_px.mean()), mean_elbo_1=float(elbo_1.mean()), mean_ess=float(ess.mean()),
                stderr_log_px=float(log_px.std(ddof=1) / np.sqrt(n)) if n > 1 else 0.0)
