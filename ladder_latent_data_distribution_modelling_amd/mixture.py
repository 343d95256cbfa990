"""The fitted full-covariance Gaussian mixture on the device: the one owner of the prepared parameter buffer, in the form of its width's tier
(mixture_forms.py, operation "term": packed, dense or wide).  The ELBO term (LadderEngine), the demo's `log_prob` (demo/demo_tools.py) and the SLP
interpolation (codes/interpolation.py, which reads the packed and the dense buffer) all evaluate the mixture through this class.  `DiagMixture` is the
owner of the VampPrior's equally weighted diagonal mixture (csrc/diag_mixture.hip), whose components arrive with every call.
"""
import numpy as np
import torch

from . import _lib as L
from .layers import _p, _timed
from .mixture_forms import check_status_word, family, sized_workspace


class DeviceMixture:
    def __init__(self, ctx, K, R):
        """`ctx`: the layers.Ctx of the model; K components on R dimensions.  The buffer is allocated once and only ever rewritten in
        place: captured graphs and the run cache of LadderEngine._run hold its address."""
        self.ctx, self.K, self.R = ctx, int(K), int(R)
        self.form = form = family("term", self.K, self.R)
        self.wide, self.dense, self.packed = "wide" in form.tiers, "dense" in form.tiers, "packed" in form.tiers
        # packed: the query answers floats per component; dense: floats; wide: bytes, 0 for a shape it does not take
        n = self.K * L.query(form.param_size, self.R) if self.packed else L.query(form.param_size, self.K, self.R)
        if self.wide and n == 0:
            raise ValueError("a mixture on more than 64 dimensions takes 64 < R <= 256 with R %% 16 == 0 and 1 <= K <= 1024 (got K = %d, R = %d)"
                             % (self.K, self.R))
        self.buf = torch.empty(n, dtype=torch.uint8 if self.wide else torch.float32, device=ctx.device)
        self.prep_ws = None                                  # (tensor, arguments) of the workspace `prepare` takes: allocated by the first set()

    def set(self, weights, means, covs):
        """(weights [K], means [K, R], covs [K, R, R]) as fp32 -> the prepared buffer (Cholesky, inverse factor, log constants)."""
        K, R, dev, form = self.K, self.R, self.ctx.device, self.form
        f = lambda a: (a.to(device=dev, dtype=torch.float32).contiguous() if isinstance(a, torch.Tensor)
                       else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev))
        shapes = tuple(tuple(np.shape(a)) for a in (weights, means, covs))
        if shapes != ((K,), (K, R), (K, R, R)):
            raise ValueError("mixture shapes %s %s %s do not fit K = %d, R = %d" % (shapes + (K, R)))
        w, m, c = f(weights), f(means), f(covs)
        if self.prep_ws is None:
            self.prep_ws = sized_workspace(form.prepare_workspace_bytes, dev, K, R)
        L.call(form.prepare, _p(w), _p(m), _p(c), K, R, _p(self.buf), *self.prep_ws[1], self.ctx.stream)
        torch.cuda.current_stream(dev).synchronize()         # w, m, c are temporaries: keep them alive until the kernel ran
        if self.wide:                                        # (the only form whose prepare leaves a status word)
            check_status_word(self.buf, "mixture", "covariance")

    def fwd_bwd(self, mu, sd, eps, sum_out, need_grad=True):
        """MC estimate of E_q[log p_GM] over the L = eps.shape[0] samples t = mu + sd * eps of each of the B rows: writes the sum of the
        log-probs to `sum_out` and returns (sum_l dlogp/dt, sum_l dlogp/dt * eps), each [B, R] -- (None, None) from the dense and wide
        forms when `need_grad` is False (the packed kernel always forms them)."""
        ctx, form, K, R = self.ctx, self.form, self.K, self.R
        Lmc, B = int(eps.shape[0]), int(mu.shape[0])
        dmu, dsd = (ctx.empty(B, R), ctx.empty(B, R)) if (need_grad or self.packed) else (None, None)
        wsp, wsn = ctx.ws(L.query(form.workspace_bytes, Lmc, B) if self.packed else L.query(form.workspace_bytes, Lmc, B, R, K))
        # (the profiler attributes the packed launch alone, kernel 7700; its flop count: two Mahalanobis passes + the gradient accumulation per component)
        _timed(7700 if self.packed else 0, float(Lmc) * B * K * (3.0 * R * (R + 1) + 4.0 * R + 8.0), form.fwd_bwd,
               (_p(mu), _p(sd), _p(eps), _p(self.buf), Lmc, B, R, K, _p(sum_out), _p(dmu), _p(dsd), wsp, wsn, ctx.stream))
        return dmu, dsd

    def log_prob_rows(self, t):
        """log p of the n points of the device tensor `t` [n, R] in one launch -> device tensor [n] (packed: one wavefront per point, lane =
        component; dense and wide: whitening GEMM + per-row logsumexp, through a workspace)."""
        n, dev, form = int(t.shape[0]), self.ctx.device, self.form
        out = torch.empty(n, device=dev)
        ws, ws_args = sized_workspace(form.workspace_bytes if form.rows_workspace else None, dev, 1, n, self.R, self.K)
        L.call(form.logprob_rows, _p(t), _p(self.buf), n, self.R, self.K, _p(out), *ws_args, self.ctx.stream)
        return out


class DiagMixture:
    """The equally weighted mixture of K diagonal Gaussians on Z dimensions (the VampPrior): its ELBO term in the form of its width (mixture_forms.py,
    operation "diag_term") and the log-density of separate points.  It keeps no parameters: the components (comp_mean, comp_sd [K, Z]) are what the
    encoder gives at the pseudo-inputs, passed with each call."""

    def __init__(self, ctx, K, Z):
        self.ctx, self.K, self.Z = ctx, int(K), int(Z)
        self.form = family("diag_term", self.K, self.Z)
        self.rows_ws = None                                  # (tensor, arguments) of the workspace log_prob_rows takes: sized once, by its first call

    def fwd_bwd(self, mu, sd, eps, comp_mean, comp_sd, sum_out):
        """MC estimate over the L = eps.shape[0] samples t = mu + sd * eps of each of the B rows: writes the sum of the log-probs to `sum_out` and
        returns (dmu, dsd [B, Z], dcomp_mean, dcomp_sd [K, Z]), the sums over the samples of dlogp/dt, dlogp/dt * eps and dlogp/d component."""
        ctx, form, K, Z = self.ctx, self.form, self.K, self.Z
        Lmc, B = int(eps.shape[0]), int(mu.shape[0])
        dmu, dsd, dcm, dcs = ctx.empty(B, Z), ctx.empty(B, Z), ctx.empty(K, Z), ctx.empty(K, Z)
        wsp, wsn = ctx.ws(L.query(form.workspace_bytes, Lmc, B, Z, K) if form.query_takes_L else L.query(form.workspace_bytes, B, Z, K))
        L.call(form.fwd_bwd, _p(mu), _p(sd), _p(eps), _p(comp_mean), _p(comp_sd), Lmc, B, Z, K, _p(sum_out), _p(dmu), _p(dsd), _p(dcm), _p(dcs),
               wsp, wsn, ctx.stream)
        return dmu, dsd, dcm, dcs

    def log_prob_rows(self, z, comp_mean, comp_sd):
        """log p of the n points of the device tensor `z` [n, Z] -> device tensor [n] (one export for every width up to 256: nothing to select)."""
        ctx, n = self.ctx, int(z.shape[0])
        if self.rows_ws is None:                             # (the size does not depend on n)
            self.rows_ws = sized_workspace("ladder_diag_mixture_logprob_rows_workspace_bytes", ctx.device, 1, self.Z, self.K)
        out = ctx.empty(n)
        L.call("ladder_diag_mixture_logprob_rows", _p(z), _p(comp_mean), _p(comp_sd), n, self.Z, self.K, _p(out), *self.rows_ws[1], ctx.stream)
        return out
