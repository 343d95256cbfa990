"""The fitted full-covariance Gaussian mixture on the device: the one owner of the prepared parameter buffer, in the form of its width's tier
(mixture_forms.py, operation "term": packed, dense or wide).  The ELBO term (LadderEngine), the demo's `log_prob` (demo/demo_tools.py) and the SLP
interpolation (codes/interpolation.py, which reads the packed and the dense buffer) all evaluate the mixture through this class.
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
