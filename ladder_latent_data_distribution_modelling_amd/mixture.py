"""The fitted full-covariance Gaussian mixture on the device: the one owner of the prepared parameter buffer and of the choice between
its three forms -- packed {c_k, mean_k, Linv_k} for narrow latents (R <= 8: csrc/mixture.hip, csrc/gmm_packed.h; also what
`ladder_slp_optimise` reads), the whitening-GEMM form for 8 < R <= 64, R % 4 == 0 (prior "GMM", or prior "ours" on a wide
representation; also what `ladder_slp_wide_optimise` reads) and the wide form for 64 < R <= 256, R % 16 == 0 (csrc/mixture_wide.hip: prior
"GMM" at the reference's shipped code_size 256).  The ELBO term (LadderEngine), the demo's `log_prob` (demo/demo_tools.py) and the SLP
interpolation (codes/interpolation.py) all evaluate the mixture through this class.
"""
import numpy as np
import torch

from . import _lib as L
from .layers import _p, _timed


class DeviceMixture:
    def __init__(self, ctx, K, R):
        """`ctx`: the layers.Ctx of the model; K components on R dimensions.  The buffer is allocated once and only ever rewritten in
        place: captured graphs and the run cache of LadderEngine._run hold its address."""
        self.ctx, self.K, self.R = ctx, int(K), int(R)
        self.wide = self.R > 64                              # 64 < R <= 256: its own kernels, the whitened product never leaves them
        self.dense = 8 < self.R <= 64                        # prior "GMM" up to 64: whitening as a GEMM on the dense kernel
        if self.wide:
            nbytes = L.query("ladder_gmm_wide_param_bytes", self.K, self.R)
            if nbytes == 0:
                raise ValueError("a mixture on more than 64 dimensions takes 64 < R <= 256 with R %% 16 == 0 and 1 <= K <= 1024 (got K = %d, R = %d)"
                                 % (self.K, self.R))
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device)
            self.prep_ws = None                              # float64 working matrices of the factorisation: allocated by the first set()
        else:
            self.buf = ctx.empty(L.query("ladder_gmm_dense_param_floats", self.K, self.R) if self.dense
                                 else self.K * L.query("ladder_gmm_packed_stride", self.R))

    def set(self, weights, means, covs):
        """(weights [K], means [K, R], covs [K, R, R]) as fp32 -> the prepared buffer (Cholesky, inverse factor, log constants)."""
        K, R, dev = self.K, self.R, self.ctx.device
        f = lambda a: (a.to(device=dev, dtype=torch.float32).contiguous() if isinstance(a, torch.Tensor)
                       else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev))
        shapes = tuple(tuple(np.shape(a)) for a in (weights, means, covs))
        if shapes != ((K,), (K, R), (K, R, R)):
            raise ValueError("mixture shapes %s %s %s do not fit K = %d, R = %d" % (shapes + (K, R)))
        w, m, c = f(weights), f(means), f(covs)
        if self.wide:
            if self.prep_ws is None:
                self.prep_ws = torch.empty(L.query("ladder_gmm_wide_prepare_workspace_bytes", K, R), dtype=torch.uint8, device=dev)
            L.call("ladder_gmm_wide_prepare", _p(w), _p(m), _p(c), K, R, _p(self.buf), _p(self.prep_ws), self.prep_ws.numel(), self.ctx.stream)
            torch.cuda.current_stream(dev).synchronize()
            status = int(self.buf[:4].view(torch.int32).item())      # (the one read of the status word)
            if status >= 0:
                raise ValueError("component %d of the mixture has no Cholesky factor (covariance not positive definite)" % status)
            if status != -1:
                raise ValueError("the weights of the mixture have no positive finite sum")
            return
        L.call("ladder_gmm_prepare_dense" if self.dense else "ladder_gmm_prepare", _p(w), _p(m), _p(c), K, R, _p(self.buf), self.ctx.stream)
        torch.cuda.current_stream(dev).synchronize()         # w, m, c are temporaries: keep them alive until the kernel ran

    def fwd_bwd(self, mu, sd, eps, sum_out, need_grad=True):
        """MC estimate of E_q[log p_GM] over the L = eps.shape[0] samples t = mu + sd * eps of each of the B rows: writes the sum of the
        log-probs to `sum_out` and returns (sum_l dlogp/dt, sum_l dlogp/dt * eps), each [B, R] -- (None, None) from the dense and wide
        forms when `need_grad` is False (the packed kernel always forms them)."""
        ctx, st, K, R = self.ctx, self.ctx.stream, self.K, self.R
        Lmc, B = int(eps.shape[0]), int(mu.shape[0])
        dmu, dsd = (ctx.empty(B, R), ctx.empty(B, R)) if (need_grad or not (self.dense or self.wide)) else (None, None)
        if self.wide:
            wsp, wsn = ctx.ws(L.query("ladder_gmm_wide_workspace_bytes", Lmc, B, R, K))
            L.call("ladder_gmm_wide_logprob_fwd_bwd", _p(mu), _p(sd), _p(eps), _p(self.buf), Lmc, B, R, K, _p(sum_out), _p(dmu), _p(dsd),
                   wsp, wsn, st)
        elif self.dense:
            wsp, wsn = ctx.ws(L.query("ladder_gmm_dense_workspace_bytes", Lmc, B, R, K))
            L.call("ladder_gmm_dense_logprob_fwd_bwd", _p(mu), _p(sd), _p(eps), _p(self.buf), Lmc, B, R, K, _p(sum_out), _p(dmu), _p(dsd),
                   wsp, wsn, st)
        else:
            wsp, wsn = ctx.ws(L.query("ladder_gmm_workspace_bytes", Lmc, B))
            # (flop count of the profiler entry: two Mahalanobis passes + the gradient accumulation per component evaluation)
            _timed(7700, float(Lmc) * B * K * (3.0 * R * (R + 1) + 4.0 * R + 8.0), "ladder_gmm_logprob_fwd_bwd",
                   (_p(mu), _p(sd), _p(eps), _p(self.buf), Lmc, B, R, K, _p(sum_out), _p(dmu), _p(dsd), wsp, wsn, st))
        return dmu, dsd

    def log_prob_rows(self, t):
        """log p of the n points of the device tensor `t` [n, R] in one launch -> device tensor [n] (ladder_gmm_logprob_rows: one
        wavefront per point, lane = component; 8 < R <= 64: whitening GEMM + per-row logsumexp, ladder_gmm_dense_logprob_rows; R > 64:
        ladder_gmm_wide_logprob_rows)."""
        n, dev, st = int(t.shape[0]), self.ctx.device, self.ctx.stream
        out = torch.empty(n, device=dev)
        if self.wide:
            ws = torch.empty(L.query("ladder_gmm_wide_workspace_bytes", 1, n, self.R, self.K), dtype=torch.uint8, device=dev)
            L.call("ladder_gmm_wide_logprob_rows", _p(t), _p(self.buf), n, self.R, self.K, _p(out), _p(ws), ws.numel(), st)
        elif self.dense:
            ws = torch.empty(L.query("ladder_gmm_dense_workspace_bytes", 1, n, self.R, self.K), dtype=torch.uint8, device=dev)
            L.call("ladder_gmm_dense_logprob_rows", _p(t), _p(self.buf), n, self.R, self.K, _p(out), _p(ws), ws.numel(), st)
        else:
            L.call("ladder_gmm_logprob_rows", _p(t), _p(self.buf), n, self.R, self.K, _p(out), st)
        return out
