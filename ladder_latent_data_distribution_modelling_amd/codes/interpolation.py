"""Shortest-likely-path (SLP) interpolation in the latent space of the fitted mixture prior -- the optimisation of the reference's
notebook `latent-space-interpolation-mnist.ipynb` (cells 18-23), without TensorFlow.

    objective(pts) = w_path * sum_i |p_{i+1} - p_i|  +  w_equal * std_i |p_{i+1} - p_i|  -  sum_i log p_GM(p_i)

over `n_step` intermediate points between two fixed embeddings, minimised with clip-[-1,1] + Adam(beta1=.9, beta2=.95) exactly like
the notebook's `opt_interpolation` (cell 19).  The mixture term and its gradient come from the HIP mixture kernel
(`DeviceMixture.fwd_bwd` with one "MC sample" and eps = 0, so t = mean = the path points); the remaining algebra is a handful
of numbers and stays on the host.  `decode_path` maps the optimised path to images (t -> inner decoder -> z -> decoder), as
demo/demo_tools.py:163-186 does through `sess.run`.
"""
import functools
import math

import numpy as np
import torch

from .. import _lib as L
from ..mixture import DeviceMixture
from ..mixture_forms import SLP_DENSE, family

MAX_STEP = 64                   # ladder_slp_optimise: 1 <= n_step <= 64
MAX_ITER_PER_LAUNCH = 4096      # ... and at most 4096 iterations per launch; longer runs are chained through its float64 state
MAX_POINTS_WIDE = SLP_DENSE.max_points # the dense tier's kernel keeps the float64 path state in LDS: n_step * R <= 2048


def path_terms(pts, start, end):
    """-> (entire_path_length, equal_length_constraint, d/dpts of each) for the intermediate points `pts` [n, R]."""
    full = np.concatenate([start[None], pts, end[None]], 0)
    d = full[1:] - full[:-1]                                  # segments, [n+1, R]
    ln = np.sqrt((d ** 2).sum(1))
    unit = d / np.maximum(ln, 1e-30)[:, None]
    g_len = unit[:-1] - unit[1:]                              # d sum(len) / d p_i : +from the segment ending at p_i, -from the one leaving it
    mean = ln.mean()
    std = math.sqrt(((ln - mean) ** 2).mean())                # tf.math.reduce_std: population standard deviation
    c = (ln - mean) / (len(ln) * max(std, 1e-30))             # d std / d len_j
    g_std = c[:-1, None] * unit[:-1] - c[1:, None] * unit[1:]
    return ln.sum(), std, g_len, g_std


class SLPInterpolator:
    def __init__(self, engine, weights, means, covs):
        """`engine`: a LadderEngine (for the device / stream / decoders); (weights, means, covs): the fitted mixture, of a width operation
        "slp" of mixture_forms.py has a row for (packed: csrc/slp.hip; dense: csrc/slp_wide.hip)."""
        self.eng = engine
        self.K, self.R = (int(n) for n in np.shape(means))
        self.form = family("slp", self.K, self.R)                # (raises for a width no row takes)
        self.mixture = DeviceMixture(engine.ctx, self.K, self.R)
        self.mixture.set(weights, means, covs)

    form = functools.cached_property(lambda self: family("slp", self.K, self.R))      # (for an object built without __init__: on first use)

    def neg_log_likelihood(self, pts):
        """-> (-sum_i log p(p_i), gradient [n, R]) from the HIP mixture kernel."""
        dev = self.eng.ctx.device
        mu = torch.as_tensor(np.ascontiguousarray(pts, dtype=np.float32)).to(dev)
        out = torch.empty(1, device=dev)
        dmu, _ = self.mixture.fwd_bwd(mu, torch.ones_like(mu), torch.zeros(1, pts.shape[0], self.R, device=dev), out)
        return -float(out.item()), -dmu.cpu().numpy().astype(np.float64)

    def optimise(self, start, end, n_step=5, n_iter=500, lr=1e-2, w_equal_length=100.0, w_path_dist=10.0, init=None):
        """Notebook cells 18-21.  Returns (pts [n_step, R], record dict of the per-iteration loss terms)."""
        start, end = np.asarray(start, np.float64), np.asarray(end, np.float64)
        pts = np.asarray(init, np.float64).copy() if init is not None else np.linspace(start, end, n_step + 1, endpoint=False)[1:]
        from .utils import register_trainable_scope
        register_trainable_scope("interpolation", pts.size)      # notebook cell 19: count_trainable_variables('interpolation')
        m, v = np.zeros_like(pts), np.zeros_like(pts)
        rec = dict(loss=[], path_length=[], step_var=[], neg_ll=[])
        for t in range(1, n_iter + 1):
            plen, std, g_len, g_std = path_terms(pts, start, end)
            nll, g_nll = self.neg_log_likelihood(pts)
            rec["loss"].append(w_path_dist * plen + w_equal_length * std + nll)
            rec["path_length"].append(plen); rec["step_var"].append(std); rec["neg_ll"].append(nll)
            g = np.clip(w_path_dist * g_len + w_equal_length * g_std + g_nll, -1.0, 1.0)      # model.ClipIfNotNone
            m = 0.9 * m + 0.1 * g
            v = 0.95 * v + 0.05 * g * g
            pts = pts - lr * math.sqrt(1 - 0.95 ** t) / (1 - 0.9 ** t) * m / (np.sqrt(v) + 1e-8)
        return pts, rec

    def decode_path(self, start, pts, end):
        """Images along [start, pts..., end] (clipped to [0,1] as the demo does)."""
        t = np.concatenate([np.asarray(start)[None], pts, np.asarray(end)[None]], 0)
        code = self.eng.decode_representation(t) if self.eng.has_inner else self.eng._dev(t)
        return np.clip(self.eng.decode(code).cpu().numpy(), 0.0, 1.0)

    # ------------------------------------------------------------------ many paths at once (csrc/slp.hip, csrc/slp_wide.hip)
    def _check_batch(self, starts, ends, n_step):
        starts, ends = np.asarray(starts, np.float64), np.asarray(ends, np.float64)
        if starts.ndim != 2 or starts.shape != ends.shape or starts.shape[0] < 1:
            raise ValueError("optimise_batch: starts and ends must both be [P, R] with P >= 1 (got %s and %s)" % (starts.shape, ends.shape))
        if starts.shape[1] != self.R:
            raise ValueError("optimise_batch: the end points have R = %d, the mixture has R = %d" % (starts.shape[1], self.R))
        if not 1 <= int(n_step) <= MAX_STEP:
            raise ValueError("optimise_batch: n_step must be in 1..%d (got %r)" % (MAX_STEP, n_step))
        if self.form.max_points is not None and int(n_step) * self.R > self.form.max_points:
            raise ValueError("optimise_batch: n_step * R = %d * %d = %d exceeds %d, what the wide kernel (R > 8) keeps of a path"
                             % (int(n_step), self.R, int(n_step) * self.R, self.form.max_points))
        return starts, ends

    def optimise_batch(self, starts, ends, n_step=5, n_iter=500, lr=1e-2, w_equal_length=100.0, w_path_dist=10.0, init=None, clip=1.0,
                       record=True):
        """`optimise` for P pairs at once, the whole loop on the device (the row of operation "slp" for the mixture's tier: one workgroup per
        path, one launch per 4096 iterations, chained through the float64 state; no host
        synchronisation in between, one copy to the host at the end).
        starts, ends [P, R]; init [P, n_step, R] (default: the notebook's linspace per pair); `clip` is the element-wise gradient bound.
        The kernel takes its inputs as fp32 and keeps points and moments in float64 from there on.
        Returns (pts [P, n_step, R]: the fp32 results as float64, rec: {loss, path_length, step_var, neg_ll} each [P, n_iter] -- None
        when `record` is False)."""
        starts, ends, form = *self._check_batch(starts, ends, n_step), self.form
        n_step, n_iter = int(n_step), int(n_iter)
        if n_iter < 1:
            raise ValueError("optimise_batch: n_iter must be >= 1 (got %d)" % n_iter)
        P, R = starts.shape
        if init is None:
            init = np.stack([np.linspace(s, e, n_step + 1, endpoint=False)[1:] for s, e in zip(starts, ends)])
        init = np.asarray(init, np.float64)
        if init.shape != (P, n_step, R):
            raise ValueError("optimise_batch: init must be [P, n_step, R] = %s (got %s)" % ((P, n_step, R), init.shape))
        from .utils import register_trainable_scope
        register_trainable_scope("interpolation", init.size)     # notebook cell 19: count_trainable_variables('interpolation')
        dev, st = self.eng.ctx.device, self.eng.ctx.stream
        f = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
        s_d, e_d, pts = f(starts), f(ends), f(init)
        state = torch.empty(L.query(form.state_bytes, P, n_step, R) // 8, dtype=torch.float64, device=dev)
        recs = []
        for t0 in range(0, n_iter, MAX_ITER_PER_LAUNCH):
            k = min(MAX_ITER_PER_LAUNCH, n_iter - t0)
            r = torch.empty(P, k, 4, dtype=torch.float64, device=dev) if record else None
            L.call(form.optimise, s_d.data_ptr(), e_d.data_ptr(), pts.data_ptr(), self.mixture.buf.data_ptr(), self.K, R, P, n_step, k, t0,
                   float(lr), 0.9, 0.95, 1e-8, float(clip), float(w_path_dist), float(w_equal_length), state.data_ptr(),
                   None if r is None else r.data_ptr(), st)
            recs.append(r)
        flat = [pts.to(torch.float64).reshape(-1)] + ([torch.cat(recs, 1).reshape(-1)] if record else [])
        host = torch.cat(flat).cpu().numpy()                     # the one copy (and the one synchronisation)
        out = host[:init.size].reshape(P, n_step, R).copy()
        rec = None
        if record:
            r = host[init.size:].reshape(P, n_iter, 4)
            rec = {k: r[:, :, i].copy() for i, k in enumerate(("loss", "path_length", "step_var", "neg_ll"))}
        return out, rec

    def decode_paths(self, starts, pts, ends, chunk=128):
        """Images along P paths [start, pts..., end] -> [P, n_step + 2, H, W, C] clipped to [0, 1]; a decoder batch holds whole paths and at
        most `chunk` points."""
        starts, ends, pts = np.asarray(starts), np.asarray(ends), np.asarray(pts)
        if pts.ndim != 3 or starts.shape != (pts.shape[0], pts.shape[2]) or ends.shape != starts.shape:
            raise ValueError("decode_paths: starts / ends [P, R] and pts [P, n_step, R] expected (got %s, %s, %s)" % (starts.shape, ends.shape, pts.shape))
        P, n = pts.shape[0], pts.shape[1] + 2
        per = int(chunk) // n
        if per < 1:
            raise ValueError("decode_paths: chunk = %d holds no whole path of %d points" % (chunk, n))
        t = np.concatenate([starts[:, None], pts, ends[:, None]], 1)
        out = []
        for lo in range(0, P, per):
            tb = t[lo:lo + per].reshape(-1, t.shape[2])
            code = self.eng.decode_representation(tb) if self.eng.has_inner else self.eng._dev(tb)
            img = np.clip(self.eng.decode(code).cpu().numpy(), 0.0, 1.0)
            out.append(img.reshape((-1, n) + img.shape[1:]))
        return np.concatenate(out, 0)
