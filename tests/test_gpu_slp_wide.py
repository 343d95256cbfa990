"""Batched shortest-likely-path interpolation for wide representations, 8 < R <= 64 with R % 4 == 0 (csrc/slp_wide.hip:
ladder_slp_wide_optimise on the dense mixture buffer; codes/interpolation.py: SLPInterpolator.optimise_batch; codes/base.py:
interpolate_paths).

The helpers follow tests/test_gpu_slp_batch.py: the float64 reference is the notebook's loop in torch autograd on the oracle's mixture
log-prob, every input the kernel takes as fp32 is rounded to fp32 before any loop sees it, and no chaotic trajectory (a long one, or one
from the exactly uniform linspace points) is compared between two implementations.  Mixtures are O.synthetic_gm rounded to fp32, as
test_gmm_dense_logprob builds them.

Shapes (K, R, n_step): R = 12 forces column padding of the 16-wide MFMA tile, R = 16 is one tile, R = 64 the limit; n_step = 17 crosses a
16-row point tile; n_step = 1 and K = 1 are the degenerate ends (K = 1: three of the four wavefronts own no component); K = 70 gives the
wavefronts 18 / 18 / 17 / 17 components.
"""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

from oracle import ladder_oracle as O

pytestmark = pytest.mark.gpu
E_SHAPE = -1
LR, W_PATH, W_EQUAL = 1e-2, 10.0, 100.0                     # the notebook's hyper-parameters (cells 19-20)
SHAPES = [(3, 12, 5), (30, 64, 5), (70, 16, 17), (5, 64, 32), (30, 16, 1), (1, 20, 4)]
G_BAR, NLL_REL, NLL_ABS = 1e-4, 3e-5, 1e-3                  # test_gmm_dense_logprob's bars for this arithmetic


def _L():
    from ladder_latent_data_distribution_modelling_amd import _lib
    _lib.load()
    return _lib


@functools.lru_cache(maxsize=None)
def _mixture(K, R):
    rng = np.random.default_rng(K * 7 + R)
    return {k: v.astype(np.float32) for k, v in O.synthetic_gm(dict(n_mixtures=K, representation_size=R), rng).items()}


def mixture(K, R):
    return {k: v.copy() for k, v in _mixture(K, R).items()}


def draw_paths(seed, P, n_step, R):
    """starts, ends ~ N(0, 1.5^2); initial points = the linspace + 0.1 Gaussian jitter; all rounded to fp32 (returned as float64)."""
    rng = np.random.default_rng(seed)
    starts, ends = rng.normal(0, 1.5, (P, R)), rng.normal(0, 1.5, (P, R))
    init = np.stack([np.linspace(s, e, n_step + 1, endpoint=False)[1:] for s, e in zip(starts, ends)]) + 0.1 * rng.standard_normal((P, n_step, R))
    return tuple(a.astype(np.float32).astype(np.float64) for a in (starts, ends, init))


def reference_loop(gm, starts, ends, init, n_iter, clip):
    """The notebook's loop in float64 autograd, all paths at once -> dict(pts, m, v [P,n,R], grads [n_iter,P,n,R] raw gradients,
    loss / path_length / step_var / neg_ll [P,n_iter])."""
    w, m, c = (torch.tensor(gm[k], dtype=torch.float64) for k in ("weights", "means", "covs"))
    s, e = torch.tensor(starts), torch.tensor(ends)
    p = torch.tensor(init, requires_grad=True)
    mom, var = torch.zeros_like(p), torch.zeros_like(p)
    out = dict(grads=[], loss=[], path_length=[], step_var=[], neg_ll=[])
    for t in range(1, n_iter + 1):
        a, b = torch.cat([s[:, None], p], 1), torch.cat([p, e[:, None]], 1)
        ln = torch.sqrt(((b - a) ** 2).sum(-1))
        plen, std, nll = ln.sum(1), ln.std(1, unbiased=False), -O.gmm_log_prob(p, w, m, c).sum(1)
        obj = W_PATH * plen + W_EQUAL * std + nll
        (g,) = torch.autograd.grad(obj.sum(), p)
        for k, val in (("loss", obj), ("path_length", plen), ("step_var", std), ("neg_ll", nll)):
            out[k].append(val.detach().numpy().copy())
        out["grads"].append(g.numpy().copy())
        g = g.clamp(-clip, clip)
        mom = 0.9 * mom + 0.1 * g
        var = 0.95 * var + 0.05 * g * g
        p = (p - LR * np.sqrt(1 - 0.95 ** t) / (1 - 0.9 ** t) * mom / (var.sqrt() + 1e-8)).detach().requires_grad_(True)
    res = {k: np.stack(v, 1) for k, v in out.items() if k != "grads"}
    res.update(grads=np.stack(out["grads"]), pts=p.detach().numpy(), m=mom.numpy(), v=var.numpy())
    return res


class Device:
    """The wide C ABI on one prepared dense mixture."""

    def __init__(self, ctx, gm):
        L = self.L = _L()
        self.st = ctx.stream
        self.K, self.R = gm["means"].shape
        w, m, c = (torch.as_tensor(np.ascontiguousarray(gm[k], np.float32)).cuda() for k in ("weights", "means", "covs"))
        self.params = torch.empty(L.query("ladder_gmm_dense_param_floats", self.K, self.R), device="cuda")
        L.call("ladder_gmm_prepare_dense", w.data_ptr(), m.data_ptr(), c.data_ptr(), self.K, self.R, self.params.data_ptr(), self.st)
        torch.cuda.synchronize()

    def run(self, starts, ends, init, n_iter, clip=1.0, t0=0, state=None):
        """-> (pts [P,n,R] fp32, state [3,P,n,R] float64, record [P,n_iter,4] float64), all on the host; `state` resumes (t0 > 0)."""
        L = self.L
        P, n, R = init.shape
        f = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()
        s, e, pts = f(starts), f(ends), f(init)
        nd = L.query("ladder_slp_wide_state_bytes", P, n, R) // 8
        assert nd == 3 * P * n * R
        sd = torch.full((nd,), float("nan"), dtype=torch.float64, device="cuda") if state is None else torch.as_tensor(state).reshape(-1).cuda()
        rec = torch.full((P, n_iter, 4), float("nan"), dtype=torch.float64, device="cuda")
        L.call("ladder_slp_wide_optimise", s.data_ptr(), e.data_ptr(), pts.data_ptr(), self.params.data_ptr(), self.K, R, P, n, n_iter, t0,
               LR, 0.9, 0.95, 1e-8, float(clip), W_PATH, W_EQUAL, sd.data_ptr(), rec.data_ptr(), self.st)
        torch.cuda.synchronize()
        assert torch.equal(s, f(starts)) and torch.equal(e, f(ends))                  # the end points are inputs only
        return pts.cpu().numpy(), sd.cpu().numpy().reshape(3, P, n, R), rec.cpu().numpy()


def close(got, ref, rtol, what=""):
    """test_gpu_kernels.close: max error relative to the reference's largest magnitude."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)
    assert np.isfinite(got).all() and err < rtol, "%s: rel err %.3e (tol %.1e)" % (what, err, rtol)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)) / np.maximum(np.abs(np.asarray(b)), 1e-300)


# ------------------------------------------------------------------------------------------------ 1. gradient and terms, one step, clip off
@pytest.mark.parametrize("K,R,n_step", SHAPES)
def test_one_step_gradient_and_terms(gpu_ctx, K, R, n_step):
    """After one step with the clip effectively off the first moment is 0.1 * g: 10 * m against the float64 autograd gradient at
    test_gmm_dense_logprob's bar (1e-4 of the largest magnitude); the record against the float64 terms; the Adam step from the host
    formulas.  An eighth path with start == end == every initial point has zero lengths: both guards active, path gradients exactly zero."""
    gm = mixture(K, R)
    starts, ends, init = draw_paths(1000 + K + R + n_step, 7, n_step, R)
    ref = reference_loop(gm, starts, ends, init, 1, 1e30)
    pt = np.random.default_rng(5).normal(0, 1.5, R).astype(np.float32).astype(np.float64)
    starts8, ends8 = np.concatenate([starts, pt[None]]), np.concatenate([ends, pt[None]])
    init8 = np.concatenate([init, np.broadcast_to(pt, (1, n_step, R))])
    pts, state, rec = Device(gpu_ctx, gm).run(starts8, ends8, init8, 1, clip=1e30)
    assert np.isfinite(pts).all() and np.isfinite(state).all() and np.isfinite(rec).all()
    g = 10.0 * state[1]
    loss, plen, std, nll = (rec[:, 0, i] for i in range(4))
    print("K %d R %d n %d: gradient rel err %.3e, neg_ll rel err %.3e" % (K, R, n_step, np.abs(g[:7] - ref["grads"][0]).max() / np.abs(ref["grads"][0]).max(),
                                                                        rel(nll[:7], ref["neg_ll"][:, 0]).max()))
    close(g[:7], ref["grads"][0], G_BAR, "gradient")
    assert rel(plen[:7], ref["path_length"][:, 0]).max() <= 1e-12 and rel(std[:7], ref["step_var"][:, 0]).max() <= 1e-12
    assert (np.abs(nll[:7] - ref["neg_ll"][:, 0]) < NLL_REL * np.abs(ref["neg_ll"][:, 0]) + NLL_ABS).all()
    assert rel(loss, W_PATH * plen + W_EQUAL * std + nll).max() <= 1e-12
    # the degenerate path: the mixture gradient alone
    w, m, c = (torch.tensor(gm[k], dtype=torch.float64) for k in ("weights", "means", "covs"))
    p8 = torch.tensor(init8[7], requires_grad=True)
    lp = O.gmm_log_prob(p8, w, m, c)
    (g8,) = torch.autograd.grad(-lp.sum(), p8)
    assert plen[7] == 0.0 and std[7] == 0.0
    close(g[7], g8.numpy(), G_BAR, "degenerate path: gradient")
    assert abs(nll[7] + lp.sum().item()) < NLL_REL * abs(lp.sum().item()) + NLL_ABS
    # moments and step of every path from the FLOAT64 reference gradient g (SLPInterpolator.optimise's formulas at t = 1: m = 0.1 g,
    # v = 0.05 g^2, step s(g) = lr sqrt(0.05) g / (sqrt(0.05) |g| + 1e-8)), each within what the gradient bar dg allows: |dv| <= 0.05 (2 |g| + dg) dg,
    # |ds| <= s'(|g| - dg) dg with s'(x) = lr sqrt(0.05) 1e-8 / (sqrt(0.05) x + 1e-8)^2 (decreasing in x), plus 1e-12 for the float64 algebra
    g_ref = np.concatenate([ref["grads"][0], g8.numpy()[None]])
    dg, r5 = G_BAR * np.abs(g_ref).max(), np.sqrt(0.05)
    assert (np.abs(state[2] - 0.05 * g_ref ** 2) <= 0.05 * (2 * np.abs(g_ref) + dg) * dg + 1e-12).all()
    want = init8 - LR * r5 * g_ref / (r5 * np.abs(g_ref) + 1e-8)
    slope = LR * r5 * 1e-8 / (r5 * np.maximum(np.abs(g_ref) - dg, 0.0) + 1e-8) ** 2
    assert (np.abs(state[0] - want) <= slope * dg + 1e-12).all()
    assert np.abs(state[0][:7] - ref["pts"]).max() <= (slope[:7] * dg + 1e-12).max()
    assert np.array_equal(pts, state[0].astype(np.float32))


# ------------------------------------------------------------------------------------------------ 2. zero-weight components
def test_zero_weight_components_contribute_nothing(gpu_ctx):
    """Components of weight exactly 0 (logc = -inf): index 0 is the first component wavefront 0 meets, 3 the first of wavefront 3, 64 a
    later one of wavefront 0.  The gradient and neg_ll are those of the float64 mixture at test 1's bars, and everything stays finite
    over chained clipped iterations."""
    gm = mixture(70, 16)
    gm["weights"][[0, 3, 64]] = 0.0
    starts, ends, init = draw_paths(11, 4, 5, 16)
    ref = reference_loop(gm, starts, ends, init, 1, 1e30)
    assert np.isfinite(ref["grads"]).all()
    dev = Device(gpu_ctx, gm)
    _, state, rec = dev.run(starts, ends, init, 1, clip=1e30)
    close(10.0 * state[1], ref["grads"][0], G_BAR, "gradient")
    assert (np.abs(rec[:, 0, 3] - ref["neg_ll"][:, 0]) < NLL_REL * np.abs(ref["neg_ll"][:, 0]) + NLL_ABS).all()
    pa, sa, ra = dev.run(starts, ends, init, 10)
    pb, sb, rb = dev.run(starts, ends, init, 10, t0=10, state=sa)
    pc, sc, rc = dev.run(starts, ends, init, 10, t0=20, state=sb)
    for a in (pa, sa, ra, pb, sb, rb, pc, sc, rc):
        assert np.isfinite(a).all()


# ------------------------------------------------------------------------------------------------ 3. ten iterations against float64, clip 1.0
# End points and initial points: draw_paths, as in the narrow test.  At these widths the mixture gradient is large, but the condition below is
# not trivial: in the float64 loop 5 % (R = 12), 6 % (R = 64) and 13 % (R = 16) of the raw gradient elements lie inside (-1, 1), so the clip
# acts on some elements and not on others and the value of the gradient, not only its sign, enters the trajectory.  Seed per shape, chosen
# on the CPU with the float64 reference only: the first seed from 0 upwards with which no raw gradient element of any of the 8 paths comes
# within 1e-4 of +-1 in any of the 10 iterations (nearest: 4.3e-4, 3.3e-4, 8.7e-4), so that both implementations clip the same elements.
TEN_ITER_SEEDS = {(3, 12, 5): 0, (30, 64, 5): 0, (70, 16, 17): 0}


@functools.lru_cache(maxsize=None)
def ten_iteration_case(K, R, n_step):
    gm = mixture(K, R)
    starts, ends, init = draw_paths(TEN_ITER_SEEDS[(K, R, n_step)], 8, n_step, R)
    return gm, starts, ends, init, reference_loop(gm, starts, ends, init, 10, 1.0)


@pytest.mark.parametrize("K,R,n_step", sorted(TEN_ITER_SEEDS))
def test_ten_iterations_vs_float64(gpu_ctx, K, R, n_step):
    """Ten clipped iterations.  The bar is set by the host loop (SLPInterpolator.optimise, which reaches the dense mixture kernels
    through DeviceMixture.fwd_bwd) on the same inputs: its largest point deviation from the float64 loop, d_host; the device loop may
    deviate 4 * d_host + 1e-7.  Measured on MI355X (d_host, device): see DESIGN.md, "Wide representations"."""
    from ladder_latent_data_distribution_modelling_amd.codes.interpolation import SLPInterpolator
    gm, starts, ends, init, ref = ten_iteration_case(K, R, n_step)
    nearest = np.abs(np.abs(ref["grads"]) - 1.0).min()
    assert nearest >= 1e-4, nearest                          # the condition on the inputs
    clipped = (np.abs(ref["grads"]) > 1.0).mean()
    slp = SLPInterpolator(types.SimpleNamespace(ctx=gpu_ctx), gm["weights"], gm["means"], gm["covs"])
    host = np.stack([slp.optimise(starts[i], ends[i], n_step=n_step, n_iter=10, lr=LR, init=init[i])[0] for i in range(8)])
    d_host = np.abs(host - ref["pts"]).max()
    _, state, rec = Device(gpu_ctx, gm).run(starts, ends, init, 10, clip=1.0)
    d_dev = np.abs(state[0] - ref["pts"]).max()
    print("K %d R %d n %d: d_host %.3e, device %.3e, nearest |g| to 1: %.2e, clipped elements: %.0f %%" % (K, R, n_step, d_host, d_dev, nearest, 100 * clipped))
    assert d_dev <= 4 * d_host + 1e-7, (d_dev, d_host)
    # the recorded loss of every iteration: test 1's bar for the fp32 mixture sum, plus (first order, with a factor 2) what the allowed
    # point deviation moves the objective by -- the sum of the path's |gradient| elements times that deviation
    slack = 2 * np.abs(ref["grads"]).sum((2, 3)).T * (4 * d_host + 1e-7)
    assert (np.abs(rec[:, :, 0] - ref["loss"]) <= NLL_REL * np.abs(ref["neg_ll"]) + NLL_ABS + slack).all()


# ------------------------------------------------------------------------------------------------ 4. independence, resume, repeatability
def test_independence_and_resume_bitwise(gpu_ctx):
    gm = mixture(30, 16)
    dev = Device(gpu_ctx, gm)
    starts, ends, init = draw_paths(33, 33, 5, 16)
    pts, state, rec = dev.run(starts, ends, init, 60)
    assert np.isfinite(pts).all() and np.isfinite(state).all() and np.isfinite(rec).all()
    # path 17 alone
    p1, s1, r1 = dev.run(starts[17:18], ends[17:18], init[17:18], 60)
    assert np.array_equal(p1[0], pts[17]) and np.array_equal(s1[:, 0], state[:, 17]) and np.array_equal(r1[0], rec[17])
    # 60 iterations = 3 x 20 chained through the state (the incoming points are ignored when t0 > 0)
    pa, sa, ra = dev.run(starts, ends, init, 20)
    pb, sb, rb = dev.run(starts, ends, np.full_like(init, np.nan), 20, t0=20, state=sa)
    pc, sc, rc = dev.run(starts, ends, np.full_like(init, np.nan), 20, t0=40, state=sb)
    assert np.array_equal(pc, pts) and np.array_equal(sc, state) and np.array_equal(np.concatenate([ra, rb, rc], 1), rec)
    assert not np.array_equal(pa, pts)
    # twice the same call
    p2, s2, r2 = dev.run(starts, ends, init, 60)
    assert np.array_equal(p2, pts) and np.array_equal(s2, state) and np.array_equal(r2, rec)


# ------------------------------------------------------------------------------------------------ 5. optimise_batch
def test_chained_launches_equal_one(gpu_ctx, monkeypatch):
    """optimise_batch on a wide mixture: launches chained through the float64 state equal one launch; record=False gives the same points."""
    from ladder_latent_data_distribution_modelling_amd.codes import interpolation as I
    gm = mixture(30, 16)
    slp = I.SLPInterpolator(types.SimpleNamespace(ctx=gpu_ctx), gm["weights"], gm["means"], gm["covs"])
    assert slp.mixture.dense
    starts, ends, init = draw_paths(7, 3, 4, 16)
    pts, rec = slp.optimise_batch(starts, ends, n_step=4, n_iter=50, init=init)
    pts3, rec3 = slp.optimise_batch(starts, ends, n_step=4, n_iter=50, init=init, record=False)
    assert rec3 is None and np.array_equal(pts3, pts)
    monkeypatch.setattr(I, "MAX_ITER_PER_LAUNCH", 16)
    pts2, rec2 = slp.optimise_batch(starts, ends, n_step=4, n_iter=50, init=init)
    assert np.array_equal(pts, pts2) and all(np.array_equal(rec[k], rec2[k]) for k in rec)


def test_notebook_settings_properties(gpu_ctx):
    """The notebook's settings (linspace start, its weights) for 4 pairs, 100 iterations: properties only -- such a trajectory is
    chaotic, so it is compared with no other implementation."""
    from ladder_latent_data_distribution_modelling_amd.codes.interpolation import SLPInterpolator
    from ladder_latent_data_distribution_modelling_amd.codes.utils import count_trainable_variables
    gm = mixture(30, 16)
    slp = SLPInterpolator(types.SimpleNamespace(ctx=gpu_ctx), gm["weights"], gm["means"], gm["covs"])
    starts, ends, _ = draw_paths(15, 4, 5, 16)
    pts, rec = slp.optimise_batch(starts, ends, n_step=5, n_iter=100)
    assert pts.shape == (4, 5, 16) and pts.dtype == np.float64 and np.isfinite(pts).all()
    assert np.array_equal(pts, pts.astype(np.float32).astype(np.float64))                       # the fp32 results
    assert sorted(rec) == ["loss", "neg_ll", "path_length", "step_var"]
    assert all(v.shape == (4, 100) and np.isfinite(v).all() for v in rec.values())
    assert rel(rec["loss"], W_PATH * rec["path_length"] + W_EQUAL * rec["step_var"] + rec["neg_ll"]).max() <= 1e-12
    assert count_trainable_variables("interpolation") == 4 * 5 * 16
    # the first record row is the objective at the (fp32-rounded) linspace points between exactly these end points
    lin = np.stack([np.linspace(s, e, 6, endpoint=False)[1:] for s, e in zip(starts, ends)]).astype(np.float32).astype(np.float64)
    full = np.concatenate([starts[:, None], lin, ends[:, None]], 1)
    ln = np.sqrt(((full[:, 1:] - full[:, :-1]) ** 2).sum(-1))
    assert rel(rec["path_length"][:, 0], ln.sum(1)).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ 6. ABI limits
def test_abi_limits(gpu_ctx):
    L = _L()
    q, st = L.query, gpu_ctx.stream
    sb = lambda *a: q("ladder_slp_wide_state_bytes", *a)
    assert sb(7, 5, 16) == 3 * 7 * 5 * 16 * 8 and sb(1, 32, 64) == 3 * 32 * 64 * 8 and sb(2, 64, 32) == 3 * 2 * 64 * 32 * 8
    assert sb(0, 5, 16) == 0 and sb(1, 0, 16) == 0 and sb(1, 65, 16) == 0 and sb(1, 5, 8) == 0 and sb(1, 5, 10) == 0 and sb(1, 5, 68) == 0
    assert sb(1, 57, 36) == 0                                                                   # n_step * R = 2052
    P, n, R, K = 3, 5, 16, 6
    s, e = torch.zeros(P, 64, device="cuda"), torch.ones(P, 64, device="cuda")
    pts = torch.full((P, 64, 64), 7.0, device="cuda")
    params = torch.zeros(L.query("ladder_gmm_dense_param_floats", 1025, 68), device="cuda")
    state = torch.full((3 * P * 64 * 64,), 7.0, dtype=torch.float64, device="cuda")
    rec = torch.full((P, 4, 4), 7.0, dtype=torch.float64, device="cuda")

    def call(K=K, R=R, P=P, n=n, n_iter=4, t0=0, s=s.data_ptr(), e=e.data_ptr(), pts=pts.data_ptr(), params=params.data_ptr(), state=state.data_ptr(),
             entry="ladder_slp_wide_optimise"):
        return q(entry, s, e, pts, params, K, R, P, n, n_iter, t0, LR, 0.9, 0.95, 1e-8, 1.0, W_PATH, W_EQUAL, state, rec.data_ptr(), st)

    assert call(R=8) == E_SHAPE and call(R=10) == E_SHAPE and call(R=68) == E_SHAPE
    assert call(K=0) == E_SHAPE and call(K=1025) == E_SHAPE
    assert call(n=0) == E_SHAPE and call(n=65) == E_SHAPE
    assert call(n=57, R=36) == E_SHAPE                                                          # n_step * R = 2052 with n_step <= 64
    assert call(P=0) == E_SHAPE and call(P=-1) == E_SHAPE
    assert call(n_iter=0) == E_SHAPE and call(n_iter=4097) == E_SHAPE
    assert call(t0=-1) == E_SHAPE
    assert call(t0=4, state=None) == E_SHAPE
    assert call(s=None) == E_SHAPE and call(e=None) == E_SHAPE and call(pts=None) == E_SHAPE and call(params=None) == E_SHAPE
    assert call(entry="ladder_slp_optimise") == E_SHAPE                                         # the narrow entry stays at R <= 8
    torch.cuda.synchronize()
    assert torch.all(pts == 7.0) and torch.all(state == 7.0) and torch.all(rec == 7.0)          # a rejected call launched nothing
    assert torch.all(s == 0.0) and torch.all(e == 1.0) and torch.all(params == 0.0)


# ------------------------------------------------------------------------------------------------ 7. the trainer
def test_trainer_interpolates_wide_representation(golden_dir):
    from ladder_latent_data_distribution_modelling_amd.codes import models as M
    from ladder_latent_data_distribution_modelling_amd.codes.base import BaseTrain_joint
    from ladder_latent_data_distribution_modelling_amd.codes.interpolation import SLPInterpolator
    from ladder_latent_data_distribution_modelling_amd.codes.session import Session
    d = np.load(os.path.join(golden_dir, "oracle_mnist_digit.npz"))
    R = 16
    cfg = dict(json.loads(str(d["config"])), prior="ours", representation_size=R, checkpoint_dir="/tmp/", result_dir="/tmp/res/")
    model = M.MNISTModel_digit(cfg, device="cuda:0", seed=1)
    tr = BaseTrain_joint(Session(), model, None, cfg)
    tr.cur_epoch = 3
    K = int(cfg["n_mixtures"])
    syn = O.synthetic_gm(dict(n_mixtures=K, representation_size=R), np.random.default_rng(K * 7 + R))
    gm = tuple(syn[k].astype(np.float32) for k in ("weights", "means", "covs"))
    P, n_step = 6, 5
    starts, ends, init = draw_paths(3, P, n_step, R)
    with pytest.raises(RuntimeError, match="not been fitted"):
        tr.interpolate_paths(starts, ends, mode="crude-GM")
    tr.gm_params = tr.gm_final_params = gm
    pts, rec, imgs = tr.interpolate_paths(starts, ends, n_step=n_step, n_iter=20, init=init)
    H, W, C = (int(cfg[k]) for k in ("dim_input_x", "dim_input_y", "dim_input_channel"))
    assert pts.shape == (P, n_step, R) and rec["loss"].shape == (P, 20) and imgs.shape == (P, n_step + 2, H, W, C)
    assert np.isfinite(pts).all() and np.isfinite(rec["loss"]).all() and imgs.min() >= 0.0 and imgs.max() <= 1.0
    pts_c, _, none = tr.interpolate_paths(starts, ends, mode="crude-GM", n_step=n_step, n_iter=20, init=init, decode=False, record=False)
    assert none is None and np.array_equal(pts_c, pts)                                      # the same mixture under both names
    slp = SLPInterpolator(tr.engine, *gm)
    assert np.array_equal(imgs, slp.decode_paths(starts, pts, ends))
    with pytest.raises(ValueError, match=r"\[P, 16\]"):
        tr.interpolate_paths(starts[:, :2], ends[:, :2])
    # R = 10: refused with the R % 4 message, by the trainer and by the interpolator, not by an error of the mixture preparation
    tr10 = types.SimpleNamespace(config=dict(cfg, representation_size=10), gm_params=gm, gm_final_params=gm)
    with pytest.raises(ValueError, match=r"R % 4 == 0"):
        BaseTrain_joint.interpolate_paths(tr10, np.zeros((2, 10)), np.zeros((2, 10)))
    with pytest.raises(ValueError, match=r"R % 4 == 0"):
        SLPInterpolator(tr.engine, np.ones(3, np.float32) / 3, np.zeros((3, 10), np.float32), np.stack([np.eye(10, dtype=np.float32)] * 3))
