"""Host-side driver of the HIP LaDDer path: the three reference architectures and the four per-minibatch "runs" of the reference iteration
(codes/base.py:583-641) on top of layers.py (device context, parameter store, layers with explicit backward), comm.py (exchange steps C1-C4) and
profiler.py.  PyTorch supplies device memory, streams and torch.distributed only; every arithmetic op is a call into libladder_hip.so (see _lib.py)
-- there is no CPU path.
"""
import os

import numpy as np
import torch

from . import _lib as L
from . import arch
from . import layers as _layers
from .comm import Comm, VirtualComm, VirtualGroup, run_virtual_ranks, _NoComm, _DoneWork, _TracedWork  # noqa: F401  (re-exported: tests, bench.py)
from .layers import (ADAM_B1, ADAM_B2, ADAM_EPS, BN_EPS, DEFAULT_PRECISION, IN_EPS, PRECISION_NOTES, PRECISIONS, BatchNormAct, Conv2D, Ctx, Dense,  # noqa: F401
                     DepthToSpace, InstanceNormStyleAct, ParamStore, PlanesOnly, Resize, _p, _timed, add_, pad_symmetric, plan_decoder)
from .mixture import DeviceMixture, DiagMixture
from .mixture_forms import check_status_word, family, sized_workspace
from .profiler import KernelProfiler  # noqa: F401


def set_profiler(prof):
    """Install (or, None, remove) the KernelProfiler that brackets the contraction launches of layers.py with HIP events (bench.py's roofline leg)."""
    _layers.PROF = prof


# ------------------------------------------------------------------------------------------ networks
class Encoder:
    def __init__(self, ctx, ps, cfg):
        self.ctx, self.cfg = ctx, cfg
        self.exp = cfg["exp_name"]
        self.convs, self.bns = [], []
        for i, (cin, cout, k, s, pad, act, bn) in enumerate(arch.encoder_convs(cfg)):
            self.convs.append(Conv2D(ctx, ps, "encoder/" + arch.tfname("conv2d", i), k, cin, cout, s, pad, act, bias_grad=not bn, want_bn_sums=bool(bn)))
            self.bns.append(BatchNormAct(ctx, ps, "encoder/" + arch.tfname("batch_normalization", i), cout, "leaky_relu") if bn else None)
        feat, hid = arch.encoder_flat_dim(cfg), arch.encoder_hidden(cfg)
        self.hidden = Dense(ctx, ps, "encoder/dense", feat, hid, "leaky_relu") if hid is not None else None
        feat = hid if hid is not None else feat
        Z = int(cfg["code_size"])
        self.head_mu = Dense(ctx, ps, "encoder/code_mean", feat, Z, None)
        self.head_sd = Dense(ctx, ps, "encoder/code_std_dev", feat, Z, "relu")

    def forward(self, x):
        h = pad_symmetric(self.ctx, x, 2) if self.exp != "celeba" else x
        for i, (conv, bn) in enumerate(zip(self.convs, self.bns)):
            h = conv.forward(h)
            if bn is not None:
                nxt = self.convs[i + 1] if i + 1 < len(self.convs) else None
                h = bn.forward(h, sums=conv.bn_sums, planes=nxt.planes_demand(h.shape) if nxt is not None else (False, True))
            conv.bn_sums = None
        self.conv_shape = h.shape
        h = h.reshape(h.shape[0], -1)
        if self.hidden is not None:
            h = self.hidden.forward(h)
        return self.head_mu.forward(h), self.head_sd.forward(h)

    def backward(self, dmu, dsd_raw, wgrad=True, need_input_dx=False):
        """`need_input_dx`: also return d loss / d x (only the VampPrior pseudo-inputs are trainable inputs)."""
        dh = self.head_mu.backward(dmu, wgrad=wgrad)
        add_(self.ctx, dh, self.head_sd.backward(dsd_raw, wgrad=wgrad, act_done=True))
        if self.hidden is not None:
            dh = self.hidden.backward(dh, wgrad=wgrad)
        dh = dh.reshape(self.conv_shape)
        for i in range(len(self.convs) - 1, -1, -1):
            if self.bns[i] is not None:
                dh = self.bns[i].backward(dh, wgrad=wgrad)
            dh = self.convs[i].backward(dh, need_dx=(i > 0 or need_input_dx), wgrad=wgrad)
        if need_input_dx and self.exp != "celeba":                 # undo the SYMMETRIC 28 -> 32 pad
            N, Hp, Wp, C = dh.shape
            dx = self.ctx.empty(N, Hp - 4, Wp - 4, C)
            L.call("ladder_pad_symmetric_bwd", _p(dh), _p(dx), N, Hp - 4, Wp - 4, C, 2, self.ctx.stream)
            dh = dx
        return dh if need_input_dx else None


class MnistDecoder:
    def __init__(self, ctx, ps, cfg):
        self.ctx = ctx
        width, r0, convs = arch.mnist_decoder_convs(cfg)
        self.dense = Dense(ctx, ps, "decoder/dense", int(cfg["code_size"]), width, "leaky_relu")
        self.d2s0 = DepthToSpace(ctx, r0)
        self.convs, self.d2s = [], []
        for i, (k, ci, co, pad, act, d) in enumerate(convs):
            self.convs.append(Conv2D(ctx, ps, "decoder/" + arch.tfname("conv2d", i), k, ci, co, 1, pad, act))
            self.d2s.append(DepthToSpace(ctx, d) if d else None)

    def forward(self, z):
        h = self.dense.forward(z)
        h = self.d2s0.forward(h.view(h.shape[0], 1, 1, -1))
        for conv, d in zip(self.convs, self.d2s):
            h = conv.forward(h)
            if d is not None:
                h = d.forward(h)
        return h

    def backward(self, dxhat, need_dz=True):
        dh = dxhat
        for conv, d in zip(reversed(self.convs), reversed(self.d2s)):
            if d is not None:
                dh = d.backward(dh)
            dh = conv.backward(dh)
        dh = self.d2s0.backward(dh)
        return self.dense.backward(dh.reshape(dh.shape[0], -1), need_dx=need_dz)


class CelebADecoder:
    """codes/models.py:499-587: mapping MLP -> dlatent; 1x1 conv on `encoded`; 7 3x3 convs with
    IN+style+leaky on four of them and legacy-bilinear upsampling in between; 1x1 conv to RGB."""

    def __init__(self, ctx, ps, cfg):
        self.ctx = ctx
        nh, Z = int(cfg["num_hidden_units"]), int(cfg["code_size"])
        self.nh = nh
        self.dense0 = Dense(ctx, ps, "decoder/dense", Z, nh, "leaky_relu")
        self.mapping = [Dense(ctx, ps, "decoder/dense_%d" % i, nh, nh, "leaky_relu") for i in range(1, 9)]
        self.conv0 = Conv2D(ctx, ps, "decoder/conv2d", 1, nh, nh, 1, "same", None)
        self.up0 = Resize(ctx, 2, 2)
        self.blocks = []
        si = 0
        for i, (k, ci, co, styled, act, rs) in enumerate(arch.celeba_decoder_convs(cfg)):
            conv = Conv2D(ctx, ps, "decoder/conv2d_%d" % (i + 1), k, ci, co, 1, "same", act, bias_grad=not styled)
            sty = norm = None
            if styled:
                sty = Dense(ctx, ps, "decoder/StyleMod_%d/dense" % si, nh, 2 * co, None)
                norm = InstanceNormStyleAct(ctx, co, "leaky_relu")
                si += 1
            self.blocks.append((conv, sty, norm, Resize(ctx, rs, rs) if rs else None))
        self.conv_out = Conv2D(ctx, ps, "decoder/conv2d_8", 1, nh // 4, int(cfg["dim_input_channel"]), 1, "same", None)
        self._plans, self.plan = {}, None       # plan_decoder's cache; the plan of the last training forward

    def forward(self, z):
        B = z.shape[0]
        encoded = self.dense0.forward(z)
        d = encoded
        for lyr in self.mapping:
            d = lyr.forward(d)
        dlatent = d
        keep = self.ctx.keep_activations
        h = self.conv0.forward(encoded.view(B, 1, 1, self.nh))
        plan = plan_decoder(self._plans, self.ctx, self.up0, self.blocks, self.conv_out, tuple(h.shape[:3]))
        if keep:
            self.plan = plan          # (the backward pass follows the plan of the training forward, not those of the forward-only runs in between)
        # h: the tensor at the next conv's resolution (None where the plan never materialises it); lo: the low-resolution tensor behind it where
        # the conv reads that one.  The 1x1 -> 2x2 resize in front of conv2d_1 folds into it like every other one
        h, lo = (None, h) if plan[0].resize in ("virtual", "fold_forward_only") else (self.up0.forward(h), None)
        for e, (conv, sty, norm, rs) in zip(plan, self.blocks):
            proj = self.conv_out if e.proj else None
            if e.form != "plain":
                h = conv.forward_up2(lo, e, proj, keep_y=keep, upsampled=h)
            elif proj is not None:        # the last 3x3 conv feeds the 1x1 output conv directly (its resize is the identity): one fused launch
                h = conv.forward_fused_proj(h, proj, keep_y=keep)
            else:
                h = conv.forward(h)
            if proj is not None:
                return h
            lo = None
            if norm is not None:
                style = sty.forward(dlatent)
                h, lo = (norm.forward(h, style), None) if e.norm_out == "lowres" else norm.forward_resized(h, style, rs, e.norm_out == "both")
            if e.behind in ("virtual", "fold_forward_only"):
                h, lo = None, h
            elif e.behind is not None and e.norm_out in (None, "lowres"):
                # (keep_both behind an un-normalised layer -- conv2d_5: its output IS the low-resolution tensor)
                h, lo = rs.forward(h), (h if e.behind == "keep_both" else None)
        return self.conv_out.forward(h)

    def backward(self, dxhat, need_dz=True):
        ctx, plan = self.ctx, self.plan
        # the last 3x3 conv feeds conv_out directly (its resize is the identity at full resolution): its leaky-ReLU backward is fused into conv_out's
        # backward-data epilogue (saves a read+write pass over the largest map) -- and where that conv ran in the projected form, its backward combination
        # is formed straight from dxhat: neither the 1x1 conv's backward-data result nor the read of it exist, and conv_out's filter / bias gradient comes
        # out of the same launch
        last = plan[-1]
        dh = None if last.proj_grad else self.conv_out.backward(dxhat, gate_prev=self.blocks[-1][0].act if last.fuse_last else None)
        ddlat = None
        for i in range(len(self.blocks) - 1, -1, -1):
            e, (conv, sty, norm, rs) = plan[i], self.blocks[i]
            if e.gated:               # leaky conv -> resize: its activation backward rides on the transpose
                dh, _ = rs.backward(dh, gate=(conv.kept.y, conv.act))
            elif e.rs_bwd:
                dh = rs.backward(dh)
            if norm is not None:
                dh, dstyle = norm.backward(dh)
                g = sty.backward(dstyle)
                ddlat = g if ddlat is None else add_(ctx, ddlat, g)
            # (lowres_dx: the block below ends in a resize and this conv's backward-data returns the gradient of the resize's INPUT; lgate: that block's own
            # activation backward rides on it when it is an un-normalised leaky conv -- conv2d_5 under conv2d_6)
            below = self.blocks[i - 1][0]
            dh = conv.backward(dh, act_done=e.fuse_last or e.gated or e.pre_gated, lowres_dx=e.lowres_dx,
                               lowres_gate=(below.kept.y, below.act) if e.lgate else None, proj_grad=(dxhat, self.conv_out) if e.proj_grad else None)
        dh = self.conv0.backward(dh if plan[0].lowres_dx else self.up0.backward(dh))     # (lowres_dx: conv2d_1 returned the gradient of the 1x1 map itself)
        denc = dh.reshape(dh.shape[0], self.nh)
        # mapping MLP: each layer's backward-data epilogue applies the previous layer's leaky-ReLU derivative
        for i in range(len(self.mapping) - 1, -1, -1):
            ddlat = self.mapping[i].backward(ddlat, act_done=(i < len(self.mapping) - 1), gate_prev="leaky_relu" if i > 0 else None)
        add_(ctx, denc, ddlat)
        return self.dense0.backward(denc, need_dx=need_dz)


class InnerVAE:
    """codes/base.py:127-213."""

    def __init__(self, ctx, ps, cfg):
        self.ctx = ctx
        Z, H = int(cfg["code_size"]), int(cfg["num_hidden_units_inner_VAE"])
        R, nl = int(cfg["representation_size"]), int(cfg["n_layers_inner_VAE"])
        a = cfg["inner_activation"]
        dims = [(Z, H)] + [(H, H)] * (nl - 1)
        self.enc = [Dense(ctx, ps, "prior/" + arch.tfname("dense", i), ci, co, a) for i, (ci, co) in enumerate(dims)]
        self.head_mu = Dense(ctx, ps, "prior/" + arch.tfname("dense", nl), H, R, None)
        self.head_sd = Dense(ctx, ps, "prior/" + arch.tfname("dense", nl + 1), H, R, "relu")
        dims = [(R, H)] + [(H, H)] * (nl - 1)
        self.dec = [Dense(ctx, ps, "prior/" + arch.tfname("dense", nl + 2 + i), ci, co, a) for i, (ci, co) in enumerate(dims)]
        self.dec_out = Dense(ctx, ps, "prior/" + arch.tfname("dense", 2 * nl + 2), H, Z, None)

    def encode(self, z):
        h = z
        for lyr in self.enc:
            h = lyr.forward(h)
        return self.head_mu.forward(h), self.head_sd.forward(h)

    def decode(self, t):
        h = t
        for lyr in self.dec:
            h = lyr.forward(h)
        return self.dec_out.forward(h)

    def decode_backward(self, dzhat, wgrad):
        # every backward-data epilogue applies the activation derivative of the layer below it (its input)
        a = self.dec[0].act
        dh = self.dec_out.backward(dzhat, wgrad=wgrad, gate_prev=a)
        for i in range(len(self.dec) - 1, -1, -1):
            dh = self.dec[i].backward(dh, wgrad=wgrad, act_done=True, gate_prev=a if i > 0 else None)
        return dh

    def encode_backward(self, dmu, dsd_raw, wgrad, need_dz):
        dh = self.head_mu.backward(dmu, wgrad=wgrad)
        add_(self.ctx, dh, self.head_sd.backward(dsd_raw, wgrad=wgrad, act_done=True))
        a = self.enc[0].act
        for i in range(len(self.enc) - 1, -1, -1):
            # the head gradients were summed with a separate add, so the top hidden layer applies its own activation
            # derivative; below it each backward-data epilogue carries the derivative of the layer underneath
            dh = self.enc[i].backward(dh, need_dx=(need_dz or i > 0), wgrad=wgrad, act_done=(i < len(self.enc) - 1),
                                      gate_prev=a if i > 0 else None)
        return dh


class _AsyncFetch:
    """Handle of LadderEngine.fetch_async()."""

    def __init__(self, host, event, names, pool, undefined=()):
        self._host, self._event, self._names, self._pool, self._val = host, event, names, pool, None
        self._undefined = frozenset(undefined)

    def ready(self):
        """True when get() would not block."""
        return self._val is not None or self._event.query()

    def get(self):
        if self._val is None:
            self._event.synchronize()
            s = self._host.numpy()
            self._val = {n: (float("nan") if n in self._undefined else float(s[L.S_INDEX[n]])) for n in self._names}
            self._pool.append(self._host)          # the pinned buffer goes back to the engine's pool
            self._host = None
        return self._val


# scalars that exist only when the decoder ran (RUN#3 / RUN#4, sample_code, sample_representation evaluate encoder + inner VAE only)
DEC_SCALARS = frozenset(("sigma", "mean_pixel_error", "l1_reconstruction_error", "l2_reconstruction_error", "reconstruction_likelihood",
                         "sigma_regularisor", "elbo", "loss_ae"))


PRIOR_METHODS = arch.PRIOR_METHODS


class PriorSampler:
    """Handle of LadderEngine.prior_sampler(): ancestral samples of one prior, drawn on the device (reference codes/base.py:1065-1122).

    Owns the prepared parameter buffer of csrc/sample.hip (one layout for both of its families).
    Its Philox stream is its own -- (seed, offset) of this object, never the engine's training noise position -- and sample index i draws the same values whatever the chunking: sample(n, first) returns samples
    first .. first+n-1 of ONE stream, so a bulk run may be cut into chunks (or, later, sharded over ranks) freely."""

    def __init__(self, eng, method, form, K, R, params, seed=0, offset=0):
        """`form`: the row of operation "sampler" (mixture_forms.py) whose `prepare` filled `params`."""
        self.eng, self.method, self.form, self.K, self.R, self.params = eng, method, form, int(K), int(R), params
        self.seed, self.offset = int(seed), int(offset)
        self.to_code = method in ("ours", "hierarchical")      # the draw is t: the code is the inner decoder's output (base.py:1088-1118)

    def sample(self, n, first=0, noise=None, seed=None):
        """-> (code [n, Z], latent [n, R or Z], comp [n] int32), device tensors.  `noise` = {"u": [n], "eps": [n, R]} feeds the draws."""
        eng, n = self.eng, int(n)
        ctx = eng.ctx
        latent = ctx.empty(n, self.R)
        comp = torch.empty(n, dtype=torch.int32, device=ctx.device)
        u = eps = None
        if noise is not None:
            u, eps = eng._dev(noise["u"]).reshape(-1), eng._dev(noise["eps"])
            if tuple(u.shape) != (n,) or tuple(eps.shape) != (n, self.R):
                raise ValueError("noise: u %s, eps %s; expected (%d,) and (%d, %d)" % (tuple(u.shape), tuple(eps.shape), n, n, self.R))
        L.call(self.form.sample, _p(self.params), self.K, self.R, n, int(first), _p(u), _p(eps),
               self.seed if seed is None else int(seed), self.offset, _p(latent), _p(comp), ctx.stream)
        code = eng.decode_representation(latent) if self.to_code else latent
        return code, latent, comp


# ------------------------------------------------------------------------------------------ engine
class LadderEngine:
    """Owns parameters + optimiser state and evaluates the reference's four per-minibatch runs.

    run_ae          = RUN#1  (codes/base.py:587-594)   full fwd+bwd, clip+Adam on encoder+decoder
    run_sigma       = RUN#2  (601-606)                 encoder+decoder fwd, scalar Adam on sigma/Variable
    run_prior       = RUN#3  (615-622)                 encoder fwd, inner-VAE fwd+bwd, Adam on prior/*
    run_inner_sigma = RUN#4  (636-639)                 encoder + inner-VAE fwd, scalar Adam on inner_sigma
    evaluate        = val_step / test_step fetches     (643-679, 944-986)
    """

    def __init__(self, cfg, device="cuda:0", values=None, seed=1, comm=None, noise_seed=1234):
        self.cfg = cfg
        if comm is None and bool(int(cfg.get("deterministic_allreduce", 0))):
            comm = Comm(deterministic=True)
        self.ctx = Ctx(device, comm)
        prec = str(cfg.get("matmul_precision", DEFAULT_PRECISION))
        if prec not in PRECISIONS:
            raise ValueError("matmul_precision %r: expected one of %s" % (prec, sorted(PRECISIONS)))
        self.ctx.ns = PRECISIONS[prec]
        # 0: off, 1: forward-only runs, 2: also the training forward and the backward-data of the last 3x3 conv, 3: also conv2d_6's backward-data (no gain measured)
        # (strict fp32 default 3: with the fp32 MFMA the 11 / 36 of conv2d_6's backward-data outweigh its border strips, +0.5 %; f16x3: no gain, 2)
        self.ctx.up2 = int(cfg.get("upsample_fused_convs", 4 if prec == "f32" else 2))
        # (default 2: in the whole iteration fusing EVERY eligible pair measured fastest -- 19.24 ms against 19.39 with only the pairs that win as isolated
        # launches and 19.81 with none, same box, profiles/r06_f32_bench_fused_level*.json: a pair that is level in isolation still spares its neighbours 1.2 GB
        # of HBM traffic and an allocation)
        self.ctx.fuse_fwd = int(cfg.get("fused_projected_forward", 2))
        self.ctx.fuse_bwd_proj = int(cfg.get("fused_projection_backward", 1))
        self.precision = prec
        if self.ctx.comm.rank == 0:
            print("Contraction precision (config key matmul_precision): {} -- {}".format(prec, PRECISION_NOTES[prec]))
        self.ps = ParamStore(cfg, self.ctx, values, seed)
        self.encoder = Encoder(self.ctx, self.ps, cfg)
        self.decoder = (CelebADecoder if cfg["exp_name"] == "celeba" else MnistDecoder)(self.ctx, self.ps, cfg)
        self.has_inner = cfg["prior"] in ("ours", "hierarchical")
        self.hier = cfg["prior"] == "hierarchical"          # inner VAE against N(0,I): no mixture term, no mask (base.py:331-359)
        self.gmm_z = cfg["prior"] == "GMM"                   # mixture directly on z (R = code_size), no inner VAE (base.py:322-329)
        self.vamp = cfg["prior"] == "vampPrior"              # diagonal mixture on z from trainable pseudo-inputs (base.py:216-254)
        if cfg["prior"] not in ("ours", "hierarchical", "GMM", "vampPrior", "standard_gaussian"):
            raise ValueError("unknown prior %r" % cfg["prior"])
        if self.vamp:
            # second pass of the SAME encoder weights over the K pseudo-inputs (tf.variable_scope('encoder', reuse=True)); the
            # pseudo-inputs are replicated on every rank, so its batch-norm statistics are not exchanged
            self.encoder_p = Encoder(self.ctx.local(), self.ps, cfg)
            self._enc_range = self.ps.prefix_range("ae", "encoder/")
        self.inner = InnerVAE(self.ctx, self.ps, cfg) if self.has_inner else None
        self.Z = int(cfg["code_size"])
        self.R = int(cfg["code_size"]) if cfg["prior"] in ("GMM", "vampPrior") else int(cfg.get("representation_size", 1))   # mixture dimension
        self.K = int(cfg.get("n_mixtures", 1))
        self.Lmc = int(cfg.get("n_MC_samples", 1))
        self.D = int(cfg["dim_input_x"]) * int(cfg["dim_input_y"]) * int(cfg["dim_input_channel"])
        self.lvp = float(cfg["latent_variance_precision"])
        self.partials = self.ctx.zeros(L.P_FIXED + self.Z + self.R)
        self.scalars = self.ctx.zeros(L.S_COUNT)
        self.noise_seed = int(noise_seed) + 7919 * self.ctx.comm.rank
        self.rng_counter = torch.zeros(1, dtype=torch.int64, device=self.ctx.device)   # Philox stream position (device)
        self._run_calls = 0
        self.mixture = None                                  # DeviceMixture, once set_mixture() / set_sg_mixture() was called
        self.vamp_mixture = DiagMixture(self.ctx, self.K, self.Z) if self.vamp else None
        self.use_graphs = False
        # filter gradients on a second stream beside the backward chain (config key `overlap_filter_gradients` / environment variable
        # LADDER_OVERLAP_FILTER_GRADIENTS): +0.7-1 % per iteration with the f16x3 kernels, nothing with the fp32 ones (round 4: 3 328 / 3 327 img/s --
        # both partners are bound by the fp32 matrix pipe), bit-identical results -- OFF by default because kernels that share the
        # chip stretch each other, so the per-kernel HIP-event durations bench.py reports (roofline.achieved) stop describing the kernels
        if bool(int(cfg.get("overlap_filter_gradients", os.environ.get("LADDER_OVERLAP_FILTER_GRADIENTS", 0)))):
            self.ctx.side = torch.cuda.Stream(device=self.ctx.device)
        self._graphs, self._warm = {}, {}
        self._dec_range = self.ps.prefix_range("ae", "decoder/")   # C1 bucket boundary (data parallel)
        # RUN#3 / RUN#4 on their own HIP stream beside RUN#2's decoder forward (enable_prior_overlap; the trainer turns it on)
        self.ps.before_read = self._join_aux
        self._aux_on = False
        self._enc_event, self._aux_event = None, None              # "z of the last main-stream forward exists" / "the aux runs are done"
        self._main_calls, self._aux_calls = 0, 0                    # noise calls of the last main forward / of the aux runs since
        self._on_aux = False
        self._fetch_src = None                                      # (scalars buffer, stream) of the last run
        self._sigma_one = torch.ones(1, dtype=torch.float32, device=self.ctx.device)   # stand-in for sigma/Variable in decoder-less runs

    def enable_prior_overlap(self, on=True):
        """RUN#3 and RUN#4 (inner VAE forward / backward, mixture term, Adam on prior/* and inner_sigma: ~150 launches of a few
        microseconds, 0.9 ms of latency-bound chain on CelebA) read only the encoder output that RUN#2 computes FIRST and write only the
        prior variables, which RUN#2 never touches: with this on, run_prior / run_inner_sigma called with reuse_encoder=True are
        enqueued on a second HIP stream behind an event recorded right after RUN#2's code sample, and run beside RUN#2's decoder
        forward (big MFMA-bound kernels).  Separate partials / scalars buffers and scratch; the noise positions are those of the
        sequential order (snapshot of the device counter + host-known call counts), so results are bit-identical to the sequential
        schedule.  The next main-stream run waits for the aux stream first.  Off under data parallelism (collectives stay on one
        stream) and with hipGraph replay."""
        on = bool(on) and not self.ctx.comm.on
        self._aux_on = on
        if on and self.ctx.aux is None:
            # (high priority: its few-microsecond kernels should not queue behind the thousands of workgroups of a decoder conv)
            self.ctx.aux = torch.cuda.Stream(device=self.ctx.device, priority=int(os.environ.get("LADDER_AUX_PRIORITY", -1)))
            self.partials_aux, self.scalars_aux = torch.zeros_like(self.partials), torch.zeros_like(self.scalars)
            self.rng_counter_aux = torch.zeros_like(self.rng_counter)

    def _join_aux(self):
        """The main stream waits for the runs enqueued on the aux stream (no-op when none are pending)."""
        if self._aux_event is not None:
            torch.cuda.current_stream(self.ctx.device).wait_event(self._aux_event)
            self._aux_event = None
            self._aux_calls = 0

    # -- inputs ---------------------------------------------------------------------------------
    def _dev(self, a):
        if a is None:
            return None
        if isinstance(a, torch.Tensor):
            return a.to(device=self.ctx.device, dtype=torch.float32).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(self.ctx.device)

    @staticmethod
    def _batch_token(x):
        """(address, shape) of a minibatch as the caller holds it: the key of the encoder-output cache."""
        if isinstance(x, torch.Tensor):
            return ("t", x.data_ptr(), tuple(x.shape))
        a = np.asarray(x)
        return ("n", a.__array_interface__["data"][0], tuple(a.shape))

    def _randn(self, *shape):
        t = self.ctx.empty(*shape)
        if self._on_aux:      # sequential position: the counter as RUN#2 saw it + RUN#2's calls + the earlier aux runs' calls + this run's
            L.call("ladder_randn_dev", _p(t), t.numel(), self.noise_seed, _p(self.rng_counter_aux),
                   self._main_calls + self._aux_calls + self._run_calls, self.ctx.stream)
        else:
            L.call("ladder_randn_dev", _p(t), t.numel(), self.noise_seed, _p(self.rng_counter), self._run_calls, self.ctx.stream)
        self._run_calls += 1
        return t

    def _noise(self, noise, key, shape):
        if noise is not None and noise.get(key) is not None:
            t = self._dev(noise[key])
            assert tuple(t.shape) == tuple(shape), (key, t.shape, shape)
            return t
        return self._randn(*shape)

    def set_mixture(self, weights, means, covs):
        """Feed of prior_weight / prior_mean / prior_cov (codes/base.py:110-112, 870-888); fp32 like the placeholders."""
        mix = self.mixture or DeviceMixture(self.ctx, self.K, self.R)    # persistent: captured graphs keep pointing at the current mixture
        mix.set(weights, means, covs)
        self.mixture = mix

    def set_sg_mixture(self):
        """The dummy N(0,I) mixture of the SG-pretraining feed (codes/base.py:870-876)."""
        K, R = self.K, self.R
        self.set_mixture(np.full(K, 1.0 / K), np.zeros((K, R)), np.tile(np.eye(R), (K, 1, 1)))

    # -- forward --------------------------------------------------------------------------------
    def forward(self, x, noise=None, use_sg=True, use_mask=False, parts=("dec", "inner", "gmm"), reuse_encoder=False, keep_acts=True):
        """`reuse_encoder`: the caller asserts that this run evaluates the SAME minibatch as the previous run and that no
        encoder variable changed in between (RUN#2/#3/#4 after RUN#1: only sigma / prior variables are updated,
        codes/base.py:601-639).  The encoder output (code_mean, code_std_dev) of the previous run is then bit-identical to
        what a re-evaluation would give (deterministic kernels, batch statistics of the same batch) and is reused; the
        fresh noise of the run still produces a new code_sample.  Guarded by the AE optimiser step counter."""
        ctx, st = self.ctx, self.ctx.stream
        if not self._on_aux:
            self._join_aux()                       # (prior variables / noise position: the aux runs of the last iteration come first)
            # whoever calls forward() on the main stream -- a run, evaluate(), sample_*, the Session facade -- fetches THIS forward's scalars
            # (evaluate() after an overlapped RUN#3 / RUN#4 used to read the aux run's stale buffer)
            self._fetch_src = (self.scalars, torch.cuda.current_stream(ctx.device))
        ctx.keep_activations = bool(keep_acts)     # forward-only runs (RUN#2, val_step): fused kernels skip backward-only tensors
        Z, R = self.Z, self.R
        P = self.partials
        L.call("ladder_axpy", None, _p(P), P.numel(), 0.0, 2, st)
        self._run_calls = 0
        use_mask = bool(use_mask) and not self.hier
        # identity of the minibatch the caller handed in (set by _run; direct callers of forward() are identified by their tensor)
        tok = self.__dict__.pop("_x_token", None) or self._batch_token(x)
        cache = getattr(self, "_enc_cache", None)
        if (reuse_encoder and cache is not None and cache[0] == self.ps.step["ae"] and cache[4] == tok
                and not self._enc_needs_grad(parts)):
            # the cached codes belong to ONE minibatch: a caller handing in another tensor (or shape) gets a fresh encoder pass, never
            # stale codes (an in-place refill of the same buffer must go through a run without reuse_encoder first)
            _, x, mu, sd_raw, _ = cache
        else:
            x = self._dev(x)
            mu, sd_raw = self.encoder.forward(x)
            self._enc_cache = (self.ps.step["ae"], x, mu, sd_raw, tok)
        B = x.shape[0]
        self.x, self.B = x, B
        self.Bg = B * ctx.comm.world
        eps_z = self._noise(noise, "eps_z", (B, Z))
        z, sd = ctx.empty(B, Z), ctx.empty(B, Z)
        L.call("ladder_latent_fwd", _p(mu), _p(sd_raw), _p(eps_z), self.lvp, _p(z), _p(sd), _p(P[L.P_LOG_SDZ:]),
               _p(P[L.P_MU2SD2_Z:]), _p(P[L.P_FIXED:]), B, Z, st)
        self.lat_z = (mu, sd, sd_raw, eps_z, z)
        # everything a following aux run reads from this forward exists now (the encoder output).  If this forward draws no further noise
        # (RUN#2: decoder only) the aux stream may start here, beside the decoder; else only after the last draw (end of the forward)
        early_aux = "inner" not in parts and "gmm" not in parts
        if early_aux:
            self._mark_for_aux()
        self.xhat = None
        if "dec" in parts:
            xhat = self.decoder.forward(z)
            nb = L.query("ladder_pixel_partials_workspace_bytes", x.numel())
            wsp, wsn = ctx.ws(nb)
            L.call("ladder_pixel_partials", _p(x), _p(xhat), x.numel(), _p(P[L.P_PIX_ABS:]), wsp, wsn, st)
            self.xhat = xhat
        if self.gmm_z and "gmm" in parts:
            self.gmm_grads = self._mixture_term(mu, sd, noise, B, need_grad="gmm_grad" in parts)
        vamp_on = self.vamp and "gmm" in parts and not use_sg
        if vamp_on:
            self.gmm_grads = self._vamp_term(mu, sd, noise, B)
        inner_on = self.has_inner and "inner" in parts
        if inner_on:
            mu_t, sdraw_t = self.inner.encode(z)
            eps_t = self._noise(noise, "eps_t", (B, R))
            t, sd_t = ctx.empty(B, R), ctx.empty(B, R)
            L.call("ladder_latent_fwd", _p(mu_t), _p(sdraw_t), _p(eps_t), self.lvp, _p(t), _p(sd_t), _p(P[L.P_LOG_SDT:]),
                   _p(P[L.P_MU2SD2_T:]), _p(P[L.P_FIXED + Z:]), B, R, st)
            zhat = self.inner.decode(t)
            L.call("ladder_code_partials", _p(z), _p(zhat), _p(sd), int(use_mask), _p(P[L.P_CODE_ERR:]), B, Z, st)
            self.lat_t = (mu_t, sd_t, sdraw_t, eps_t, t)
            self.zhat = zhat
            self.gmm_grads = None
            if "gmm" in parts and not self.hier:
                self.gmm_grads = self._mixture_term(mu_t, sd_t, noise, B)
        ctx.comm.allreduce_(P, "C3 partials")                    # C3: scalar partials of the GLOBAL batch
        ecfg = L.LadderElboCfg(self.Bg, self.D, Z, R, self.Lmc,
                               1 if (self.cfg["exp_name"] == "celeba" or int(self.cfg["TRAIN_sigma"]) == 1) else 0,
                               1 if inner_on else 0, 1 if use_sg else 0,
                               1 if (self.has_inner and int(self.cfg["TRAIN_inner_sigma"]) == 1) else 0,
                               float(self.cfg.get("inner_sigma_lb", 0.0)), float(self.cfg.get("inner_sigma_ub", 0.0)),
                               1 if self.hier else 0, 1 if (self.gmm_z or vamp_on) else 0)
        # A run without the decoder (RUN#3 / RUN#4, the t-sample passes of the mixture fit) has no pixel term: its sigma-dependent scalars
        # (sigma, reconstruction likelihood, elbo, loss_ae) are not part of what the reference fetches from it (base.py:615-639).  They are
        # evaluated against a CONSTANT 1 instead of sigma/Variable, which RUN#2's optimiser step may be writing on the main stream while
        # these runs execute on the aux stream (cross-stream race; the values were timing-dependent).  inner_sigma/Variable is
        # only read by runs that evaluate the inner VAE, all of which are ordered with its writer (RUN#4, same stream / joined).
        sig = self.ps.w["sigma/Variable"] if "dec" in parts else self._sigma_one
        # (the decoder-dependent scalars of such a run are computed against that stand-in and mean nothing: fetch() reports them as NaN)
        self._undefined = () if "dec" in parts else DEC_SCALARS
        L.call("ladder_elbo_finalize", _p(P), _p(sig),
               _p(self.ps.w["inner_sigma/Variable"]) if self.has_inner else None, ecfg, _p(self.scalars), st)
        if not early_aux:
            self._mark_for_aux()
        if self._run_calls:
            L.call("ladder_u64_add", _p(self.rng_counter), self._run_calls, st)      # advance the device noise stream (atomic add)
        if self._on_aux:
            self._aux_calls += self._run_calls
        else:
            self._main_calls = self._run_calls
        self.use_sg, self.use_mask = use_sg, use_mask

    def _mark_for_aux(self):
        """Main-stream forward: snapshot of the noise position (before this run's advance) + the event an aux run waits for."""
        if self._aux_on and not self._on_aux and not torch.cuda.is_current_stream_capturing():
            self.rng_counter_aux.copy_(self.rng_counter, non_blocking=True)
            self._enc_event = torch.cuda.Event()
            self._enc_event.record(torch.cuda.current_stream(self.ctx.device))

    def _mixture_term(self, mu, sd, noise, B, need_grad=True):
        """MC estimate of E_q[log p_GM] over L samples of N(mu, sd^2) (base.py:308-313 on t, 322-329 on z): writes the sum of
        the log-probs into the partials and returns (sum_l dlogp/dt, sum_l dlogp/dt * eps) for the latent backward."""
        if self.mixture is None:
            raise L.LadderHipError("set_mixture()/set_sg_mixture() must be called before a run that evaluates the GM prior")
        eps_mc = self._noise(noise, "eps_mc", (self.Lmc, B, self.R))
        return self.mixture.fwd_bwd(mu, sd, eps_mc, self.partials[L.P_LOGP:], need_grad)

    def _vamp_components(self):
        """The K diagonal components of the VampPrior as they are NOW: encoder pass over the pseudo-inputs, then the latent head with
        zero noise -> (means, std devs, raw std-dev head output, the zero noise), each [K, Z]."""
        ctx, Z, K = self.ctx, self.Z, self.K
        mu_p, sdraw_p = self.encoder_p.forward(self.ps.w["prior/Variable"])
        eps0, sd_p, scratch = ctx.zeros(K, Z), ctx.empty(K, Z), ctx.zeros(4)
        L.call("ladder_latent_fwd", _p(mu_p), _p(sdraw_p), _p(eps0), self.lvp, None, _p(sd_p), _p(scratch), _p(scratch[1:]), None, K, Z, ctx.stream)
        return mu_p, sd_p, sdraw_p, eps0

    def _vamp_term(self, mu, sd, noise, B):
        """crossEntropy_prior of the VampPrior (base.py:361-370): the components at the pseudo-inputs, then the MC mixture term and its
        gradients towards both the posterior heads and the components."""
        mu_p, sd_p, sdraw_p, eps0 = self._vamp_components()
        eps_mc = self._noise(noise, "eps_mc", (self.Lmc, B, self.Z))
        dmu, dsd, dcm, dcs = self.vamp_mixture.fwd_bwd(mu, sd, eps_mc, mu_p, sd_p, self.partials[L.P_LOGP:])
        self.vamp_state = (mu_p, sd_p, sdraw_p, eps0, dcm, dcs)
        return dmu, dsd

    def _vamp_backward(self, wgrad, need_input_dx):
        """Backward of the pseudo-input pass: d loss/d components = -(1/LB) * (dcomp_mean, dcomp_sd) through the heads."""
        ctx, st, Z, K = self.ctx, self.ctx.stream, self.Z, self.K
        mu_p, sd_p, sdraw_p, eps0, dcm, dcs = self.vamp_state
        dmu_h, dsdraw_h = ctx.empty(K, Z), ctx.empty(K, Z)
        L.call("ladder_latent_bwd", None, _p(mu_p), _p(sd_p), _p(sdraw_p), _p(eps0), _p(dcm), _p(dcs), -1.0, _p(self.scalars), 0,
               _p(dmu_h), _p(dsdraw_h), K, Z, st)
        return self.encoder_p.backward(dmu_h, dsdraw_h, wgrad=wgrad, need_input_dx=need_input_dx)

    @staticmethod
    def _enc_needs_grad(parts):
        return False          # only run_ae back-propagates into the encoder, and it never asks for reuse

    def fetch(self, names=None):
        """Host copy of the fetched scalars (ONE device->host sync)."""
        self._join_aux()
        src = self._fetch_src[0] if self._fetch_src is not None else self.scalars
        s = src.detach().cpu().numpy()
        und = getattr(self, "_undefined", ())
        # (default list: the scalars the last run DEFINES -- a decoder-less run has no sigma / reconstruction / elbo; asked for by name they are NaN)
        names = names or [n for n in L.S_NAMES if not n.startswith("_") and n not in und]
        return {n: (float("nan") if n in und else float(s[L.S_INDEX[n]])) for n in names}

    def fetch_async(self, names=None):
        """fetch() without stalling the host: the scalars are copied into pinned host memory behind the kernels enqueued so far and an
        event marks the copy; `.get()` on the returned handle waits for THAT event only.  A caller that enqueues the next run before it
        reads the values keeps the GPU busy across the read (a synchronous fetch after every run left ~0.35 ms of bubbles per CelebA
        iteration: the device drains, then waits for the host to enqueue the next run's first kernels)."""
        pool = self.__dict__.setdefault("_pinned_pool", [])
        host = pool.pop() if pool else torch.empty(L.S_COUNT, dtype=torch.float32, pin_memory=True)
        src, stream = self._fetch_src if self._fetch_src is not None else (self.scalars, torch.cuda.current_stream(self.ctx.device))
        with torch.cuda.stream(stream):                  # (the stream the run was enqueued on: its scalars buffer, its order)
            host.copy_(src, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
        und = getattr(self, "_undefined", ())
        return _AsyncFetch(host, ev, names or [n for n in L.S_NAMES if not n.startswith("_") and n not in und], pool, und)

    def std_dev_code(self):
        return (self.partials[L.P_FIXED:L.P_FIXED + self.Z] / self.Bg).cpu().numpy()

    def std_dev_representation(self):
        return (self.partials[L.P_FIXED + self.Z:L.P_FIXED + self.Z + self.R] / self.Bg).cpu().numpy()

    # -- backward pieces ------------------------------------------------------------------------
    def _sc(self, name):
        return self.scalars[L.S_INDEX[name]:]

    def _backward_ae(self):
        ctx, st, B, Z, R = self.ctx, self.ctx.stream, self.B, self.Z, self.R
        mu, sd, sd_raw, eps_z, z = self.lat_z
        vamp_on = self.vamp and not self.use_sg
        saved_enc = None
        if vamp_on:
            # the encoder weights receive two gradient contributions (data pass + pseudo-input pass); the filter-gradient kernels
            # overwrite, so the pseudo-pass result is parked and added back after the data pass
            self._vamp_backward(wgrad=True, need_input_dx=False)
            ctx.join_side()
            lo, hi = self._enc_range
            saved_enc = self.ps.grad["ae"][lo:hi].clone()
        dxhat = torch.empty_like(self.xhat)
        L.call("ladder_pixel_grad", _p(self.x), _p(self.xhat), _p(self._sc("_g_pix")), _p(dxhat), dxhat.numel(), st)
        dz = self.decoder.backward(dxhat)
        self._c1_pending = None
        if ctx.comm.on and self._dec_range is not None:
            # C1, first bucket: every decoder gradient is final here (~3/4 of the 72 MB); its all-reduce runs over xGMI
            # while the inner-VAE and encoder backward kernels keep the CUs busy.  The rest follows in _ae.
            lo, hi = self._dec_range
            ctx.join_side()                                       # the decoder's filter gradients are final only after the side stream
            self._c1_pending = ctx.comm.allreduce_async_(self.ps.grad["ae"][lo:hi], "C1 bucket 1 (decoder, async)")
        mode = 1
        if self.has_inner and not self.use_sg:
            mu_t, sd_t, sdraw_t, eps_t, t = self.lat_t
            dzhat = ctx.empty(B, Z)
            L.call("ladder_code_grad", _p(z), _p(self.zhat), _p(sd), int(self.use_mask), _p(self.scalars), _p(dz), _p(dzhat), B, Z, st)
            dt = self.inner.decode_backward(dzhat, wgrad=False)
            dmu_t, dsdraw_t = ctx.empty(B, R), ctx.empty(B, R)
            gm_mu, gm_sd = (None, None) if self.hier else self.gmm_grads       # hierarchical: closed-form N(0,I) term (mode bit 1)
            L.call("ladder_latent_bwd", _p(dt), _p(mu_t), _p(sd_t), _p(sdraw_t), _p(eps_t), _p(gm_mu),
                   _p(gm_sd), -1.0, _p(self.scalars), 3 if self.hier else 1, _p(dmu_t), _p(dsdraw_t), B, R, st)
            add_(ctx, dz, self.inner.encode_backward(dmu_t, dsdraw_t, wgrad=False, need_dz=True))
        else:
            mode = 3
        ex_mu, ex_sd = (None, None)
        if self.gmm_z or vamp_on:                             # -crossEntropy_prior = -(1/LB) sum log p(z_l): mixture grads, no SG term
            mode, (ex_mu, ex_sd) = 1, self.gmm_grads
        dmu, dsdraw = ctx.empty(B, Z), ctx.empty(B, Z)
        L.call("ladder_latent_bwd", _p(dz), _p(mu), _p(sd), _p(sd_raw), _p(eps_z), _p(ex_mu), _p(ex_sd), -1.0, _p(self.scalars), mode,
               _p(dmu), _p(dsdraw), B, Z, st)
        self.encoder.backward(dmu, dsdraw)
        ctx.join_side()
        if saved_enc is not None:
            lo, hi = self._enc_range
            add_(ctx, self.ps.grad["ae"][lo:hi], saved_enc)

    def _backward_prior(self):
        ctx, st, B, Z, R = self.ctx, self.ctx.stream, self.B, self.Z, self.R
        mu, sd, sd_raw, eps_z, z = self.lat_z
        mu_t, sd_t, sdraw_t, eps_t, t = self.lat_t
        dzhat = ctx.empty(B, Z)
        L.call("ladder_code_grad", _p(z), _p(self.zhat), _p(sd), int(self.use_mask), _p(self.scalars), None, _p(dzhat), B, Z, st)
        dt = self.inner.decode_backward(dzhat, wgrad=True)
        dmu_t, dsdraw_t = ctx.empty(B, R), ctx.empty(B, R)
        gm_mu, gm_sd = (None, None) if self.hier else self.gmm_grads
        L.call("ladder_latent_bwd", _p(dt), _p(mu_t), _p(sd_t), _p(sdraw_t), _p(eps_t), _p(gm_mu),
               _p(gm_sd), -1.0, _p(self.scalars), 3 if self.hier else 1, _p(dmu_t), _p(dsdraw_t), B, R, st)
        self.inner.encode_backward(dmu_t, dsdraw_t, wgrad=True, need_dz=False)

    # -- the four runs --------------------------------------------------------------------------
    def _ae(self, x, lr, noise, use_sg, use_mask, reuse_encoder=False):
        # in the SG regime the inner VAE does not enter loss_ae's gradient (tf.cond, base.py:318-320) nor its fetches
        parts = ("dec",) if (use_sg or not self.has_inner) else ("dec", "inner", "gmm")
        if self.gmm_z:
            parts = ("dec", "gmm", "gmm_grad")
        if self.vamp:
            parts = ("dec", "gmm")
        self.forward(x, noise, use_sg, use_mask, parts)
        self._backward_ae()
        g = self.ps.grad["ae"]                                    # C1 (sum of per-rank grads of the global-mean loss)
        if getattr(self, "_c1_pending", None) is not None:
            lo, hi = self._dec_range                              # decoder bucket already in flight: reduce what is left
            if lo > 0:
                self.ctx.comm.allreduce_(g[:lo], "C1 bucket 2 (rest)")
            if hi < g.numel():
                self.ctx.comm.allreduce_(g[hi:], "C1 bucket 2 (rest)")
            self._c1_pending.wait()
            self._c1_pending = None
        else:
            self.ctx.comm.allreduce_(g, "C1 (one bucket)")
        self.ps.adam("ae", lr)
        self._repack_filters()

    def _repack_filters(self):
        """Every split filter image the convolutions have asked for so far, re-packed from the just-updated weights in TWO launches
        (ladder_filter_pack_split_multi) instead of memset + absmax + pack per bank on first use (~25 banks on the CelebA nets).  Eager
        mode only: a hipGraph capture keeps the lazy per-bank path (it re-packs inside the graph)."""
        ctx = self.ctx
        banks = ctx.pack_banks
        if not banks or self.use_graphs or torch.cuda.is_current_stream_capturing():
            return
        tab = ctx._pack_table
        if tab is None or tab[0] != len(banks):
            import numpy as np
            dt = np.dtype([("w", "<u8"), ("packed", "<u8"), ("ntaps", "<i4"), ("cin", "<i4"), ("cout", "<i4"), ("flip", "<i4"),
                           ("block_begin", "<i4"), ("reserved", "<i4")])
            rows, blk = np.zeros(len(banks), dtype=dt), 0
            for r, (ent, w, taps, cin, cout, flip, ns, _grp) in zip(rows, banks):
                assert ns == ctx.ns
                r["w"], r["packed"], r["ntaps"], r["cin"], r["cout"], r["flip"], r["block_begin"] = w.data_ptr(), ent[1].data_ptr(), taps, cin, cout, flip, blk
                blk += L.query("ladder_filter_pack_job_blocks", taps, cin, cout)
            dev = torch.from_numpy(rows.view(np.uint8).copy()).to(ctx.device)
            scratch = torch.empty(L.query("ladder_filter_pack_split_multi_scratch_bytes", len(banks)), dtype=torch.uint8, device=ctx.device)
            tab = ctx._pack_table = (len(banks), dev, blk, scratch)
        L.call("ladder_filter_pack_split_multi", _p(tab[1]), tab[0], tab[2], ctx.ns, _p(tab[3]), tab[3].numel(), ctx.stream)
        for ent, *_, grp in banks:
            ent[0] = self.ps.version[grp]

    def _sigma(self, x, lr, noise, use_sg, use_mask, reuse_encoder=False):
        self.forward(x, noise, use_sg, use_mask, ("dec",), reuse_encoder, keep_acts=False)
        self.ps.adam("sigma", lr, grad=self._sc("_g_sigma_var"), n=1)

    def _prior(self, x, lr, noise, use_sg, use_mask, reuse_encoder=False):
        if self.vamp:
            # loss_prior = -elbo w.r.t. the pseudo-inputs (base.py:408-409, 474-481): only the mixture term depends on them; with
            # the standard-Gaussian switch on, the gradient is identically zero (the optimiser still steps, as tf.cond does)
            self.forward(x, noise, use_sg, use_mask, ("dec", "gmm"), reuse_encoder)
            g = self.ps.g["prior/Variable"]
            if use_sg:
                L.call("ladder_axpy", None, _p(g), g.numel(), 0.0, 2, self.ctx.stream)
            else:
                g.copy_(self._vamp_backward(wgrad=False, need_input_dx=True))
            self.ctx.comm.allreduce_(self.ps.grad["prior"], "C4 prior gradients")       # C4
            self.ps.adam("prior", lr)
            return
        self.forward(x, noise, use_sg, use_mask, ("inner", "gmm"), reuse_encoder)
        self._backward_prior()
        self.ctx.comm.allreduce_(self.ps.grad["prior"], "C4 prior gradients")           # C4
        self.ps.adam("prior", lr)

    def _inner_sigma(self, x, lr, noise, use_sg, use_mask, reuse_encoder=False):
        self.forward(x, noise, use_sg, use_mask, ("inner",), reuse_encoder)
        self.ps.adam("inner_sigma", lr, grad=self._sc("_g_inner_sigma_var"), n=1)

    _GROUP = {"ae": "ae", "sigma": "sigma", "prior": "prior", "inner_sigma": "inner_sigma"}
    _SNAP = ("x", "B", "Bg", "lat_z", "lat_t", "xhat", "zhat", "gmm_grads", "vamp_state", "use_sg", "use_mask")

    def _run(self, kind, x, lr, noise, use_sg, use_mask, reuse_encoder):
        """Eager, or -- with `use_graphs` -- one captured hipGraph per (run kind, regime, batch shape): after two eager
        warm-up calls the run's ~10^2..10^3 launches are replayed as a single graph launch.  Every per-step scalar (Adam step /
        lr_t, noise stream position) lives in device memory, so a replay is exactly the eager run."""
        fn = getattr(self, "_" + kind)
        # (also on a graph REPLAY, which does not pass through forward(): RUN#3 / RUN#4 evaluate no decoder -> their sigma-dependent scalars are NaN)
        self._undefined = DEC_SCALARS if (kind in ("prior", "inner_sigma") and not self.vamp) else ()
        if not self.use_graphs or noise is not None or self.ctx.comm.on:
            cache = getattr(self, "_enc_cache", None)
            if (self._aux_on and not self.use_graphs and kind in ("prior", "inner_sigma") and reuse_encoder and not self.vamp
                    and self._enc_event is not None and cache is not None and cache[0] == self.ps.step["ae"]
                    and cache[4] == self._batch_token(x)):
                return self._run_on_aux(fn, x, lr, noise, use_sg, use_mask)
            self._join_aux()
            self._fetch_src = (self.scalars, torch.cuda.current_stream(self.ctx.device))
            try:
                return fn(x, lr, noise, use_sg, use_mask, reuse_encoder)
            finally:
                self.ctx.join_side()
        self._join_aux()
        self._fetch_src = (self.scalars, torch.cuda.current_stream(self.ctx.device))
        group = self._GROUP[kind]
        tok = self._batch_token(x)
        xin = self._dev(x)
        cache = getattr(self, "_enc_cache", None)
        reuse = bool(reuse_encoder and cache is not None and cache[0] == self.ps.step["ae"] and cache[4] == tok)
        key = (kind, bool(use_sg), bool(use_mask), tuple(xin.shape), cache[2].data_ptr() if reuse else 0, self.mixture.buf.data_ptr()
               if self.mixture is not None else 0, self.ctx.ws_generation)
        ent = self._graphs.get(key)
        if ent is None:
            if self._warm.get(key, 0) < 2:                         # eager warm-up: sizes the workspace and the allocator
                self._warm[key] = self._warm.get(key, 0) + 1
                self._x_token = tok
                return fn(xin, lr, None, use_sg, use_mask, reuse_encoder)
            static_x = cache[1] if reuse else xin.clone()
            self.ps.set_lr(group, lr)
            steps, calls = dict(self.ps.step), self._run_calls
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            self._x_token = tok
            with torch.cuda.graph(graph):                          # records the launches; nothing executes, host counters restored
                fn(static_x, lr, None, use_sg, use_mask, reuse_encoder)
            snap = {k: getattr(self, k, None) for k in self._SNAP}
            enc = None if reuse else self._enc_cache[1:4]
            self.ps.step, self._run_calls = steps, calls
            if self.ctx.ws_generation != key[-1]:                  # the workspace grew while recording: this graph is void
                self._warm[key[:-1] + (self.ctx.ws_generation,)] = 2
                return self._run(kind, x, lr, noise, use_sg, use_mask, reuse_encoder)
            ent = self._graphs[key] = (graph, static_x, snap, enc)
        graph, static_x, snap, enc = ent
        if not reuse and static_x.data_ptr() != xin.data_ptr():
            static_x.copy_(xin)
        self.ps.set_lr(group, lr)
        if enc is not None:
            self._enc_cache = (self.ps.step["ae"],) + tuple(enc) + (tok,)   # as the eager forward does (pre-update step)
        graph.replay()
        self.ps.step[group] += 1
        # the replay changed the group's weights on the device: packed split-filter images stamped with the old version are stale
        # for any EAGER forward that follows (val_step, fit_GMM_VI, decode, Session) -- graphs re-pack inside their own capture
        self.ps.version[group] += 1
        for k, v in snap.items():
            setattr(self, k, v)

    def _run_on_aux(self, fn, x, lr, noise, use_sg, use_mask):
        """One of RUN#3 / RUN#4 on the aux stream (see enable_prior_overlap)."""
        aux = self.ctx.aux
        aux.wait_event(self._enc_event)
        main_bufs = (self.partials, self.scalars)
        self.partials, self.scalars, self._on_aux = self.partials_aux, self.scalars_aux, True
        try:
            with torch.cuda.stream(aux):
                fn(x, lr, noise, use_sg, use_mask, True)
                self._aux_event = torch.cuda.Event()
                self._aux_event.record(aux)
        finally:
            self.partials, self.scalars = main_bufs
            self._on_aux = False
        self._fetch_src = (self.scalars_aux, aux)

    def run_ae(self, x, lr, noise=None, use_sg=True, use_mask=False):
        self._run("ae", x, lr, noise, use_sg, use_mask, False)

    def run_sigma(self, x, lr, noise=None, use_sg=True, use_mask=False, reuse_encoder=False):
        self._run("sigma", x, lr, noise, use_sg, use_mask, reuse_encoder)

    def run_prior(self, x, lr, noise=None, use_sg=True, use_mask=False, reuse_encoder=False):
        self._run("prior", x, lr, noise, use_sg, use_mask, reuse_encoder)

    def run_inner_sigma(self, x, lr, noise=None, use_sg=True, use_mask=False, reuse_encoder=False):
        self._run("inner_sigma", x, lr, noise, use_sg, use_mask, reuse_encoder)

    def evaluate(self, x, noise=None, use_sg=True, use_mask=False):
        parts = ("dec", "inner", "gmm") if (((self.has_inner or self.gmm_z) and self.mixture is not None) or self.vamp) else ("dec", "inner")
        self.forward(x, noise, use_sg, use_mask, parts, keep_acts=False)

    # -- generation -----------------------------------------------------------------------------
    def decode(self, code):
        """decoded given code_input (is_code_input=True; models.py:107,265,500)."""
        self._join_aux()
        self.ctx.keep_activations = False
        try:
            return self.decoder.forward(self._dev(code))
        finally:
            self.ctx.keep_activations = True

    def decode_representation(self, t):
        """decoded_code given representation_input (base.py:171-186)."""
        self._join_aux()
        return self.inner.decode(self._dev(t))

    def prior_sampler(self, method=None, mixture=None, seed=0):
        """Device sampler of the prior `method` (default: the configured one) for generation (reference codes/base.py:1065-1122):
        "standard_gaussian" N(0, I_Z) on z; "hierarchical" N(0, I_R) on t; "GMM" / "ours" the full-covariance mixture `mixture` =
        (weights, means, covs) on z / on t; "vampPrior" the K equally weighted diagonal components the encoder gives at the pseudo-inputs
        NOW (base.py:241-254; a later optimiser step needs a new sampler).  Raises ValueError for a mixture that cannot be sampled."""
        method = method or self.cfg["prior"]
        if method not in PRIOR_METHODS:
            raise ValueError("unknown prior %r: expected one of %s" % (method, list(PRIOR_METHODS)))
        if method in ("ours", "hierarchical") and self.inner is None:
            raise ValueError("method %r needs the inner VAE; this model's prior is %r" % (method, self.cfg["prior"]))
        self._join_aux()
        ctx, st = self.ctx, self.ctx.stream
        full = method in ("GMM", "ours")                         # (weights, means, covs); else K diagonal components (means, scales)
        if full:
            if mixture is None:
                raise ValueError("method %r samples a fitted mixture: pass mixture=(weights, means, covs)" % method)
            w, m, c = (self._dev(a) for a in mixture)
            K, R = int(w.numel()), int(self.Z if method == "GMM" else self.cfg["representation_size"])
            if tuple(m.shape) != (K, R) or tuple(c.shape) != (K, R, R):
                raise ValueError("mixture shapes %s %s %s do not fit K = %d, R = %d" % (tuple(w.shape), tuple(m.shape), tuple(c.shape), K, R))
            keep = (w, m, c)
        elif method == "vampPrior":
            if not self.vamp:
                raise ValueError("method 'vampPrior' needs the pseudo-inputs; this model's prior is %r" % self.cfg["prior"])
            K, R = self.K, self.Z
            keep = self._vamp_components()[:2]
        else:
            K, R = 1, int(self.Z if method == "standard_gaussian" else self.cfg["representation_size"])
            keep = (ctx.zeros(1, R), torch.ones(1, R, dtype=torch.float32, device=ctx.device))
        form = family("sampler", K, R)                           # (both families: same buffer, same draws, csrc/sample.hip)
        nbytes = L.query(form.param_bytes, K, R)
        if nbytes == 0:
            raise ValueError("the device sampler takes K >= 1 and 1 <= R <= 64, or 64 < R <= 256 with R %% 16 == 0 (got K = %d, R = %d)" % (K, R))
        params = torch.empty(nbytes, dtype=torch.uint8, device=ctx.device)
        fws, fws_args = sized_workspace(form.prepare_workspace_bytes if full else None, ctx.device, K, R)
        L.call(form.prepare if full else form.prepare_diag, *(_p(a) for a in keep), K, R, _p(params), *fws_args, st)
        check_status_word(params, "%s mixture" % method, "covariance / scale")      # (the read also keeps the temporaries alive until the kernels ran)
        return PriorSampler(self, method, form, K, R, params, seed)

    def images_to_u8(self, x):
        """uint8 device tensor of x's shape: rint(255 * clip(x, 0, 1)), NaN -> 0 (ladder_images_to_u8)."""
        x = x.contiguous()
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
        L.call("ladder_images_to_u8", _p(x), _p(out), x.numel(), self.ctx.stream)
        return out

    def generate(self, n, sampler, chunk=128, as_uint8=False, first=0, sink=None):
        """Images of samples first .. first+n-1 of `sampler` as ONE host array [n, H, W, C] (float32 raw decoder output, or uint8 with
        `as_uint8`): per chunk sample -> decode -> optional byte packing -> asynchronous copy into one of two pinned host buffers on a
        copy stream, so the copy of chunk j runs beside the decode of chunk j+1.
        `sink`: each decoded DEVICE chunk [b, H, W, C] (after the byte packing, if asked for) is handed to sink(chunk, first) on the current stream
        instead, `first` = the sample index of the chunk's first image; nothing is copied to the host and the call returns None (fid.py: the images
        never leave the device)."""
        n, chunk = int(n), int(chunk)
        if n < 0 or chunk < 1:
            raise ValueError("generate: n >= 0 and chunk >= 1 (got %d, %d)" % (n, chunk))
        cfg, ctx = self.cfg, self.ctx
        shape = (int(cfg["dim_input_x"]), int(cfg["dim_input_y"]), int(cfg["dim_input_channel"]))
        dt_t, dt_n = (torch.uint8, np.uint8) if as_uint8 else (torch.float32, np.float32)
        out = None if sink is not None else np.empty((n,) + shape, dtype=dt_n)
        if n == 0:
            return out
        self._join_aux()
        main = torch.cuda.current_stream(ctx.device)
        nb = min(chunk, n)
        pinned = [torch.empty((nb,) + shape, dtype=dt_t, pin_memory=True) for _ in range(2)] if sink is None else None
        inflight = [None, None]                  # per pinned buffer: (copy-done event, offset, rows, device tensor kept alive)

        def drain(slot):
            if inflight[slot] is not None:
                ev, lo, b, _keep = inflight[slot]
                ev.synchronize()
                out[lo:lo + b] = pinned[slot][:b].numpy()
                inflight[slot] = None

        def to_host(img, j, lo, b):              # the consumer of a chunk when no sink is given
            slot, cs = j & 1, ctx.copy_stream
            ready = torch.cuda.Event()
            ready.record(main)
            drain(slot)                          # (host: the buffer's previous copy has landed and been consumed)
            with torch.cuda.stream(cs):
                cs.wait_event(ready)
                pinned[slot][:b].copy_(img, non_blocking=True)
                done = torch.cuda.Event()
                done.record(cs)
            inflight[slot] = (done, lo, b, img)

        ctx.keep_activations = False
        try:
            for j, lo in enumerate(range(0, n, chunk)):
                b = min(chunk, n - lo)
                code, _, _ = sampler.sample(b, first=int(first) + lo)
                img = self.decoder.forward(code)
                if as_uint8:
                    img = self.images_to_u8(img)
                img = img.reshape((b,) + shape)
                if sink is not None:
                    sink(img, int(first) + lo)
                else:
                    to_host(img, j, lo, b)
            drain(0)
            drain(1)
        finally:
            ctx.keep_activations = True
            for e in inflight:                   # an exception mid-way: nothing may outlive its copy
                if e is not None:
                    e[0].synchronize()
        return out

    def sample_code(self, x, noise=None):
        """code_sample for fit_GMM_VI(space="z") (base.py:699-710): encoder -> z."""
        self.forward(x, noise, True, False, ())
        return self.lat_z[4]

    def sample_representation(self, x, noise=None):
        """representation_sample for fit_GMM_VI (base.py:683-698): encoder -> z -> inner encoder -> t."""
        self.forward(x, noise, True, False, ("inner",))
        return self.lat_t[4]
