"""Device context, parameter store and the layers with explicit backward passes of the HIP LaDDer path.  PyTorch supplies device memory, streams and
torch.distributed only; every arithmetic op below is a call into libladder_hip.so (see _lib.py) -- there is no CPU path."""
import functools
import os
from collections import namedtuple

import numpy as np
import torch

from . import _lib as L
from . import arch
from .comm import Comm, _NoComm

BN_EPS = 1e-3      # tf.layers.batch_normalization default
IN_EPS = 1e-6      # tf.contrib.layers.instance_norm default
ADAM_B1, ADAM_B2, ADAM_EPS = 0.9, 0.95, 1e-8   # codes/base.py:459-461


def _p(t):
    return None if t is None else t.data_ptr()


# config key `matmul_precision`: how the large 3x3 convolutions are contracted (csrc/convsplit.hip; values = LADDER_PREC_*).
#   "f32"     v_mfma_f32_32x32x2_f32: bit-exact fp32 FMA chains at the fp32 vector rate
#   "f16x3"   fp32 operands scaled by a power of two (from the absolute maximum of their sample, or tensor) and split into 2 fp16 planes (22 bits),
#             3 plane products on the fp16 matrix cores, fp32 accumulate: fp32-class error (measured: below the f32 FMA chain's)
#   "bf16x6"  3 bf16 planes (24 bits), 6 plane products, no scaling: fp32-class error
#   "bf16x3"  2 bf16 planes (16 bits), 3 products (error ~1e-5 relative per product: between TF32 and fp32)
PRECISIONS = {"f32": 0, "bf16x3": 2, "bf16x6": 3, "f16x3": 4}
DEFAULT_PRECISION = "f32"       # the reference computes in fp32 end to end (codes/models.py:348,388): split formats are an explicit opt-in

PRECISION_NOTES = {
    "f32": "native fp32 MFMA (v_mfma_f32_32x32x2_f32), bit-exact fp32 FMA chains",
    "f16x3": "fp32-class EMULATION: fp32 operands as 2 scaled fp16 planes (22 significand bits, power-of-two scales per sample / "
             "per tensor, see DESIGN 4a), 3 fp16 MFMAs per product, fp32 accumulation; set \"matmul_precision\": \"f32\" for strict fp32",
    "bf16x6": "fp32-class EMULATION: 3 bf16 planes (24 bits), 6 bf16 MFMAs per product, fp32 accumulation",
    "bf16x3": "REDUCED precision: 2 bf16 planes (16 bits), 3 bf16 MFMAs per product (between TF32 and fp32)"}

PROF = None   # set to a KernelProfiler by bench.py


def _igemm_plan(M, Cin, Cout, Kdim, conv=None):
    """(split-K workspace bytes -- None: the call is handed a null workspace --, profiler kernel id) of a forward-type implicit-GEMM call (conv fwd /
    bwd_data with the 13 geometry arguments `conv` of ladder_conv2d_fwd_kernel_id, dense fwd / bwd_data without)."""
    nb = L.query("ladder_igemm_fwd_workspace_bytes", M, Kdim, Cout)
    kid = L.query("ladder_conv2d_fwd_kernel_id", *conv) if conv else L.query("ladder_igemm_fwd_tile", M, Cin, Cout)
    if kid != 256128 and nb and L.query("ladder_igemm_fwd_splits", M, Kdim, Cout) > 1:
        kid = 0         # split-K launch: two kernels, not attributed
    return nb or None, kid if kid in (256128, 128128) else 0


def _timed(kid, flops, name, args, executed=None):
    """One launch, bracketed by HIP events on the launch stream and attributed to kernel `kid` when a profiler is installed (bench.py's roofline
    leg; kid 0: a launch the profiler does not attribute)."""
    if PROF is None or not kid:
        L.call(name, *args)
        return
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    L.call(name, *args)
    e.record()
    PROF.add(kid, s, e, flops, executed)


def _gather_executed(kid, flops, geo, bwd_data):
    """The FLOPs a gather-kernel launch issues when its tiles skip the padding taps of a small map (ladder_igemm_fwd_live_chunks over the twelve
    geometry arguments `geo`), for `_timed`'s `executed`; None when nothing is skipped, another kernel runs the call or no profiler is installed."""
    if PROF is None or not kid:
        return None
    live = L.query("ladder_igemm_fwd_live_chunks", *geo, int(bwd_data), -1)
    full = L.query("ladder_igemm_fwd_live_chunks", *geo, int(bwd_data), 0)
    return flops * live / full if 0 < live < full else None


class PlanesOnly:
    """Stand-in for an activation that exists ONLY as its fp16 plane images (registered with Ctx.set_planes / set_amax): the batch-norm
    apply of an encoder layer whose consumer is a split gather convolution never writes the fp32 tensor.  Any fp32 use raises."""

    def __init__(self, shape):
        self.shape = torch.Size(shape)

    def numel(self):
        n = 1
        for d in self.shape:
            n *= int(d)
        return n

    def data_ptr(self):
        raise RuntimeError("this activation exists only as fp16 planes (PlanesOnly): an fp32 kernel was routed to it")


class Ctx:
    """Device context shared by all layers: stream handle, grow-only workspace, communicator."""

    def __init__(self, device, comm=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise L.LadderHipError("the LaDDer HIP path needs a GPU device (got %s); there is no CPU fallback" % device)
        L.load()
        self.comm = comm or Comm()
        self._ws = torch.empty(1 << 20, dtype=torch.uint8, device=self.device)
        self._ws_retired, self.ws_generation = [], 0
        self._amax = {}      # id(tensor) -> (weakref, absolute-maximum record)
        self._planes = {}    # id(tensor) -> (weakref, pre-split planes)
        self.pack_banks, self._pack_table = [], None              # split filter images known so far; their device job table
        # second HIP stream for the filter gradients (MFMA-bound, needed only by the optimiser step): they run beside the backward-data /
        # resize / norm backward kernels of the layers below, which are HBM-bound and fit on the same CUs (Conv2D.backward, join_side)
        self.side, self._side_active, self._side_refs = None, False, []
        self._ws_side = torch.empty(1 << 20, dtype=torch.uint8, device=self.device)
        self._ws_side_retired = []
        self.aux = None      # third HIP stream: RUN#3 / RUN#4 beside RUN#2's decoder forward (LadderEngine.enable_prior_overlap)
        self._ws_aux = None
        self.keep_activations = True   # False inside forward-only runs: fused kernels may skip writing tensors only a backward pass reads
        self.ns = 0          # LADDER_PREC_* of the split-precision contraction kernels (0 = native f32 MFMA); set by the engine
        self.up2_used = {}   # layer name -> number of upsample-fused launches so far (bench.py's executed-FLOP model)
        self.up2_skipped = {}  # ... and the fraction of the reference's products such a launch never issues (11 / 36 tap-folded, 27 / 36 projected)
        self.fuse_bwd_proj = 1   # last pair: backward combination straight from the 1x1 output conv's gradient (config `fused_projection_backward`)
        self.fuse_fwd = 2    # projected pairs: forward GEMM + combination in one launch (config `fused_projected_forward`: 2 wherever eligible (default), 1 only where the isolated launch measured faster, 0 off)
        self.up2 = True      # resize -> 3x3 conv pairs of the decoder as ONE upsample-fused convolution in forward-only runs (config `upsample_fused_convs`)

    @property
    def sfx(self):
        """Suffix of the batch-sized dense entry points for the configured precision ("_f32": strict fp32 MFMA; "": bf16x6)."""
        return "" if self.ns else "_f32"

    @property
    def stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream

    def fork_side(self, *keep):
        """Context manager: what is launched inside runs on the side stream, ordered after everything enqueued on the main stream so
        far.  `keep`: tensors the side stream reads -- referenced until join_side() so that the caching allocator (which only knows the
        main stream) does not hand their memory out again."""
        ev = torch.cuda.Event()
        ev.record()
        self.side.wait_event(ev)
        self._side_refs.extend(k for k in keep if k is not None)
        self._side_active = True
        return torch.cuda.stream(self.side)

    def side_or_main(self, *keep):
        """fork_side() when the side stream is enabled (eager mode, not inside a hipGraph capture), else a no-op context."""
        if self.side is None or torch.cuda.is_current_stream_capturing():
            import contextlib
            return contextlib.nullcontext()
        return self.fork_side(*keep)

    def join_side(self):
        """The main stream waits for the side stream (before anything reads the filter gradients)."""
        if self._side_active:
            torch.cuda.current_stream(self.device).wait_stream(self.side)
            self._side_active = False
            self._side_refs.clear()
            self._ws_side_retired.clear()

    def ws(self, nbytes):
        if nbytes is None:       # (a launch that is handed no workspace)
            return None, 0
        if self.aux is not None and torch.cuda.current_stream(self.device) == self.aux:        # ... and so has the prior-run stream
            if self._ws_aux is None or self._ws_aux.numel() < nbytes:
                # (stream-ordered: the old buffer belongs to this stream's allocator pool, kernels already enqueued on it run first)
                self._ws_aux = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=self.device)
            return self._ws_aux.data_ptr(), self._ws_aux.numel()
        if self.side is not None and torch.cuda.current_stream(self.device) == self.side:      # the side stream has its own scratch
            if self._ws_side.numel() < nbytes:
                self._ws_side_retired.append(self._ws_side)
                self._ws_side = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=self.device)
            return self._ws_side.data_ptr(), self._ws_side.numel()
        if self._ws.numel() < nbytes:
            # a captured hipGraph has the pointer of the workspace it was recorded with baked in: superseded buffers stay alive (the
            # caching allocator must never hand their memory to a live tensor) and every graph recorded so far is dropped, so the
            # next call of a run re-captures against the new buffer
            self._ws_retired.append(self._ws)
            self._ws = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=self.device)
            self.ws_generation += 1
        return self._ws.data_ptr(), self._ws.numel()

    def empty(self, *shape):
        return torch.empty(*shape, dtype=torch.float32, device=self.device)

    # -- absolute-maximum records of the f16x3 split kernels (include/ladder_hip.h: ladder_absmax) --------------------------------
    # Producers that can compute max|y| while they write y (split conv epilogue, instance-norm apply, ...) register the record
    # for the tensor object; consumers look it up and fall back to a standalone pass over the tensor.  Entries are keyed by the
    # tensor OBJECT (dropped when it is collected), never by address: a view / reshape is a different object and simply misses.
    def new_amax(self):
        return torch.empty(L.ABSMAX_FLOATS, dtype=torch.float32, device=self.device)

    def set_amax(self, t, rec):
        if self.ns == 4 and rec is not None:
            import weakref
            k, reg = id(t), self._amax
            reg[k] = (weakref.ref(t, lambda _r, k=k, reg=reg: reg.pop(k, None)), rec)

    def known_amax(self, t):
        e = self._amax.get(id(t))
        return e[1] if e is not None and e[0]() is t else None

    def drop_amax(self, t):
        self._amax.pop(id(t), None)
        self._planes.pop(id(t), None)

    def absmax(self, t):
        """Absolute-maximum record of `t` (an upper bound is as good: it only moves the 2^-38 representation floor); None when
        the precision mode needs none.  A standalone pass writes a PER-SAMPLE record for [N, ...] tensors (include/ladder_hip.h)."""
        if self.ns != 4:
            return None
        rec = self.known_amax(t)
        if rec is None:
            rec = self.new_amax()
            per = t.numel() // int(t.shape[0]) if t.dim() >= 2 else 0
            if per and per % 4 == 0 and int(t.shape[0]) > 1:
                L.call("ladder_absmax_samples", _p(t), int(t.shape[0]), per, _p(rec), self.stream)
            else:
                L.call("ladder_absmax", _p(t), t.numel(), _p(rec), self.stream)
            self.set_amax(t, rec)
        return rec

    def set_planes(self, t, buf):
        """Registers plane images a producer wrote for `t` itself (ladder_bn_fwd_apply_planes)."""
        import weakref
        k, reg = id(t), self._planes
        reg[k] = (weakref.ref(t, lambda _r, k=k, reg=reg: reg.pop(k, None)), buf)

    def planes(self, t, per_sample=False):
        """Pre-split 16-bit planes of `t` (ladder_presplit) for the gather kernels, cached per tensor object like the absmax records:
        a layer input is split once and serves the forward call and the filter gradient, an output gradient the backward-data call
        and the filter gradient.  `per_sample`: scale every sample by its own maximum (when the record carries per-sample bounds; the
        planes' header tells the consumer) -- the caller asks for it only where the filter-gradient kernel can follow (a sample's output
        pixels a multiple of its 32-pixel chunks)."""
        e = self._planes.get(id(t))
        if e is not None and e[0]() is t:
            return e[1]
        import weakref
        buf = torch.empty(L.query("ladder_presplit_bytes", t.numel(), self.ns), dtype=torch.uint8, device=self.device)
        ns = int(t.shape[0]) if (per_sample and t.dim() == 4 and (t.numel() // int(t.shape[0])) % 8 == 0) else 0
        L.call("ladder_presplit", _p(t), _p(self.absmax(t)), _p(buf), t.numel(), ns, self.ns, self.stream)
        k, reg = id(t), self._planes
        reg[k] = (weakref.ref(t, lambda _r, k=k, reg=reg: reg.pop(k, None)), buf)
        return buf

    def zeros(self, *shape):
        return torch.zeros(*shape, dtype=torch.float32, device=self.device)

    def fork(self, precision=None, forward_only=False):
        """A fresh context on the same device and communicator for a network that is not the model's (fid.VGG16Features): its own workspace, records,
        packed-bank list and streams; only the copy stream is shared with this one.  `precision`: a LADDER_PREC_* value (default: this context's);
        `forward_only`: nothing is ever kept for a backward pass."""
        c = Ctx(self.device, self.comm)
        c.ns = self.ns if precision is None else int(precision)
        c.keep_activations = not forward_only
        c._copy_root = getattr(self, "_copy_root", self)
        return c

    @property
    def copy_stream(self):
        """The one stream for host <-> device copies that run beside compute (LadderEngine.generate, fid._device_chunks), created on first use and shared
        by every context forked from this one."""
        root = getattr(self, "_copy_root", self)
        if getattr(root, "_copy_stream", None) is None:
            root._copy_stream = torch.cuda.Stream(device=root.device)
        return root._copy_stream

    def local(self):
        """The same device context without cross-rank exchange (batch statistics of a replicated batch stay local)."""
        import copy
        c = copy.copy(self)
        c.comm = _NoComm()
        return c


class ParamStore:
    """Flat fp32 buffers per optimiser group (theta, grad, m, v) with named views.

    One flat gradient buffer per group = one all-reduce (C1/C4) and one clip+Adam launch (N11)."""

    ALIGN = 64  # elements (256 B): keeps every view 16-byte aligned for float4 loads

    def __init__(self, cfg, ctx, values=None, seed=1):
        self.cfg, self.ctx = cfg, ctx
        self.specs = arch.param_specs(cfg)
        values = values if values is not None else arch.init_values(cfg, seed)
        self.offsets, sizes = {}, {}
        for name, shp in self.specs.items():
            g = arch.group_of(name)
            off = sizes.get(g, 0)
            n = int(np.prod(shp)) if len(shp) else 1
            self.offsets[name] = (g, off, n)
            sizes[g] = off + (n + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.theta = {g: ctx.zeros(n) for g, n in sizes.items()}
        self.grad = {g: ctx.zeros(n) for g, n in sizes.items()}
        self.m = {g: ctx.zeros(n) for g, n in sizes.items()}
        self.v = {g: ctx.zeros(n) for g, n in sizes.items()}
        self.step = {g: 0 for g in sizes}                       # host mirror of the per-optimiser step counters
        self.version = {g: 0 for g in sizes}                    # bumped whenever a group's values change (packed-filter caches)
        # device-resident optimiser state {lr, lr_t, step}: a captured hipGraph replays the step without host scalars
        self.adam_state = {g: ctx.zeros(4) for g in sizes}
        self._lr_host = {g: None for g in sizes}
        self.w, self.g = {}, {}
        for name, shp in self.specs.items():
            g, off, n = self.offsets[name]
            self.w[name] = self.theta[g][off:off + n].view(*shp) if len(shp) else self.theta[g][off:off + 1]
            self.g[name] = self.grad[g][off:off + n].view(*shp) if len(shp) else self.grad[g][off:off + 1]
        self.load_dict(values)

    def prefix_range(self, group, prefix):
        """[lo, hi) of the flat `group` buffers covered by the variables whose name starts with `prefix`, or None if they are
        not one contiguous run (param_specs orders names, so each scope is contiguous)."""
        runs = [(off, off + (n + self.ALIGN - 1) // self.ALIGN * self.ALIGN, name.startswith(prefix))
                for name, (g, off, n) in self.offsets.items() if g == group]
        runs.sort()
        inside = [r for r in runs if r[2]]
        if not inside:
            return None
        lo, hi = inside[0][0], inside[-1][1]
        if any(lo <= r[0] < hi and not r[2] for r in runs):
            return None
        return lo, hi

    def load_dict(self, values, strict=True):
        getattr(self, "before_read", lambda: None)()
        for name in self.specs:
            if name not in values:
                if strict:
                    raise KeyError("missing variable %s" % name)
                continue
            v = torch.as_tensor(np.asarray(values[name], np.float32).reshape(self.w[name].shape))
            self.w[name].copy_(v.to(self.ctx.device))
            self.version[arch.group_of(name)] += 1

    def to_dict(self, groups=None):
        getattr(self, "before_read", lambda: None)()           # (the engine: wait for runs in flight on the aux stream)
        return {n: self.w[n].detach().cpu().numpy().reshape(self.specs[n]) for n in self.specs
                if groups is None or arch.group_of(n) in groups}

    def num_params(self, prefix):
        return sum(self.offsets[n][2] for n in self.specs if n.startswith(prefix))

    def set_lr(self, group, lr):
        """Write the learning rate into the device state (only when it changed; never inside a graph capture)."""
        if self._lr_host[group] != lr:
            L.call("ladder_axpy", None, _p(self.adam_state[group]), 1, float(lr), 2, self.ctx.stream)       # (fill: no torch elementwise launch on the path)
            self._lr_host[group] = lr

    def adam(self, group, lr, grad=None, n=None):
        """clip to [-1,1] + TF-form Adam on the whole group (codes/base.py:459-517); lr_t = lr*sqrt(1-b2^t)/(1-b1^t) is
        evaluated on the device from the device step counter.  `grad` may be a device pointer into the scalars vector
        (n = 1) for the two scalar optimisers."""
        self.ctx.join_side()                                    # filter gradients computed on the side stream
        self.set_lr(group, lr)
        self.step[group] += 1
        self.version[group] += 1
        g = self.grad[group] if grad is None else grad
        L.call("ladder_adam_clip_dev", _p(self.theta[group]), _p(g), _p(self.m[group]), _p(self.v[group]),
               self.theta[group].numel() if n is None else n, _p(self.adam_state[group]), ADAM_B1, ADAM_B2, ADAM_EPS, 1.0,
               self.ctx.stream)


# ------------------------------------------------------------------------------------------ layers
# environment switches of this module: name -> (default, meaning).  The first three are read at every use (tests flip them between engines of one
# process), the others once, at import.
SWITCHES = {
    "LADDER_DISABLE_HALO": ("0", "1: strict fp32 runs on the round-1 generic gather kernels everywhere, no halo kernels and no projected pairs (test switch)"),
    "LADDER_DISABLE_BNSTATS": (None, "set (to anything): no convolution epilogue emits batch-norm statistics, they come from the separate pass (test switch; "
                                     "the library reads it itself at every workspace query -- here it is part of Conv2D.route's cache key)"),
    "LADDER_ENABLE_LOWRES_GATE": ("0", "1: the low-resolution backward-data of a resize -> conv pair also applies the activation backward of the layer below"),
    "LADDER_PROJ_MAX_BYTES": (str(32 << 30), "largest Z / D temporary of a projected pair (conv2d_7 at batch 128: 2.4 GB)"),
    "LADDER_UP2T_MIN_PIXELS": ("256", "smallest low-resolution map whose backward-data runs upsample-fused"),
    "LADDER_UP2W_MIN_PIXELS": ("256", "... and whose filter gradient does (8x8: 758 us fused against 612 direct)")}


def switch(name):
    """Value of an environment switch of SWITCHES (the only place of this module that reads the environment)."""
    return os.environ.get(name, SWITCHES[name][0])


def halo_disabled():
    return switch("LADDER_DISABLE_HALO") == "1"


UP2T_MIN_PIXELS = int(switch("LADDER_UP2T_MIN_PIXELS"))
PROJ_MAX_BYTES = int(switch("LADDER_PROJ_MAX_BYTES"))
UP2W_MIN_PIXELS = int(switch("LADDER_UP2W_MIN_PIXELS"))

# what a Conv2D forward kept for its backward pass:
#   form    "plain" (the convolution over x) | "tapfold" (resize -> conv as four parity classes with effective taps, 25 of 36 products) |
#           "projected" (nine 1x1 convolutions on the low-resolution tensor + combination, 9 of 36)
#   x       the kept input operand; x_kind says what it is: "input" (the layer's input itself) | "upsampled" (the materialised resize of the tensor
#           the forward read) | "lowres" (the low-resolution tensor: its upsample by `factor` was never materialised)
#   y       the activated output;  x_amax  the absolute-maximum record of x (f16x3) or None;  route  the ConvRoute of the layer over its input
Kept = namedtuple("Kept", "form x x_kind factor y x_amax route")

# one planned launch:
#   run     the Conv2D method that assembles its arguments and launches it;  fn  the C entry point (include/ladder_hip.h)
#   ws      bytes of workspace it is handed (0: whatever the grow-only workspace holds; None: it takes none, or a null one)
#   kid     profiler kernel id (profiler.KernelProfiler.NAMES; 0: not attributed)
#   bank    orientation of the packed filter bank it reads (BANK_*; None: the HWIO bank itself, or a transpose made on the fly)
Launch = namedtuple("Launch", "run fn ws kid bank", defaults=(None, 0, None))

# how one Conv2D runs over one input shape (Conv2D.route plans it once; forward and backward follow it):
#   N H W Ho Wo pt pl   the geometry: input map, output map, top / left padding;  geo: the twelve geometry arguments of the generic entry points;
#                       flops: operation count of one pass
#   fwd, wgrad          the forward and the filter-gradient launch;  stats: the forward's epilogue also emits the batch-norm statistics (Conv2D.bn_sums)
#   dx, dx_gated        the backward-data launch without / with the activation derivative of the layer below in its epilogue (`gate_prev`)
#   fused_bwd           dx, dW and db from ONE pass over x where that exists (taken when the filter gradient is wanted), else None
#   halo                the forward runs on the fused 3x3 halo kernels
#   up2_kids            profiler ids of the upsample-fused forward / backward-data launches over the half-resolution map (where the input is a factor-2 upsample)
#   wants_planes, needs_fp32    what planes_demand answers the batch norm in front
ConvRoute = namedtuple("ConvRoute", "N H W Ho Wo pt pl geo flops fwd stats wgrad dx dx_gated fused_bwd halo up2_kids wants_planes needs_fp32")

# orientations of a packed filter bank: the `transpose_flip` values of ladder_filter_pack_split, which documents each layout (include/ladder_hip.h)
BANK_FWD, BANK_BWD, BANK_S2_BWD, BANK_UP2_FWD, BANK_UP2_BWD, BANK_S2_FWD, BANK_PROJ, BANK_PROJ_T = range(8)
# orientation -> (taps, cin, cout) of the packed bank of a layer with t = k * k taps, i input and o output channels
BANK_SHAPE = {BANK_FWD: lambda t, i, o: (t, i, o), BANK_BWD: lambda t, i, o: (t, o, i), BANK_S2_BWD: lambda t, i, o: (t, o, 4 * i),
              BANK_UP2_FWD: lambda t, i, o: (t, i, 4 * o), BANK_UP2_BWD: lambda t, i, o: (t, 4 * o, i), BANK_S2_FWD: lambda t, i, o: (t, 4 * i, o),
              BANK_PROJ: lambda t, i, o: (1, i, 9 * o), BANK_PROJ_T: lambda t, i, o: (1, 9 * o, i)}


class Conv2D:
    """tf.layers.conv2d (NHWC / HWIO), bias + activation fused in the kernel epilogue.  `want_bn_sums`: a batch norm follows -- a forward whose
    epilogue can emit the statistics of its output does (bn_sums)."""

    def __init__(self, ctx, ps, name, k, cin, cout, stride=1, padding="same", act=None, bias_grad=True, want_bn_sums=False):
        self.ctx, self.ps, self.name = ctx, ps, name
        self.k, self.cin, self.cout, self.stride, self.padding, self.act = k, cin, cout, stride, padding, act
        # a conv feeding batch-/instance-norm has an identically-zero bias gradient (the norm subtracts the mean):
        # it is not computed and stays 0 in the flat gradient buffer
        self.bias_grad = bias_grad
        self._packed = {}      # (transpose_flip, ns) -> [weight version, packed bf16 planes]
        self._routes = {}      # route()'s cache
        # optimiser group whose version stamps the packed images (a store of frozen weights outside the model names its own: fid.VGG16Features)
        self.group = getattr(ps, "group_of", arch.group_of)(name + "/kernel")
        self.want_bn_sums, self.bn_sums = want_bn_sums, None   # batch-norm statistics of the output from the conv epilogue
        self.kept = None                                        # Kept record of the last forward (None: a forward-only run kept nothing, or backward consumed it)

    def _keep(self, form, x, y, route, x_kind="input", factor=1, x_amax=None, keep=True):
        """The one place a forward variant records what the backward pass gets (backward() clears it)."""
        self.kept = Kept(form, x, x_kind, factor, y, x_amax, route) if keep else None

    def route(self, in_shape, x_kind="input"):
        """The ConvRoute of this layer over an input [N, H, W, cin] = `in_shape` whose kept operand is of kind `x_kind` (Kept.x_kind; for the other two
        kinds the shape is that of the upsampled tensor).  Every eligibility query, workspace size, profiler id and switch that routes the layer is
        consulted here and only here -- no device needed; routes are cached by everything that enters them."""
        ctx, halo_v, stats_v = self.ctx, switch("LADDER_DISABLE_HALO"), switch("LADDER_DISABLE_BNSTATS")      # (the values as set: the library reads both itself)
        key = (tuple(in_shape[:3]), x_kind != "input", ctx.ns, ctx.up2, ctx.keep_activations, halo_v, stats_v)
        if key not in self._routes:
            self._routes[key] = self._plan(*key[:5], halo_v == "1")
        return self._routes[key]

    def _plan(self, shape, upsampled_x, ns, up2, keep, halo_sw):
        (N, H, W), k, s, cin, cout = shape, self.k, self.stride, self.cin, self.cout
        (pt, Ho), (pl, Wo) = (arch.conv_out(d, k, s, self.padding) for d in (H, W))
        geo, M = (N, H, W, cin, Ho, Wo, cout, k, k, s, pt, pl), N * H * W
        sfx = "" if ns else "_f32"
        halo_off = ns == 0 and halo_sw                # (test switch: the round-1 generic fp32 gather kernels everywhere)
        stats = self.want_bn_sums and self.act is None

        def halo_ok(h, w, ci, co):
            # the fused 3x3 halo kernels of the configured precision (strict fp32: csrc/convf32.hip, and the 16- / 8-pixel-wide maps of
            # csrc/convf32s.hip; split formats: csrc/convsplit.hip) -- same tiling, same eligibility
            return bool(not halo_off and k == 3 and s == 1 and self.padding == "same"
                        and L.query("ladder_conv3x3_f32_eligible" if ns == 0 else "ladder_conv3x3_split_eligible", N, h, w, ci, co))

        def halo_kid(h, w, ci, co, class_cout=None):
            # profiler id of a halo-kernel launch over an [N, h, w] map with `ci` gathered and `co` bank columns: the 8x32-pixel tiling or -- strict
            # fp32 only -- a small-map tiling (csrc/convf32s.hip).  `class_cout`: channels per class of a class-structured launch (8x32 needs 128)
            if ns:
                return 256120 + ns
            big = L.query("ladder_conv3x3_split_eligible", N, h, w, ci, co) and (class_cout is None or class_cout == 128)
            return 256120 if big else 256064

        halo = halo_ok(H, W, cin, cout)
        # 1x1 conv over a tiny map (decoder conv0 on the 1x1 map) = a batch-sized dense layer
        dense = bool(k == 1 and s == 1 and M <= 512 and cin >= 16 and L.query("ladder_dense_small_eligible", M, cin, cout))
        # the image-side encoder conv (3 -> Cout channels, stride 2; csrc/convrgb.hip).  The kernels are f16x3 inside -- the filter gradient takes tensor-wide
        # absmax records -- so they belong to that precision mode; strict fp32 runs the fp32 instantiations
        rgb = bool(cin == 3 and (ns == 4 or (ns == 0 and not halo_sw)) and L.query("ladder_conv_rgb_s2_eligible", N, H, W, cin, cout, k, k, s, pt, pl))

        def plan_fwd():
            if halo:
                return Launch(self._fwd_halo, "ladder_conv3x3_split", None, halo_kid(H, W, cin, cout), BANK_FWD)
            if dense:
                return Launch(self._fwd_dense, "ladder_dense_fwd_small" + sfx)
            if rgb:
                return Launch(self._fwd_rgb, "ladder_conv_rgb_s2_fwd" + ("_bnstats" if stats else "") + sfx,
                              L.query("ladder_conv_rgb_s2_fwd_bnstats_workspace_bytes", N, H, W, cout) if stats else None)
            if ns and L.query("ladder_conv2d_fwd_split_eligible", *geo):
                nb = L.query("ladder_conv2d_fwd_split_workspace_bytes", *geo)
                snb = L.query("ladder_conv2d_fwd_split_bnstats_workspace_bytes", *geo) if stats and not nb else 0
                if snb:                                  # the epilogue also emits the batch-norm statistics of y (no second pass over it)
                    return Launch(self._fwd_gather_split, "ladder_conv2d_fwd_split_bnstats", snb, 0, BANK_FWD)
                return Launch(self._fwd_gather_split, "ladder_conv2d_fwd_split", nb, 0 if nb else 128120 + ns, BANK_FWD)    # (split-K launch: two kernels, not attributed)
            if ns == 0 and stats:
                snb = L.query("ladder_conv2d_fwd_bnstats_workspace_bytes", *geo)
                if snb:                                  # strict fp32: the epilogue also emits the batch-norm statistics of y (no second pass over it)
                    return Launch(self._fwd_gather, "ladder_conv2d_fwd_bnstats", snb)
            if ns == 0 and k == 3 and s == 2 and pt == 0 and pl == 0 and not halo_sw and L.query("ladder_conv3x3_s2_fwd_f32_eligible", N, H, W, cin, Ho, Wo, cout):
                # strict fp32, 3x3 / stride 2 over an even map (encoder conv2d_2 / conv2d_3): a stride-1 correlation over the four pixel-parity classes
                # of x on the halo kernels (x staged once per slab for all taps; csrc/convf32s.hip): 185 / 115 us against 202 / 127 on the gather kernel.
                # (Behind the statistics-epilogue branch above: conv2d_1 measures 344 us + a statistics pass here against 356 us with them.)
                return Launch(self._fwd_s2, "ladder_conv3x3_s2_fwd_f32", None, halo_kid(Ho, Wo, 4 * cin, cout), BANK_S2_FWD)
            return Launch(self._fwd_gather, "ladder_conv2d_fwd", *_igemm_plan(N * Ho * Wo, cin, cout, k * k * cin, (N, H, W, cin, Ho, Wo, cout, k, k, s, 1, pt, pl)))

        def plan_wgrad():
            if dense:
                return Launch(self._wg_dense, "ladder_dense_bwd_weight_small" + sfx)
            if rgb:                                      # (strict fp32: the fp32 filter-gradient kernel of the same layer)
                return Launch(self._wg_rgb, "ladder_conv_rgb_s2_bwd_filter" + sfx, L.query("ladder_conv_rgb_s2_bwd_filter_workspace_bytes", N, H, W, cout))
            # the 16-bit split formats on the halo kernels: their filter gradient / planes / absmax machinery
            if ns and halo and L.query("ladder_conv3x3_wgrad_split_eligible", N, H, W, cin, cout, ns):
                return Launch(self._wg_halo_split, "ladder_conv3x3_wgrad_split", L.query("ladder_conv3x3_wgrad_split_workspace_bytes", N, H, W, cin, cout), 9120 + ns)
            if ns and L.query("ladder_conv2d_bwd_filter_split_eligible", *geo):
                return Launch(self._wg_gather_split, "ladder_conv2d_bwd_filter_split", L.query("ladder_conv2d_bwd_filter_split_workspace_bytes", *geo[:9]))
            if (ns == 0 and upsampled_x and up2 >= 2 and (H // 2) * (W // 2) >= UP2W_MIN_PIXELS
                    and L.query("ladder_conv3x3_up2_wgrad_eligible", N, H // 2, W // 2, cin, cout)):
                # strict fp32, x = resize2x(x_lo): 25 instead of 36 tap tiles, read from the even sub-grid of the kept upsample (csrc/convf32.hip)
                return Launch(self._wg_up2, "ladder_conv3x3_up2_wgrad", L.query("ladder_conv3x3_up2_wgrad_workspace_bytes", N, H // 2, W // 2, cin, cout), 9120)
            return Launch(self._wg_gather, "ladder_conv2d_bwd_filter", L.query("ladder_conv2d_bwd_filter_workspace_bytes", *geo[:9]),
                          9128 if L.query("ladder_conv2d_bwd_filter_kernel_id", *geo) == 9128 else 0)

        def plan_dx(gated):
            if dense:
                return Launch(self._dx_dense, "ladder_dense_bwd_data_small" + sfx)
            if not gated and halo_ok(Ho, Wo, cout, cin):
                return Launch(self._dx_halo, "ladder_conv3x3_split", None, halo_kid(H, W, cout, cin), BANK_BWD)
            if (ns in (0, 4) and not gated and s == 2 and not halo_off
                    and (L.query("ladder_conv3x3_s2_bwd_data_split_eligible", *geo)
                         or (ns == 0 and k == 3 and pt == 0 and pl == 0 and L.query("ladder_conv3x3_s2_bwd_data_f32_eligible", N, H, W, cin, Ho, Wo, cout)))):
                # 3x3 / stride 2 over a map whose gradient is halo-kernel sized (enc.conv1): the four output-parity classes in ONE launch
                return Launch(self._dx_s2, "ladder_conv3x3_s2_bwd_data_split", None, halo_kid(Ho, Wo, cout, 4 * cin, cin), BANK_S2_BWD)
            if ns and L.query("ladder_conv2d_bwd_data_split_eligible", *geo, 1 if gated else 0):
                return Launch(self._dx_gather_split, "ladder_conv2d_bwd_data_split", L.query("ladder_conv2d_bwd_data_split_workspace_bytes", *geo), 0, BANK_BWD)
            # (a strided backward-data call is several parity-class launches: not attributed by the profiler)
            nb, kid = _igemm_plan(M, cout, cin, k * k * cout, (N, Ho, Wo, cout, H, W, cin, k, k, 1, 1, k - 1 - pt, k - 1 - pl))
            # strict fp32 3x3: the flipped / transposed fp32 bank is re-packed with all others in one launch per step, else transposed on the fly
            return Launch(self._dx_gather, "ladder_conv2d_bwd_data", nb, kid if s == 1 else 0, BANK_BWD if (ns == 0 and cout % 16 == 0 and k == 3) else None)

        fwd, wgrad = plan_fwd(), plan_wgrad()
        # 1x1 to <= 4 channels over a wide map (the CelebA output conv): dx, dW and db from ONE pass over x
        fused_bwd = Launch(self._bwd_smallcout, "ladder_conv1x1_smallcout_bwd_absmax", L.query("ladder_conv1x1_smallcout_bwd_workspace_bytes", M, cin, cout)) if (
            k == 1 and s == 1 and L.query("ladder_conv1x1_smallcout_eligible", M, cin, cout)) else None
        up2_kids = (halo_kid(H // 2, W // 2, cin, 4 * cout, cout), halo_kid(H // 2, W // 2, 4 * cout, cin))
        wants_planes = bool(ns == 4 and cin != 3 and fwd.fn.startswith("ladder_conv2d_fwd_split"))
        needs_fp32 = bool(not wants_planes or (keep and wgrad.fn != "ladder_conv2d_bwd_filter_split"))
        return ConvRoute(N, H, W, Ho, Wo, pt, pl, geo, 2.0 * N * Ho * Wo * k * k * cin * cout, fwd, "bnstats" in fwd.fn, wgrad, plan_dx(False), plan_dx(True),
                         fused_bwd, halo, up2_kids, wants_planes, needs_fp32)

    def planes_demand(self, in_shape):
        """(wants_planes, needs_fp32) for an input of `in_shape`: whether this layer's forward reads the fp16 plane images of its input
        (split gather kernel) and whether anything of it still needs the fp32 tensor (a filter gradient outside the split kernel)."""
        r = self.route(in_shape)
        return r.wants_planes, r.needs_fp32

    @staticmethod
    def _ps(Ho, Wo):
        """Per-sample f16x3 scales for the planes of this layer's operands: where the split filter-gradient kernel, which shares them,
        can re-scale at sample boundaries (a sample's output pixels = whole 32-pixel chunks)."""
        return (Ho * Wo) % 32 == 0

    def _wb(self):
        return _p(self.ps.w[self.name + "/kernel"]), _p(self.ps.w[self.name + "/bias"])

    def _grads(self):
        return _p(self.ps.g[self.name + "/kernel"]), _p(self.ps.g[self.name + "/bias"]) if self.bias_grad else None

    def _packed_filter(self, transpose_flip):
        """Split bf16 planes of the filter bank in the kernel's LDS layout, re-packed when the weights changed (always while a
        hipGraph is being captured, so that a replay re-packs the then-current weights)."""
        ns, ps = self.ctx.ns, self.ps
        if ns == 0 and transpose_flip == BANK_FWD:    # strict fp32: the HWIO bank IS the forward bank [tap][Cin][Cout]
            return ps.w[self.name + "/kernel"]
        taps, cin, cout = BANK_SHAPE[transpose_flip](self.k * self.k, self.cin, self.cout)
        ent = self._packed.get((transpose_flip, ns))
        if ent is None:
            nb = L.query("ladder_filter_pack_split_bytes", taps, cin, cout, ns)
            ent = self._packed[(transpose_flip, ns)] = [-1, torch.empty(nb, dtype=torch.uint8, device=self.ctx.device)]
            # known to the batched re-pack after an optimiser step (LadderEngine._repack_filters): (entry, bank, taps, cin, cout, flip, ns)
            self.ctx.pack_banks.append((ent, ps.w[self.name + "/kernel"], taps, cin, cout, transpose_flip, ns, self.group))
        ver = ps.version[self.group]
        if ent[0] != ver or torch.cuda.is_current_stream_capturing():
            L.call("ladder_filter_pack_split", _p(ps.w[self.name + "/kernel"]), _p(ent[1]), taps, cin, cout, transpose_flip, ns,
                   self.ctx.stream)
            ent[0] = ver
        return ent[1]

    def forward_fused_proj(self, x, proj, keep_y):
        """This 3x3 conv + activation followed by the 1x1 conv `proj` (<= 4 output channels, no activation) in ONE launch of the split
        halo kernel (ladder_conv3x3_split_proj); returns proj's output (plan_decoder decides eligibility).  `keep_y` = the
        activation is needed later (training forward: both layers' backward read it); a forward-only run never writes it."""
        N, H, W, _ = x.shape
        y = self.ctx.empty(N, H, W, self.cout) if keep_y else None
        out = self.ctx.empty(N, H, W, proj.cout)
        x_amax = self.ctx.absmax(x)
        args = (_p(x), _p(x_amax), _p(self._packed_filter(BANK_FWD)), _p(self.ps.w[self.name + "/bias"]), _p(y),
                _p(self.ps.w[proj.name + "/kernel"]), _p(self.ps.w[proj.name + "/bias"]), _p(out), proj.cout, N, H, W, self.cin, self.cout,
                L.ACT[self.act], self.ctx.ns, self.ctx.stream)
        _timed(256120 + self.ctx.ns, 2.0 * N * H * W * 9 * self.cin * self.cout, "ladder_conv3x3_split_proj", args)
        self._keep("plain", x, y, self.route(x.shape), x_amax=x_amax)
        proj._keep("plain", y, out, proj.route(out.shape))
        return out

    def _count_up2(self, tag, skipped):
        """bench.py's executed-FLOP model: one more upsample-fused launch `tag` of this layer, which never issues `skipped` of the reference's products."""
        self.ctx.up2_used[self.name + tag] = self.ctx.up2_used.get(self.name + tag, 0) + 1
        self.ctx.up2_skipped[self.name + tag] = skipped

    def _is_projection(self, proj):
        """`proj` is a 1x1 conv to <= 4 channels without activation on this layer's output (the RGB conv behind the last 3x3 conv)."""
        return bool(proj.k == 1 and proj.stride == 1 and proj.cout <= 4 and proj.act is None and proj.cin == self.cout)

    def _forward_proj(self, x, proj, keep_y, f, one_launch):
        """forward_up2 in the project-then-upsample form (csrc/upproj.hip; strict fp32, config `upsample_fused_convs` >= 4): resize by f -> this conv over
        the LOW-resolution x as nine 1x1 convolutions on it (9 of the direct form's 36 products per 2x2 output block at f = 2, 1 of 16 at f = 4)
        + an exact elementwise combination with bias, activation and -- for the last layer -- the 1x1 output conv on the activated value:
        Z [M, 9 cout] = x [M, cin] . wcat (dense kernel), then the combination; `one_launch`: both in ONE launch.  Returns (y, out)."""
        ctx, st = self.ctx, self.ctx.stream
        N, H, W = x.shape[0], x.shape[1], x.shape[2]
        M, n9 = N * H * W, 9 * self.cout
        flops = 2.0 * N * f * f * H * W * 9 * self.cin * self.cout      # the reference's operation count (algorithmic) ...
        executed = 2.0 * M * self.cin * n9                               # ... of which 9 / 36 are issued (factor 2; 1 / 16 at factor 4)
        self._count_up2(":train" if keep_y else "", 1.0 - 1.0 / (f * f))
        bias = self.ps.w[self.name + "/bias"]
        y = ctx.empty(N, f * H, f * W, self.cout) if (keep_y or proj is None) else None
        out, pw, pb, pco = y, None, None, 0
        if proj is not None:
            out, pco = ctx.empty(N, 2 * H, 2 * W, proj.cout), proj.cout
            pw, pb = self.ps.w[proj.name + "/kernel"], self.ps.w[proj.name + "/bias"]
        if one_launch:
            # round 6: GEMM + combination in ONE launch, the nine planes in an LDS ring (csrc/upproj.hip: up2proj_fused_fwd_kernel) -- Z never reaches HBM
            nb = L.query("ladder_up2proj_fused_workspace_bytes", N, H, W, self.cout, pco)
            wsp, wsn = ctx.ws(nb) if nb else (None, 0)
            _timed(128136, flops, "ladder_up2proj_fused_fwd",
                   (_p(x), _p(self._packed_filter(BANK_PROJ_T)), _p(bias), _p(y), _p(pw), _p(pb), _p(out) if proj is not None else None, pco, N, H, W, self.cin, self.cout,
                    L.ACT[self.act], wsp, wsn, st), executed)
            return y, out
        # (the nine planes Z are a transient [N H W, 9 cout] fp32 tensor: beyond PROJ_MAX_BYTES the layer takes the forms that allocate none)
        z = ctx.empty(M, n9)
        wsp, wsn = ctx.ws(L.query("ladder_igemm_fwd_workspace_bytes", M, self.cin, n9))
        _timed(128132 if L.query("ladder_dense_fwd_is_persistent", M, self.cin, n9) else abs(L.query("ladder_igemm_fwd_tile", M, self.cin, n9)), flops, "ladder_dense_fwd",
               (_p(x), _p(self._packed_filter(BANK_PROJ)), None, _p(z), M, self.cin, n9, 0, wsp, wsn, st), executed)
        if proj is not None:
            L.call("ladder_up2proj_fwd_combine", _p(z), _p(bias), _p(y), _p(pw), _p(pb), _p(out), proj.cout, N, H, W, self.cout, L.ACT[self.act], st)
        else:
            L.call("ladder_upfproj_fwd_combine", _p(z), _p(bias), _p(y), f, N, H, W, self.cout, L.ACT[self.act], st)
        return y, out

    def _forward_tapfold(self, x, proj, keep_y, kid):
        """forward_up2 in the tap-folded form (ladder_conv3x3_up2_split: four output-parity classes with effective taps, 25 instead of 36
        low-resolution tap products and no upsampled tensor; `kid`: its profiler id) + its exact border lines.  Returns (y, out, absmax record of x)."""
        ctx = self.ctx
        N, H, W = x.shape[0], x.shape[1], x.shape[2]
        strided = 0
        bias, wk = self.ps.w[self.name + "/bias"], self.ps.w[self.name + "/kernel"]
        x_amax = ctx.absmax(x)                                           # (max |upsampled| = max |x|: the resize is a convex combination)
        flops = 2.0 * N * 4 * H * W * 9 * self.cin * self.cout          # the reference's operation count (algorithmic) ...
        executed = flops * 25.0 / 36.0                                   # ... of which 25 / 36 are issued
        self._count_up2(":train" if keep_y else "", 11.0 / 36.0)          # (forward-only / training forward)
        wsp, wsn = ctx.ws(L.query("ladder_conv3x3_up2_edges_workspace_bytes", N, H, W, self.cin, self.cout))
        if proj is not None:
            y = ctx.empty(N, 2 * H, 2 * W, self.cout) if keep_y else None
            out = ctx.empty(N, 2 * H, 2 * W, proj.cout)
            pw, pb = self.ps.w[proj.name + "/kernel"], self.ps.w[proj.name + "/bias"]
            _timed(kid, flops, "ladder_conv3x3_up2_split_proj",
                   (_p(x), _p(x_amax), _p(self._packed_filter(BANK_UP2_FWD)), _p(bias), _p(y), _p(pw), _p(pb), _p(out), proj.cout, N, H, W, self.cin, self.cout,
                    L.ACT[self.act], ctx.ns, strided, ctx.stream), executed)
            L.call("ladder_conv3x3_up2_edges", _p(x), _p(wk), _p(bias), _p(y), None, _p(pw), _p(pb), _p(out), proj.cout, N, H, W, self.cin, self.cout,
                   L.ACT[self.act], strided, wsp, wsn, ctx.stream)
            return y, out, x_amax
        y = ctx.empty(N, 2 * H, 2 * W, self.cout)
        y_amax = ctx.new_amax() if ctx.ns == 4 else None
        _timed(kid, flops, "ladder_conv3x3_up2_split",
               (_p(x), _p(x_amax), _p(self._packed_filter(BANK_UP2_FWD)), _p(bias), _p(y), _p(y_amax), N, H, W, self.cin, self.cout, L.ACT[self.act], ctx.ns,
                strided, ctx.stream), executed)
        L.call("ladder_conv3x3_up2_edges", _p(x), _p(wk), _p(bias), _p(y), _p(y_amax), None, None, None, 0, N, H, W, self.cin, self.cout,
               L.ACT[self.act], strided, wsp, wsn, ctx.stream)
        ctx.set_amax(y, y_amax)
        return y, y, x_amax

    def forward_up2(self, x, pair, proj=None, keep_y=False, upsampled=None):
        """conv(resize(x)) from the low-resolution x itself, in the form the PairPlan `pair` names; with `proj` the 1x1 output conv rides on the
        epilogue as in forward_fused_proj, or follows as a launch of its own.  Forward-only runs keep nothing.  A training forward (`keep_y`)
        keeps `upsampled` = the resized tensor where the plan materialised it (filter gradient and backward-data are then those of the plain
        convolution on it), else x itself (all three passes run from the low-resolution tensor)."""
        if proj is not None and pair.proj == "follows":
            # the fused 1x1 epilogues hold one pixel's 128 channels in a half-wave and project to <= 4 columns (csrc/upproj.hip, convf32.hip):
            # any other last-layer width (num_hidden_units != 512) runs the pair unfused -- this conv from the low-resolution tensor, then `proj`
            out = proj.forward(self.forward_up2(x, pair, None, keep_y, upsampled))
            if not keep_y:
                proj.kept = None
            return out
        # (upsampled: x = the factor-2 upsample of a tensor, the filter gradient reads its even sub-grid)
        kept_x, x_kind, x_amax = (x, "lowres", None) if upsampled is None else (upsampled, "upsampled", None)
        r = self.route((x.shape[0], pair.factor * x.shape[1], pair.factor * x.shape[2], self.cin), x_kind)
        if pair.form == "projected":
            y, out = self._forward_proj(x, proj, keep_y, pair.factor, pair.one_launch)
        else:
            y, out, x_amax = self._forward_tapfold(x, proj, keep_y, r.up2_kids[0])
        self._keep(pair.form, kept_x, y, r, x_kind, pair.factor, x_amax, keep=keep_y)
        if proj is not None:
            proj._keep("plain", y, out, proj.route(out.shape), keep=keep_y)
        return out

    def forward(self, x):
        r = self.route(x.shape)
        y = self.ctx.empty(r.N, r.Ho, r.Wo, self.cout)
        self._keep("plain", x, y, r, x_amax=r.fwd.run(r, x, y))
        return y

    # -- one launch function per forward route: each assembles the arguments of r.fwd.fn and launches; returns the absolute-maximum record of x where
    # the kernel took one (the filter gradient re-uses it)
    def _fwd_halo(self, r, x, y):
        ctx = self.ctx
        x_amax = ctx.absmax(x)
        y_amax = ctx.new_amax() if ctx.ns == 4 else None
        ctx.set_amax(y, y_amax)
        _timed(r.fwd.kid, r.flops, r.fwd.fn, (_p(x), _p(x_amax), _p(self._packed_filter(BANK_FWD)), self._wb()[1], _p(y), _p(y_amax), r.N, r.H, r.W,
                                              self.cin, self.cout, L.ACT[self.act], ctx.ns, ctx.stream))
        return x_amax

    def _fwd_dense(self, r, x, y):
        L.call(r.fwd.fn, _p(x), *self._wb(), _p(y), r.N * r.H * r.W, self.cin, self.cout, L.ACT[self.act], self.ctx.stream)

    def _sums(self, r):
        """Where the forward's epilogue emits the batch-norm statistics (such a layer has no activation): (pointer to a fresh record bn_sums,), else ()."""
        if not r.stats:
            return ()
        self.bn_sums = self.ctx.empty(6 * self.cout)       # sum | sum of squares | min | max per channel
        return (_p(self.bn_sums),)

    def _fwd_rgb(self, r, x, y):
        ws = self.ctx.ws(r.fwd.ws) if r.stats else ()
        L.call(r.fwd.fn, _p(x), *self._wb(), _p(y), r.N, r.H, r.W, self.cout, L.ACT[self.act], *self._sums(r), *ws, self.ctx.stream)

    def _fwd_gather_split(self, r, x, y):
        ctx = self.ctx
        x_amax = ctx.absmax(x)
        wsp, wsn = ctx.ws(r.fwd.ws)
        args = (_p(ctx.planes(x, self._ps(r.Ho, r.Wo))), _p(x_amax), _p(self._packed_filter(BANK_FWD)), self._wb()[1], _p(y)) + r.geo
        _timed(r.fwd.kid, r.flops, r.fwd.fn, args + (L.ACT[self.act], ctx.ns, *self._sums(r), wsp, wsn, ctx.stream))
        return x_amax

    def _fwd_s2(self, r, x, y):
        _timed(r.fwd.kid, r.flops, r.fwd.fn, (_p(x), _p(self._packed_filter(BANK_S2_FWD)), self._wb()[1], _p(y), r.N, r.H, r.W, self.cin, r.Ho, r.Wo,
                                              self.cout, L.ACT[self.act], self.ctx.stream))

    def _fwd_gather(self, r, x, y):
        wsp, wsn = self.ctx.ws(r.fwd.ws)
        _timed(r.fwd.kid, r.flops, r.fwd.fn, (_p(x), *self._wb(), _p(y), *r.geo, L.ACT[self.act], *self._sums(r), wsp, wsn, self.ctx.stream),
               _gather_executed(r.fwd.kid, r.flops, r.geo, False))

    def _backward_proj(self, dy, need_dx, wgrad, gate, proj_grad=None):
        """Backward of the project-then-upsample form from the low-resolution x: D [M, 9 cout] = (shift o up)^T dy once (elementwise), then
        dWcat = x^T D (+ the bias gradient as the centre plane's column sums) and dx_lo = D . wcatT -- two dense calls, exact on every pixel.
        `proj_grad` = (dyp, proj): dy is not given -- D comes from this layer's activated output and the gradient dyp of the 1x1 conv `proj`
        behind it, together with proj's own filter / bias gradient (plan_decoder: proj_grad)."""
        ctx, st = self.ctx, self.ctx.stream
        x, f = self.kept.x, self.kept.factor
        N, H, W, _ = x.shape
        M, n9 = N * H * W, 9 * self.cout
        flops = 2.0 * N * f * f * H * W * 9 * self.cin * self.cout
        executed = 2.0 * M * self.cin * n9
        d = ctx.empty(M, n9)
        if proj_grad is not None:
            dyp, proj = proj_grad
            wsp, wsn = ctx.ws(L.query("ladder_up2proj_bwd_combine_proj_workspace_bytes", N, H, W, self.cout, proj.cout))
            L.call("ladder_up2proj_bwd_combine_proj", _p(self.kept.y), _p(dyp), _p(proj.ps.w[proj.name + "/kernel"]), _p(d), _p(proj.ps.g[proj.name + "/kernel"]),
                   _p(proj.ps.g[proj.name + "/bias"]) if proj.bias_grad else None, proj.cout, N, H, W, self.cout, L.ACT[self.act] if self.act else 0,
                   wsp, wsn, st)
            proj.kept = None
        else:
            L.call("ladder_upfproj_bwd_combine", _p(dy), _p(d), f, N, H, W, self.cout, st)
        if wgrad:
            self._count_up2(":wgrad", 1.0 - 1.0 / (f * f))
            dwcat, db9 = ctx.empty(self.cin, n9), (ctx.empty(n9) if self.bias_grad else None)   # (a conv in front of a norm has no bias gradient)
            wsp, wsn = ctx.ws(L.query("ladder_dense_bwd_weight_workspace_bytes", M, self.cin, n9))
            _timed(9132 if L.query("ladder_dense_bwd_weight_is_persistent", M, self.cin, n9) else 9130, flops, "ladder_dense_bwd_weight",
                   (_p(x), _p(d), _p(dwcat), _p(db9), M, self.cin, n9, wsp, wsn, st), executed)
            L.call("ladder_up2proj_wgrad_unpack", _p(dwcat), _p(db9), _p(self.ps.g[self.name + "/kernel"]),
                   _p(self.ps.g[self.name + "/bias"]) if self.bias_grad else None, self.cin, self.cout, st)
        dx = None
        if need_dx:
            self._count_up2(":bwd", 1.0 - 1.0 / (f * f))
            dx = ctx.empty(N, H, W, self.cin)
            wsp, wsn = ctx.ws(L.query("ladder_igemm_fwd_workspace_bytes", M, n9, self.cin))
            gy, gact = gate if gate is not None else (None, None)
            # (ladder_dense_bwd_data: dx [M, K] = dy [M, N] . wT [N, K], optionally times act'(gate) -- here dy := D, wT := wcatT)
            if L.query("ladder_dense_fwd_is_persistent", M, n9, self.cin):
                # K-contiguous weight operand = wcat itself (orientation 6): gemm_nt16_f32_kernel (v_mfma_f32_16x16x4_f32; 3-5 % ahead of the 32x32x2 kernel
                # on this long-K shape: conv2d_7 1 202 against 1 266 us, profiles/r05_gemm_library_probe.txt)
                _timed(128134, flops, "ladder_dense_bwd_data_nt",
                       (_p(d), _p(self._packed_filter(BANK_PROJ)), _p(dx), M, self.cin, n9, _p(gy), L.ACT[gact] if gact else 0, st), executed)
            else:
                _timed(abs(L.query("ladder_igemm_fwd_tile", M, n9, self.cin)), flops, "ladder_dense_bwd_data",
                       (_p(d), _p(self._packed_filter(BANK_PROJ_T)), _p(dx), M, self.cin, n9, _p(gy), L.ACT[gact] if gact else 0, wsp, wsn, st), executed)
        return dx

    def _dx_lowres(self, dy, dy_amax, kid, gate=None):
        """d loss / d x_lo for y = conv(resize2x(x_lo)): the composite transpose is a zero-padded 5x5 / stride-2 correlation over dy (one launch of
        the halo kernel, 25 instead of 36 tap products per low-resolution pixel, the [N, 2H, 2W, cin] intermediate never written), exact on
        every pixel (`kid`: that launch's profiler id) but the four border lines of dx, where the resize's clamp and the convolution's padding change the coefficients: those
        come from 4-pixel-wide strips of dy through the plain backward-data + resize-transpose kernels (exact there by construction)."""
        ctx, st = self.ctx, self.ctx.stream
        N, OH, OW, _ = dy.shape
        H, W = OH // 2, OW // 2
        dx = ctx.empty(N, H, W, self.cin)
        dx_amax = ctx.new_amax() if ctx.ns == 4 else None
        flops = 2.0 * N * OH * OW * 9 * self.cin * self.cout
        self._count_up2(":bwd", 11.0 / 36.0)
        pk4 = self._packed_filter(BANK_UP2_BWD)
        if ctx.ns == 0:
            # strict fp32: the main launch, then its four border lines made exact in place from ONE d_up line per border (csrc/convf32.hip:
            # ladder_conv3x3_up2_bwd_borders -- 9 instead of 45 line-taps per axis; the strip path below cost 1.07 ms per iteration)
            wsp, wsn = ctx.ws(L.query("ladder_conv3x3_up2_bwd_borders_workspace_bytes", N, H, W, self.cout, self.cin))
            if gate is not None:        # (y of the layer below, its activation): dx *= act'(y) in the epilogue and in the border fix-up
                gy, gact = gate
                _timed(kid, flops, "ladder_conv3x3_up2_bwd_data_gated_f32",
                       (_p(dy), _p(pk4), _p(dx), _p(gy), L.ACT[gact], N, H, W, self.cout, self.cin, st), flops * 25.0 / 36.0)
                L.call("ladder_conv3x3_up2_bwd_borders_gated", _p(dy), _p(self.ps.w[self.name + "/kernel"]), _p(dx), _p(gy), L.ACT[gact], N, H, W, self.cout,
                       self.cin, wsp, wsn, st)
                return dx
            _timed(kid, flops, "ladder_conv3x3_up2_bwd_data_split",
                   (_p(dy), None, _p(pk4), _p(dx), None, N, H, W, self.cout, self.cin, 0, st), flops * 25.0 / 36.0)
            L.call("ladder_conv3x3_up2_bwd_borders", _p(dy), _p(self.ps.w[self.name + "/kernel"]), _p(dx), N, H, W, self.cout, self.cin, wsp, wsn, st)
            return dx
        pk = self._packed_filter(BANK_BWD)
        # border lines: dx row 0 = R(d_up[0] + d_up[1] / 2), row H-1 = R(d_up[2H-3] / 2 + d_up[2H-2] + d_up[2H-1]) with d_up = the plain
        # backward-data (needs dy rows 0..2 resp. 2H-4..2H-1) and R = the resize transpose ALONG the line; columns alike
        strips = []
        for axis, first in ((1, True), (1, False), (2, True), (2, False)):
            n_dy, n_up = (3, 2) if first else (4, 3)                      # strip widths: dy lines read, d_up lines produced
            O_ = OH if axis == 1 else OW
            sl = slice(0, n_dy) if first else slice(O_ - n_dy, O_)
            pad = 1 if first else 2                                        # forward-convolution padding that aligns the strip (see csrc/igemm.hip)
            if axis == 1:
                geo = (N, n_up, OW, self.cin, n_dy, OW, self.cout, 3, 3, 1, pad, 1)
                view, s, dup = dy[:, sl], ctx.empty(N, n_dy, OW, self.cout), ctx.empty(N, n_up, OW, self.cin)
            else:
                geo = (N, OH, n_up, self.cin, OH, n_dy, self.cout, 3, 3, 1, 1, pad)
                view, s, dup = dy[:, :, sl], ctx.empty(N, OH, n_dy, self.cout), ctx.empty(N, OH, n_up, self.cin)
            strips.append((axis, first, geo, view, s, dup))
        # (Round 4 tried the four strips -- 256-384 tiles of the gather kernel each: a quarter of the chip's workgroup slots -- on four side
        # streams beside each other in the fp32 build: 3 125 -> 2 845 img/s.  Every cross-stream dependency drains both queues on this runtime;
        # 18 of them per iteration cost far more than the 0.5 ms the overlap could save.)
        _timed(256120 + ctx.ns, flops, "ladder_conv3x3_up2_bwd_data_split",
               (_p(dy), _p(dy_amax), _p(pk4), _p(dx), _p(dx_amax), N, H, W, self.cout, self.cin, ctx.ns, st), flops * 25.0 / 36.0)
        for axis, first, geo, view, s, dup in strips:
            s.copy_(view)
            ctx.set_amax(s, dy_amax)                                       # (a strip of dy: the per-sample record of dy bounds it, no extra pass)
            s_amax = ctx.absmax(s)
            wsp, wsn = ctx.ws(L.query("ladder_conv2d_bwd_data_split_workspace_bytes", *geo))
            L.call("ladder_conv2d_bwd_data_split", _p(ctx.planes(s, self._ps(geo[1], geo[2]))), _p(s_amax), _p(pk), _p(dup), *geo, None, 0, ctx.ns, wsp, wsn, st)
            L.call("ladder_conv3x3_up2_bwd_border", _p(dup), _p(dx), _p(dx_amax), N, H, W, self.cin, axis, 1 if first else 0, st)
        ctx.set_amax(dx, dx_amax)
        return dx

    def backward(self, dy, need_dx=True, wgrad=True, act_done=False, gate_prev=None, lowres_dx=False, lowres_gate=None, proj_grad=None):
        """`act_done`: dy already carries this layer's activation derivative (fused into the consumer's epilogue).
        `proj_grad` = (dyp, proj) instead of dy: see _backward_proj.
        `gate_prev`: activation name of the layer that produced this conv's input x: its derivative act'(x) is fused into
        the backward-data epilogue, so that layer must then be called with act_done=True.
        `lowres_dx`: x is the factor-2 upsample of a tensor the caller wants the gradient of: return d / d (that tensor) (see _dx_lowres)."""
        try:
            return self._backward(self.kept, dy, need_dx, wgrad, act_done, gate_prev, lowres_dx, lowres_gate, proj_grad)
        finally:
            self.kept = None          # the one place the record of the forward is dropped

    def _backward(self, k, dy, need_dx, wgrad, act_done, gate_prev, lowres_dx, lowres_gate, proj_grad):
        r, x, x_amax, ctx = k.route, k.x, k.x_amax, self.ctx
        lo = k.x_kind == "lowres"                         # x is the low-resolution tensor: the layer's input is its (never materialised) upsample
        if proj_grad is not None:
            if not (wgrad and lo and k.form == "projected" and k.factor == 2):
                raise RuntimeError("%s: the projection-gradient form of the backward combination does not apply" % self.name)
            return self._backward_proj(None, need_dx, wgrad, lowres_gate, proj_grad)
        if self.act is not None and not act_done:
            L.call("ladder_act_bwd", _p(dy), _p(k.y), _p(dy), dy.numel(), L.ACT[self.act], ctx.stream)
        if lo and k.form == "projected":
            return self._backward_proj(dy, need_dx, wgrad, lowres_gate)
        if wgrad and r.fused_bwd is not None:
            return r.fused_bwd.run(r, x, dy, need_dx, gate_prev)
        wg, dl = r.wgrad if wgrad else None, (r.dx_gated if gate_prev else r.dx) if need_dx else None
        halo_w, halo_d = bool(wg and wg.fn == "ladder_conv3x3_wgrad_split"), bool(dl and dl.fn == "ladder_conv3x3_split")
        if halo_w and x_amax is None:
            x_amax = ctx.absmax(x)                      # (a record only under f16x3, else None)
        dy_amax = ctx.absmax(dy) if (halo_w or halo_d) else None        # one pass serves the filter gradient and the backward-data call
        if wg is not None:
            wg.run(r, x, dy, x_amax, dy_amax, lo)
        if lowres_dx:
            if not halo_d:
                raise RuntimeError("%s: the low-resolution backward-data was requested for a call the split halo kernels do not take" % self.name)
            return self._dx_lowres(dy, dy_amax, r.up2_kids[1], lowres_gate)
        if dl is None:
            return None
        dx = ctx.empty(r.N, r.H, r.W, self.cin)
        dl.run(r, dl, x, dy, dx, dy_amax, gate_prev)
        return dx

    # -- one launch function per backward route (filter gradient: r.wgrad; backward-data: `dl` = r.dx or r.dx_gated, `gate` = the activation name)
    def _bwd_smallcout(self, r, x, dy, need_dx, gate):
        ctx, M = self.ctx, r.N * r.H * r.W
        wsp, wsn = ctx.ws(r.fused_bwd.ws)
        dx = ctx.empty(r.N, r.H, r.W, self.cin) if need_dx else None
        dx_amax = ctx.new_amax() if (need_dx and ctx.ns == 4) else None
        L.call(r.fused_bwd.fn, _p(x), _p(dy), self._wb()[0], _p(dx), *self._grads(), M, self.cin, self.cout, L.ACT[gate] if gate else 0, wsp, wsn,
               _p(dx_amax), r.H * r.W, ctx.stream)
        if dx is not None:
            ctx.set_amax(dx, dx_amax)
        return dx

    def _wg_dense(self, r, x, dy, x_amax, dy_amax, lo):
        L.call(r.wgrad.fn, _p(x), _p(dy), *self._grads(), r.N * r.H * r.W, self.cin, self.cout, self.ctx.stream)

    def _wg_rgb(self, r, x, dy, x_amax, dy_amax, lo):
        ctx = self.ctx
        xa, da = (ctx.absmax(x), ctx.absmax(dy)) if ctx.ns else (None, None)
        with ctx.side_or_main(x, dy, xa, da):
            wsp, wsn = ctx.ws(r.wgrad.ws)
            ops = (_p(x), _p(xa), _p(dy), _p(da)) if ctx.ns else (_p(x), _p(dy))
            L.call(r.wgrad.fn, *ops, *self._grads(), r.N, r.H, r.W, self.cout, wsp, wsn, ctx.stream)

    def _wg_halo_split(self, r, x, dy, x_amax, dy_amax, lo):
        # (on the side stream: the filter gradient is MFMA-bound and only the optimiser step needs it; the backward-data call
        # and the HBM-bound resize / norm backward kernels of the layers underneath run beside it)
        ctx = self.ctx
        with ctx.side_or_main(x, dy, x_amax, dy_amax):
            wsp, wsn = ctx.ws(r.wgrad.ws)
            _timed(r.wgrad.kid, r.flops, r.wgrad.fn, (_p(x), _p(x_amax), _p(dy), _p(dy_amax), *self._grads(), r.N, r.H, r.W, self.cin, self.cout,
                                                            ctx.ns, wsp, wsn, ctx.stream))

    def _wg_gather_split(self, r, x, dy, x_amax, dy_amax, lo):
        ctx = self.ctx
        x_amax, dy_amax = ctx.absmax(x) if x_amax is None else x_amax, ctx.absmax(dy)
        ps_ = self._ps(r.Ho, r.Wo)
        xpl, dpl = ctx.planes(x, ps_), ctx.planes(dy, ps_)          # (split on the main stream: backward-data reads dy's planes too)
        with ctx.side_or_main(x, dy, xpl, dpl, x_amax, dy_amax):
            wsp, wsn = ctx.ws(r.wgrad.ws)
            L.call(r.wgrad.fn, _p(xpl), _p(x_amax), _p(dpl), _p(dy_amax), *self._grads(), *r.geo, ctx.ns, wsp, wsn, ctx.stream)

    def _wg_up2(self, r, x, dy, x_amax, dy_amax, lo):
        ctx, fl = self.ctx, r.flops
        wsp, wsn = ctx.ws(r.wgrad.ws)
        self._count_up2(":wgrad", 11.0 / 36.0)
        _timed(r.wgrad.kid, fl, r.wgrad.fn, (_p(x), 0 if lo else 1, _p(dy), *self._grads(), r.N, r.H // 2, r.W // 2, self.cin, self.cout, wsp, wsn,
                                            ctx.stream), fl * 25.0 / 36.0)

    def _wg_gather(self, r, x, dy, x_amax, dy_amax, lo):
        # (a low-resolution x is [N, H/2, W/2, cin]: the generic kernel would read 4x past it.  plan_decoder plans a virtual upsample only where
        # ladder_conv3x3_up2_wgrad takes the filter gradient)
        assert not lo, "%s: virtual upsample without the low-resolution filter gradient" % self.name
        wsp, wsn = self.ctx.ws(r.wgrad.ws)
        _timed(r.wgrad.kid, r.flops, r.wgrad.fn, (_p(x), _p(dy), *self._grads(), *r.geo, wsp, wsn, self.ctx.stream))    # (+ its fixed-order split reduction)

    def _dx_dense(self, r, dl, x, dy, dx, dy_amax, gate):
        gate_args = (_p(x), L.ACT[gate]) if gate else (None, 0)
        L.call(dl.fn, _p(dy), self._wb()[0], _p(dx), r.N * r.H * r.W, self.cin, self.cout, *gate_args, self.ctx.stream)

    def _dx_halo(self, r, dl, x, dy, dx, dy_amax, gate):
        ctx = self.ctx
        dx_amax = ctx.new_amax() if ctx.ns == 4 else None
        ctx.set_amax(dx, dx_amax)
        _timed(dl.kid, r.flops, dl.fn,
               (_p(dy), _p(dy_amax), _p(self._packed_filter(BANK_BWD)), None, _p(dx), _p(dx_amax), r.N, r.H, r.W, self.cout, self.cin, 0, ctx.ns, ctx.stream))

    def _dx_s2(self, r, dl, x, dy, dx, dy_amax, gate):
        ctx = self.ctx
        dy_amax = ctx.absmax(dy)
        dx_amax = ctx.new_amax() if ctx.ns == 4 else None
        ctx.set_amax(dx, dx_amax)
        _timed(dl.kid, 2.0 * r.N * r.Ho * r.Wo * 9 * self.cin * self.cout, dl.fn,
               (_p(dy), _p(dy_amax), _p(self._packed_filter(BANK_S2_BWD)), _p(dx), _p(dx_amax), r.N, r.H, r.W, self.cin, r.Ho, r.Wo, self.cout, ctx.ns, ctx.stream))

    def _dx_gather_split(self, r, dl, x, dy, dx, dy_amax, gate):
        ctx = self.ctx
        dy_amax = ctx.absmax(dy)
        wsp, wsn = ctx.ws(dl.ws)
        L.call(dl.fn, _p(ctx.planes(dy, self._ps(r.Ho, r.Wo))), _p(dy_amax), _p(self._packed_filter(BANK_BWD)), _p(dx), *r.geo,
               _p(x) if gate else None, L.ACT[gate] if gate else 0, ctx.ns, wsp, wsn, ctx.stream)

    def _dx_gather(self, r, dl, x, dy, dx, dy_amax, gate):
        ctx = self.ctx
        wT = self._packed_filter(dl.bank) if dl.bank is not None else ctx.empty(self.k * self.k * self.cin * self.cout)
        if dl.bank is None:
            L.call("ladder_filter_flip_transpose", self._wb()[0], _p(wT), self.k, self.k, self.cin, self.cout, ctx.stream)
        wsp, wsn = ctx.ws(dl.ws)
        flops = 2.0 * r.N * r.H * r.W * self.k * self.k * self.cin * self.cout
        _timed(dl.kid, flops, dl.fn,
               (_p(dy), _p(wT), _p(dx), *r.geo, _p(x) if gate else None, L.ACT[gate] if gate else 0, wsp, wsn, ctx.stream),
               _gather_executed(dl.kid, flops, r.geo, True))


# How one block of the CelebA decoder (resize in front -> 3x3 conv -> [instance norm] -> resize behind) runs, forward and backward:
#   resize      the resize in FRONT of the conv: None (none, or the identity) | "materialise" (a resize pass writes the resized tensor, the conv reads it) |
#               "keep_both" (training: the conv reads the low-resolution tensor, the resized one is written beside it for the backward pass) |
#               "virtual" (training: forward, backward-data and filter gradient all run from the low-resolution tensor, the resized one never exists) |
#               "fold_forward_only" (forward-only run: the conv reads the low-resolution tensor, nothing is kept);  factor: 2 or 4 (0: neither)
#   form        of the conv (Kept.form);  one_launch: projected form as GEMM + combination in one launch
#   proj        the 1x1 RGB conv behind the last 3x3 conv: None (a layer call of its own after the loop) | "rides" (on this conv's epilogue) |
#               "follows" (an upsample-fused conv whose epilogue cannot take it: the conv, then the 1x1 conv)
#   norm_out    what this block's instance norm writes: None (no norm) | "lowres" (its plain output) | "resized" (only the resize of it, by the resize
#               behind the block) | "both";  behind: `resize` of the next block (last block: None, or "materialise")
#   lowres_dx   backward: the conv's backward-data returns the gradient of the low-resolution tensor (the transpose of the resize in front is in it) ...
#   lgate       ... and applies the activation derivative of the conv below;  pre_gated: dy arrives with this conv's derivative applied that way
#   rs_bwd      the transpose of the resize behind runs as a launch of its own;  gated: ... and applies this conv's activation derivative
#   fuse_last   last block: the 1x1 conv's backward-data applies this conv's activation derivative;  proj_grad: ... or rather the backward combination of
#               the projected form is formed straight from the 1x1 conv's gradient (ladder_up2proj_bwd_combine_proj: dy of this layer never exists)
PairPlan = namedtuple("PairPlan", "resize factor form one_launch proj norm_out behind lowres_dx lgate pre_gated gated rs_bwd fuse_last proj_grad")


def plan_decoder(cache, ctx, up0, blocks, conv_out, shape):
    """One PairPlan per block of `blocks` [(conv, style dense, norm, resize behind)] for an input map `shape` = (N, H, W) in front of the resize `up0`,
    under ctx.keep_activations.  Every eligibility query, config level and switch that routes a resize -> conv pair is consulted here and only here;
    CelebADecoder.forward and .backward follow the list.  Plans are cached in `cache` by everything that enters them."""
    keep, ns, up2 = ctx.keep_activations, ctx.ns, ctx.up2
    halo_sw, gate_sw = halo_disabled(), switch("LADDER_ENABLE_LOWRES_GATE") == "1"
    key = (tuple(shape), keep, ns, up2, ctx.fuse_fwd, ctx.fuse_bwd_proj, halo_sw, gate_sw)
    if key in cache:
        return cache[key]
    N = shape[0]
    halo_off = ns == 0 and halo_sw          # (test switch: the round-1 generic fp32 gather kernels everywhere)

    def c3(c):
        return c.k == 3 and c.stride == 1 and c.padding == "same"

    def factor(rs, H, W):                   # integer factor (2 or 4) of resize `rs` applied to an H x W map, 0 when it is neither
        return next((f for f in (2, 4) if rs is not None and (rs.oh, rs.ow) == (f * H, f * W)), 0)

    def proj_ok(c, H, W, f):
        # projected form (strict fp32, config `upsample_fused_convs` >= 4; factor 2 or 4).  The nine planes Z / D are a transient [N H W, 9 cout] fp32
        # tensor: beyond PROJ_MAX_BYTES the pair takes the forms that allocate none
        return bool(ns == 0 and up2 >= 4 and c3(c) and not halo_sw and 36 * N * H * W * c.cout <= PROJ_MAX_BYTES
                    and L.query("ladder_upfproj_eligible", f, N, H, W, c.cin, c.cout))

    def fold_ok(c, H, W, f):
        # the conv can take the LOW-resolution tensor [N, H, W, cin] in its forward: projected (factor 2 or 4), else tap-folded (factor 2)
        if proj_ok(c, H, W, f):
            return True
        return bool(f == 2 and not halo_off and up2 and ns in (0, 2, 4) and c3(c) and L.query("ladder_conv3x3_up2_split_eligible", N, H, W, c.cin, c.cout, ns))

    def tap_bwd_ok(c, H, W):
        # the gradient of the low-resolution tensor behind a MATERIALISED factor-2 resize from ONE launch (ladder_conv3x3_up2_bwd_data_split) + border strips
        if halo_off:
            return False
        if ns == 0 and H * W < UP2T_MIN_PIXELS:
            # policy (measured, profiles/r05_small_maps.txt): on an 8x8 low-resolution map the four exact border lines cost more than the
            # 11 / 36 of the products the fused launch saves (conv2d_4: 461 + 221 us against 595 + 26 for the direct pair)
            return False
        return bool(up2 >= 2 and ns in (0, 2, 4) and c3(c) and L.query("ladder_conv3x3_up2_bwd_data_split_eligible", N, H, W, c.cout, c.cin, ns)
                    and (ns == 0 or all(L.query("ladder_conv2d_bwd_data_split_eligible", *g, 0) for g in (
                        (N, 2, 2 * W, c.cin, 3, 2 * W, c.cout, 3, 3, 1, 1, 1), (N, 3, 2 * W, c.cin, 4, 2 * W, c.cout, 3, 3, 1, 2, 1),
                        (N, 2 * H, 2, c.cin, 2 * H, 3, c.cout, 3, 3, 1, 1, 1), (N, 2 * H, 3, c.cin, 2 * H, 4, c.cout, 3, 3, 1, 1, 2)))))

    def virtual_ok(c, H, W, f):
        # a training forward may skip materialising the resize altogether: strict fp32, and forward, backward-data AND filter gradient of the conv all
        # run from the low-resolution tensor (projected form; or, factor 2, the tap-folded kernels of csrc/convf32.hip)
        if proj_ok(c, H, W, f):
            return True
        return bool(f == 2 and ns == 0 and up2 >= 3 and fold_ok(c, H, W, 2) and tap_bwd_ok(c, H, W) and H * W >= UP2W_MIN_PIXELS
                    and L.query("ladder_conv3x3_up2_wgrad_eligible", N, H, W, c.cin, c.cout))

    # forward: the resize in front of each block and the form of its conv
    n, fwd, front, (h, w) = len(blocks), [], up0, shape[1:3]
    for i, (conv, _, norm, rs) in enumerate(blocks):
        f, resize = factor(front, h, w), None
        if front is not None and (front.oh, front.ow) != (h, w):
            if not (f and fold_ok(conv, h, w, f)):
                resize = "materialise"
            elif not keep:
                resize = "fold_forward_only"
            elif virtual_ok(conv, h, w, f):
                resize = "virtual"
            elif i and up2 >= 2 and f == 2 and (blocks[i - 1][2] is None or blocks[i - 1][0].cout % 4 == 0):
                resize = "keep_both"        # (behind a norm: written by ladder_in_style_fwd_resize2x_keep; the 1x1 -> 2x2 resize in front of conv2d_1 never)
            else:
                resize = "materialise"
        lo_hw, (h, w) = (h, w), ((front.oh, front.ow) if front is not None else (h, w))
        # the last 3x3 conv feeds the 1x1 output conv directly (its resize is the identity)
        last = i == n - 1 and norm is None and (rs is None or (rs.oh, rs.ow) == (h, w))
        if resize in (None, "materialise"):
            form, one_launch = "plain", False
            proj = "rides" if (last and conv.cout <= 128 and conv._is_projection(conv_out) and conv.route((N, h, w, conv.cin)).halo) else None
        else:
            form = "projected" if proj_ok(conv, lo_hw[0], lo_hw[1], f) else "tapfold"
            one_launch = bool(form == "projected" and f == 2 and ctx.fuse_fwd and L.query(
                "ladder_up2proj_fused_eligible" if ctx.fuse_fwd >= 2 else "ladder_up2proj_fused_preferred", N, lo_hw[0], lo_hw[1], conv.cin, conv.cout))
            # (the fused 1x1 epilogues hold one pixel's 128 channels in a half-wave)
            proj = None if not (last and f == 2) else "rides" if (conv.cout == 128 and conv._is_projection(conv_out)) else "follows"
        fwd.append((resize, f, form, one_launch, proj, lo_hw, (h, w), last))
        front = rs
    # the tail of each block (norm, resize behind) and the backward pass, from the last block down
    plan, above_lowres, above_lgate = [None] * n, False, False
    for i in range(n - 1, -1, -1):
        conv, _, norm, rs = blocks[i]
        resize, f, form, one_launch, proj, (lh, lw), (ho, wo), last = fwd[i]        # (lh x lw: the map in front of the resize; ho x wo: the conv's)
        if i + 1 < n:
            behind, fb = fwd[i + 1][0], fwd[i + 1][1]
        else:
            behind, fb = ("materialise" if rs is not None and (rs.oh, rs.ow) != (ho, wo) else None), factor(rs, ho, wo)
        norm_out = None if norm is None else "both" if behind == "keep_both" else \
            "resized" if (behind == "materialise" and fb == 2 and conv.cout % 4 == 0) else "lowres"
        # a kept upsample: the low-resolution backward-data only for the last block or at `upsample_fused_convs` >= 3
        lowres_dx = bool(keep and (resize == "virtual" or (
            resize in ("materialise", "keep_both") and i and f == 2 and (i == n - 1 or up2 >= 3) and tap_bwd_ok(conv, lh, lw))))
        below = blocks[i - 1] if i else None
        # OFF by default (LADDER_ENABLE_LOWRES_GATE=1): measured in round 5, the gate loads in the epilogue of conv2d_6's fused backward-data cost 72 us
        # (1 631 -> 1 703 us), on the projected form's dense kernel 772 against 655 us -- more than the 67 / ~85 us ladder_act_bwd pass they replace
        lgate = bool(lowres_dx and below is not None and below[2] is None and below[0].act is not None and gate_sw and (
            (resize == "virtual" and form == "projected")
            or (ns == 0 and L.query("ladder_conv3x3_up2_bwd_data_gated_f32_eligible", N, lh, lw, conv.cout, conv.cin))))
        fuse_last = bool(last and conv.act is not None)
        proj_grad = bool(keep and fuse_last and ctx.fuse_bwd_proj and resize == "virtual" and form == "projected" and f == 2
                         and conv.act in ("leaky_relu", "relu") and conv_out.k == 1 and conv_out.stride == 1 and conv_out.act is None
                         and conv_out.cin == conv.cout and L.query("ladder_up2proj_bwd_combine_proj_eligible", N, lh, lw, conv.cout, conv_out.cout))
        rs_bwd = bool(behind in ("materialise", "keep_both") and not above_lowres)
        gated = bool(rs_bwd and norm is None and conv.act is not None and not fuse_last and fb == 2)
        plan[i] = PairPlan(resize, f, form, one_launch, proj, norm_out, behind, lowres_dx, lgate, above_lgate, gated, rs_bwd, fuse_last, proj_grad)
        above_lowres, above_lgate = lowres_dx, lgate
    cache[key] = plan
    return plan


class Dense:
    """tf.layers.dense, W [in,out]; MFMA-f32 GEMM with bias + activation epilogue."""

    def __init__(self, ctx, ps, name, cin, cout, act=None):
        self.ctx, self.ps, self.name, self.cin, self.cout, self.act = ctx, ps, name, cin, cout, act

    _plan = staticmethod(functools.lru_cache(maxsize=None)(_igemm_plan))      # (no switch enters the plan of a dense GEMM)

    def _igemm(self, name, M, K, Cout, *args):
        """Implicit-GEMM call [M, K] . [K, Cout] (dense fwd / bwd_data): appends the split-K workspace and the stream."""
        nb, kid = self._plan(M, K, Cout, K)
        _timed(kid, 2.0 * M * K * Cout, name, args + self.ctx.ws(nb) + (self.ctx.stream,))

    def _small(self, M):
        """Batch-sized layer: the one-launch kernels of csrc/densesplit.hip (strict fp32 MFMA when matmul_precision is "f32", else bf16x6)."""
        return bool(L.query("ladder_dense_small_eligible", M, self.cin, self.cout))

    def forward(self, x):
        M = x.shape[0]
        y = self.ctx.empty(M, self.cout)
        if self._small(M):
            L.call("ladder_dense_fwd_small" + self.ctx.sfx, _p(x), _p(self.ps.w[self.name + "/kernel"]), _p(self.ps.w[self.name + "/bias"]), _p(y),
                   M, self.cin, self.cout, L.ACT[self.act], self.ctx.stream)
        else:
            self._igemm("ladder_dense_fwd", M, self.cin, self.cout, _p(x), _p(self.ps.w[self.name + "/kernel"]), _p(self.ps.w[self.name + "/bias"]), _p(y),
                        M, self.cin, self.cout, L.ACT[self.act])
        self.x, self.y = x, y
        return y

    def backward(self, dy, need_dx=True, wgrad=True, act_done=False, gate_prev=None):
        x, y, st = self.x, self.y, self.ctx.stream
        M = x.shape[0]
        if self.act is not None and not act_done:
            L.call("ladder_act_bwd", _p(dy), _p(y), _p(dy), dy.numel(), L.ACT[self.act], st)
        if self._small(M):
            if wgrad and need_dx:                               # both gradient GEMMs in one launch
                dx = self.ctx.empty(M, self.cin)
                L.call("ladder_dense_bwd_small" + self.ctx.sfx, _p(x), _p(dy), _p(self.ps.w[self.name + "/kernel"]), _p(dx),
                       _p(self.ps.g[self.name + "/kernel"]), _p(self.ps.g[self.name + "/bias"]), M, self.cin, self.cout,
                       _p(x) if gate_prev else None, L.ACT[gate_prev] if gate_prev else 0, st)
                self.x = self.y = None
                return dx
            if wgrad:
                L.call("ladder_dense_bwd_weight_small" + self.ctx.sfx, _p(x), _p(dy), _p(self.ps.g[self.name + "/kernel"]),
                       _p(self.ps.g[self.name + "/bias"]), M, self.cin, self.cout, st)
            dx = None
            if need_dx:
                dx = self.ctx.empty(M, self.cin)
                L.call("ladder_dense_bwd_data_small" + self.ctx.sfx, _p(dy), _p(self.ps.w[self.name + "/kernel"]), _p(dx), M, self.cin, self.cout,
                       _p(x) if gate_prev else None, L.ACT[gate_prev] if gate_prev else 0, st)
            self.x = self.y = None
            return dx
        if wgrad:
            nb = L.query("ladder_dense_bwd_weight_workspace_bytes", M, self.cin, self.cout)
            wsp, wsn = self.ctx.ws(nb)
            L.call("ladder_dense_bwd_weight", _p(x), _p(dy), _p(self.ps.g[self.name + "/kernel"]),
                   _p(self.ps.g[self.name + "/bias"]), M, self.cin, self.cout, wsp, wsn, st)
        dx = None
        if need_dx:
            w = self.ps.w[self.name + "/kernel"]
            wT = self.ctx.empty(w.numel())
            L.call("ladder_filter_flip_transpose", _p(w), _p(wT), 1, 1, self.cin, self.cout, st)
            dx = self.ctx.empty(M, self.cin)
            self._igemm("ladder_dense_bwd_data", M, self.cout, self.cin, _p(dy), _p(wT), _p(dx), M, self.cin, self.cout,
                        _p(x) if gate_prev else None, L.ACT[gate_prev] if gate_prev else 0)
        self.x = self.y = None
        return dx


class BatchNormAct:
    """tf.layers.batch_normalization(training=True) + activation; statistics of the GLOBAL batch (C2)."""

    def __init__(self, ctx, ps, name, C, act):
        self.ctx, self.ps, self.name, self.C, self.act = ctx, ps, name, C, act

    def forward(self, x, sums=None, planes=(False, True)):
        """`sums`: the statistics record of x when its producer already computed it (conv epilogue: 2C doubles sum | sum of squares, then min | max),
        else a pass over x.  `planes` = (emit the fp16 plane images of y, also keep y in fp32): with the per-channel extremes max|y| is
        known before y is written, so the apply kernel can split it on the fly -- and when nothing needs the fp32 tensor it is never
        written (returns a PlanesOnly stand-in)."""
        C, ctx = self.C, self.ctx
        rows = x.numel() // C
        want_planes, need_fp32 = planes
        want_planes = bool(want_planes and ctx.ns == 4 and C % 4 == 0 and x.numel() % 8 == 0)
        if sums is None:
            nb = L.query("ladder_bn_workspace_bytes", rows, C)
            if want_planes:
                wsp, wsn = ctx.ws(2 * nb)
                sums = ctx.empty(6 * C)
                L.call("ladder_bn_fwd_stats_minmax", _p(x), _p(sums), rows, C, wsp, wsn, ctx.stream)
            else:
                wsp, wsn = ctx.ws(nb)
                sums = ctx.empty(4 * C)
                L.call("ladder_bn_fwd_stats", _p(x), _p(sums), rows, C, wsp, wsn, ctx.stream)
        # the statistics RECORD (csrc/norm.hip): 2C doubles = sum x | sum x^2 (the first 4C floats of the buffer), then optionally min | max as
        # 2C floats.  C2 all-reduces the doubles: E[x^2] - mean^2 in fp64 keeps the variance exact on channels far off zero (TF's fused batch
        # norm centres first, reference codes/models.py:398-460) -- 2 KB per layer instead of 1 KB.
        want_planes = want_planes and sums.numel() == 6 * C
        ctx.comm.allreduce_(sums[:4 * C].view(torch.float64), "C2 fwd " + self.name.split("/")[-1])   # (the extremes stay local: they bound THIS rank's tensor)
        self.count = float(rows) * ctx.comm.world
        self.mean_rstd = ctx.empty(2 * C)
        gam, bet = self.ps.w[self.name + "/gamma"], self.ps.w[self.name + "/beta"]
        if want_planes:
            y = torch.empty_like(x) if need_fp32 else None
            out = y if need_fp32 else PlanesOnly(x.shape)
            buf = torch.empty(L.query("ladder_presplit_bytes", x.numel(), ctx.ns), dtype=torch.uint8, device=ctx.device)
            y_amax = ctx.new_amax()
            L.call("ladder_bn_fwd_apply_planes", _p(x), _p(sums), self.count, _p(gam), _p(bet), _p(y), _p(buf), _p(self.mean_rstd), rows, C,
                   BN_EPS, L.ACT[self.act], _p(y_amax), ctx.stream)
            ctx.set_amax(out, y_amax)
            ctx.set_planes(out, buf)
            self.x = x
            return out
        y = torch.empty_like(x)
        y_amax = ctx.new_amax() if (ctx.ns == 4 and C % 4 == 0) else None
        L.call("ladder_bn_fwd_apply_absmax", _p(x), _p(sums), self.count, _p(gam), _p(bet), _p(y), _p(self.mean_rstd), rows, C, BN_EPS,
               L.ACT[self.act], _p(y_amax), ctx.stream)
        ctx.set_amax(y, y_amax)
        self.x = x
        return y

    def backward(self, dy, need_dx=True, wgrad=True):
        C, ctx, x = self.C, self.ctx, self.x
        rows = x.numel() // C
        gam, bet = self.ps.w[self.name + "/gamma"], self.ps.w[self.name + "/beta"]
        nb = L.query("ladder_bn_workspace_bytes", rows, C)
        wsp, wsn = ctx.ws(nb)
        dsums = ctx.empty(2 * C)
        L.call("ladder_bn_bwd_stats", _p(dy), _p(x), _p(self.mean_rstd), _p(gam), _p(bet), _p(dsums), rows, C,
               L.ACT[self.act], wsp, wsn, ctx.stream)
        ctx.comm.allreduce_(dsums, "C2 bwd " + self.name.split("/")[-1])
        dx = torch.empty_like(x) if need_dx else None
        # dgamma/dbeta are global sums already: written on every rank, the group all-reduce must not re-sum
        # them -> the engine divides BN parameter grads by world size before the flat all-reduce.
        dx_amax = ctx.new_amax() if (need_dx and ctx.ns == 4 and C % 4 == 0) else None
        L.call("ladder_bn_bwd_apply_absmax", _p(dy), _p(x), _p(self.mean_rstd), _p(gam), _p(bet), _p(dsums), self.count, _p(dx),
               _p(self.ps.g[self.name + "/gamma"]) if wgrad else None, _p(self.ps.g[self.name + "/beta"]) if wgrad else None,
               rows, C, L.ACT[self.act], _p(dx_amax), ctx.stream)
        if dx is not None:
            ctx.set_amax(dx, dx_amax)
        if wgrad and ctx.comm.world > 1:
            for t in (self.ps.g[self.name + "/gamma"], self.ps.g[self.name + "/beta"]):
                L.call("ladder_axpy", _p(t), _p(t), t.numel(), 1.0 / ctx.comm.world, 0, ctx.stream)
        self.x = None
        return dx


class InstanceNormStyleAct:
    """instance_norm(center=False, scale=False) -> style_mod -> activation (models.py:522-528 ..., modules.py:6-10)."""

    def __init__(self, ctx, C, act):
        self.ctx, self.C, self.act = ctx, C, act

    def forward(self, x, style):
        N, H, W, C = x.shape
        y = torch.empty_like(x)
        self.mean_rstd = self.ctx.empty(N, 2 * C)
        wsp, wsn = self.ctx.ws(L.query("ladder_in_style_workspace_bytes", N, H * W, C))
        y_amax = self.ctx.new_amax() if (self.ctx.ns == 4 and C % 4 == 0) else None
        L.call("ladder_in_style_fwd_absmax", _p(x), _p(style), _p(y), _p(self.mean_rstd), N, H * W, C, IN_EPS, L.ACT[self.act],
               wsp, wsn, _p(y_amax), self.ctx.stream)
        self.ctx.set_amax(y, y_amax)
        self.x, self.style = x, style
        return y

    def forward_resized(self, x, style, rs, keep_lowres=False):
        """forward() followed by the factor-2 resize `rs` in ONE pass over x (ladder_in_style_fwd_resize2x; C a multiple of 4): the normalised
        tensor is never written -- unless `keep_lowres` (the input of an upsample-fused convolution behind the resize).  Returns (resized tensor,
        normalised tensor or None).  The backward passes are those of the two separate layers."""
        N, H, W, C = x.shape
        up, y_lo = self.ctx.empty(N, 2 * H, 2 * W, C), None
        self.mean_rstd = self.ctx.empty(N, 2 * C)
        wsp, wsn = self.ctx.ws(L.query("ladder_in_style_workspace_bytes", N, H * W, C))
        up_amax = self.ctx.new_amax() if self.ctx.ns == 4 else None
        if keep_lowres:
            y_lo = self.ctx.empty(N, H, W, C)
            L.call("ladder_in_style_fwd_resize2x_keep", _p(x), _p(style), _p(up), _p(y_lo), _p(self.mean_rstd), N, H, W, C, IN_EPS,
                   L.ACT[self.act], wsp, wsn, _p(up_amax), self.ctx.stream)
            self.ctx.set_amax(y_lo, up_amax)                   # max |y| = max |up| (the record receives max |y|)
        else:
            L.call("ladder_in_style_fwd_resize2x", _p(x), _p(style), _p(up), _p(self.mean_rstd), N, H, W, C, IN_EPS, L.ACT[self.act], wsp, wsn,
                   _p(up_amax), self.ctx.stream)
        self.ctx.set_amax(up, up_amax)
        self.x, self.style = x, style
        rs.in_shape = (N, H, W, C)                             # (this pass stands in for rs.forward: rs.backward is the transpose of it)
        return up, y_lo

    def backward(self, dy):
        x = self.x
        N, H, W, C = x.shape
        dx = torch.empty_like(x)
        dstyle = self.ctx.empty(N, 2 * C)
        wsp, wsn = self.ctx.ws(L.query("ladder_in_style_workspace_bytes", N, H * W, C))
        dx_amax = self.ctx.new_amax() if (self.ctx.ns == 4 and C % 4 == 0) else None
        L.call("ladder_in_style_bwd_absmax", _p(dy), _p(x), _p(self.style), _p(self.mean_rstd), _p(dx), _p(dstyle), N, H * W, C,
               L.ACT[self.act], wsp, wsn, _p(dx_amax), self.ctx.stream)
        self.ctx.set_amax(dx, dx_amax)
        self.x = self.style = None
        return dx, dstyle


class Resize:
    """tf.image.resize_images TF1-legacy bilinear."""

    def __init__(self, ctx, oh, ow):
        self.ctx, self.oh, self.ow = ctx, oh, ow

    def forward(self, x):
        N, H, W, C = x.shape
        self.in_shape = (N, H, W, C)
        if (H, W) == (self.oh, self.ow):
            return x
        y = self.ctx.empty(N, self.oh, self.ow, C)
        L.call("ladder_resize_bilinear_fwd", _p(x), _p(y), N, H, W, C, self.oh, self.ow, self.ctx.stream)
        self.ctx.set_amax(y, self.ctx.known_amax(x))        # bilinear interpolation is a convex combination: max|y| <= max|x|
        return y

    def backward(self, dy, gate=None):
        """`gate` = (y, act) of the layer that produced the resized tensor: its activation backward is applied to dx in the same pass
        (factor-2 resizes; returns (dx, True) then, so that the caller skips that layer's own activation backward)."""
        N, H, W, C = self.in_shape
        if (H, W) == (self.oh, self.ow):
            return (dy, False) if gate is not None else dy
        dx = self.ctx.empty(N, H, W, C)
        if gate is not None and (self.oh, self.ow) == (2 * H, 2 * W) and gate[1] is not None:
            L.call("ladder_resize_bilinear_bwd_gated", _p(dy), _p(dx), N, H, W, C, self.oh, self.ow, _p(gate[0]), L.ACT[gate[1]],
                   self.ctx.stream)
            return dx, True                                     # (no absmax record: the gate rescales elements)
        L.call("ladder_resize_bilinear_bwd", _p(dy), _p(dx), N, H, W, C, self.oh, self.ow, self.ctx.stream)
        rec = self.ctx.known_amax(dy)
        if rec is not None:      # the transpose sums interpolation weights: column sums are bounded per axis (arch.resize_transpose_gain)
            self.ctx.set_amax(dx, rec * float(arch.resize_transpose_gain(H, self.oh) * arch.resize_transpose_gain(W, self.ow)))
        return (dx, False) if gate is not None else dx


class DepthToSpace:
    def __init__(self, ctx, r):
        self.ctx, self.r = ctx, r

    def forward(self, x):
        N, H, W, C = x.shape
        r = self.r
        y = self.ctx.empty(N, H * r, W * r, C // (r * r))
        L.call("ladder_depth_to_space", _p(x), _p(y), N, H, W, C, r, 0, self.ctx.stream)
        return y

    def backward(self, dy):
        N, HR, WR, Cp = dy.shape
        r = self.r
        dx = self.ctx.empty(N, HR // r, WR // r, Cp * r * r)
        L.call("ladder_depth_to_space", _p(dy), _p(dx), N, HR // r, WR // r, Cp * r * r, r, 1, self.ctx.stream)
        return dx


def pad_symmetric(ctx, x, p):
    N, H, W, C = x.shape
    y = ctx.empty(N, H + 2 * p, W + 2 * p, C)
    L.call("ladder_pad_symmetric", _p(x), _p(y), N, H, W, C, p, ctx.stream)
    return y


def add_(ctx, out, inp):
    L.call("ladder_axpy", _p(inp), _p(out), out.numel(), 1.0, 1, ctx.stream)
    ctx.drop_amax(out)                       # values changed in place: a registered absolute-maximum record no longer bounds them
    return out
