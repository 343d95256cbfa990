"""Shared by tests/test_norm_cases_cpu.py and tests/test_gpu_norm_matrix.py: the case table of the HBM-bound passes of csrc/norm.hip (batch-norm and
instance-norm statistics and apply passes, the two column-statistics stages, legacy bilinear resize, depth-to-space, symmetric pad, activation backward),
what each row reaches (`features`: pure arithmetic on the tuple -- a port of the host decisions ew_grid, stats_nblk / rows_per_blk, in_split, vec4_ok /
in_vec_ok, the fold condition, pgrad_rides, bpr and the `fixed` predicate, which the CPU test holds against the library's two workspace queries), the
float64 references -- the oracle's batch_norm_train, instance_norm + style_mod + leaky_relu, resize_bilinear_legacy, depth_to_space, pad_symmetric, act
and autograd, formed as tests/test_gpu_kernels.py forms them -- and a runner that launches the public entry points on guard-banded buffers: outputs start
as NaN, workspaces as 0xFF bytes, every band is compared bitwise after the launches and every output must be finite.

A row is a plain tuple, (entry, shape..., flags...):

  ("bn", rows, C, act, variant)      batch norm forward + backward against the oracle.  variant: plain | absmax (the _absmax entries, record exact) |
                                     shift_x | shift_y (that tensor -- and dx with y -- starts one float past a 16-byte boundary) | pgrad_only (dx == NULL)
                                     | planes (ladder_bn_fwd_stats_minmax + ladder_bn_fwd_apply_planes)
  ("refuse", what)                   a documented refusal: the code, and no output written
  ("colstats", rows, C, shift)       ladder_bn_fwd_stats, ladder_bn_fwd_stats_minmax (C % 4 == 0, aligned), ladder_bn_bwd_stats
  ("stage2", minmax, nblk, C)        ladder_bn_stats_from_partials / ladder_bn_stats_minmax_from_partials on synthetic partials
  ("in", N, H, W, C, data)           instance norm + style + leaky, forward + backward: workspace route, ws == NULL route, x-shifted route; the fused
                                     resize2x_keep where C % 4 == 0.  data: off (means +-50 sd) | off_corner (... and pixel (0, 0) zeroed) | absmax (off, and the
                                     _absmax entries with exact records)
  ("resize", N, H, W, C, OH, OW, shift)
  ("d2s", N, H, W, C, r, shift)
  ("pad", N, H, W, C, p)
  ("act_bwd", n, act)

THE METRIC of the normalisation rows is per channel: the largest error of a channel over that channel's largest |reference| (tests/test_gpu_kernels.py
divides by the tensor's largest value, under which a channel with a small gamma may be wrong by orders of magnitude).  The bars are the ones the project
states for these kernels (y 1e-5; dx 2e-5 batch norm, 5e-5 instance norm; dgamma / dbeta / dstyle 2e-5 of their own vector's scale).  Nobody had measured
the kernels in that metric, so every row also evaluates an fp32 numpy restatement of the same formulas (mean and 1 / sd rounded to fp32, the expression of
csrc/norm_util.h) against float64 in the same metric: where the restatement alone exceeds a quarter of a bar, that row's bar is four times the
restatement's error (summation order, fused multiply-adds).  No bar is derived from a kernel's output.

Leaky masks: a pre-activation within fp32 rounding of zero may legitimately fall on the other side in float64 (each flip moves dx by O(1), see
test_conv2d_fwd_bwd).  The norm kernels form the mask themselves, so it cannot be handed over from the oracle; instead the data keep every
pre-activation at least 1e-5 away from zero (`_clear_kinks`), forty times the rounding error of an O(1) pre-activation.  ladder_act_bwd takes the oracle's
output, as that test does."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from guarded import _Guarded, _NAN_BITS, _FF_BITS  # noqa: E402

E_SHAPE, E_ALIGN = -1, -2                            # LADDER_E_SHAPE, LADDER_E_ALIGN
ACT = {None: 0, "leaky_relu": 1, "relu": 2, "tanh": 3}           # (_lib.ACT without its alias)
BN_EPS, IN_EPS = 1e-3, 1e-6
BAR_Y, BAR_DX_BN, BAR_DX_IN, BAR_PARAM = 1e-5, 2e-5, 5e-5, 2e-5  # the project's stated bars (tests/test_gpu_kernels.py)
BAR_BWD_SUMS = 2e-5                                  # fp32 backward sums, of sum |term| per channel
BAR_COPY = 1e-6                                      # resize, pad backward (as tests/test_gpu_kernels.py)
ABSMAX_FLOATS = 512

# ---------------------------------------------------------------------------------------------------------------------------------- the table
_BN_SHAPES = [(33000, 96), (30000, 100), (40000, 64), (60000, 10)]           # two sweeps: float4 !fixed; the same with idle lanes; fixed / fold; scalar
BN_ROWS = ([("bn", r, c, a, "plain") for r, c in _BN_SHAPES for a in ("leaky_relu", None)]
           + [("bn", 40000, 64, "leaky_relu", "absmax"), ("bn", 40000, 64, "leaky_relu", "pgrad_only"),
              ("bn", 9000, 64, "leaky_relu", "shift_x"), ("bn", 9000, 64, None, "shift_y"),
              ("bn", 33000, 96, "leaky_relu", "planes"),
              ("bn", 100, 96, "leaky_relu", "plain"), ("bn", 77, 10, None, "plain")])       # one sweep: float4 (!fixed), scalar
REFUSE_ROWS = [("refuse", w) for w in ("record_on_scalar_route", "minmax_misaligned_x", "minmax_planes_c_not_4", "planes_n_not_8")]
COLSTATS_ROWS = ([("colstats", r, 8, 0) for r in (1, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 2049)]
                 + [("colstats", r, 3, 0) for r in (1, 3, 4, 5, 31, 32, 33, 1025)]
                 + [("colstats", 525288, 4, 0), ("colstats", 525288, 3, 0), ("colstats", 129, 8, 1)])
STAGE2_NBLK = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023)
STAGE2_C = (1, 3, 16, 100)
STAGE2_ROWS = [("stage2", m, nb, c) for m in (0, 1) for nb in STAGE2_NBLK for c in STAGE2_C]
IN_ROWS = [("in", 2, 16, 16, 32, "off"), ("in", 2, 16, 16, 32, "off_corner"), ("in", 2, 3, 5, 8, "off"), ("in", 1, 17, 241, 4, "off"),
           ("in", 1, 65, 63, 4, "off"), ("in", 1024, 16, 16, 4, "off"), ("in", 3, 16, 16, 72, "absmax"), ("in", 2, 5, 5, 10, "off")]
RESIZE_ROWS = [("resize", 2, 3, 5, 8, 6, 20, 0), ("resize", 1, 4, 2, 3, 12, 2, 0), ("resize", 1, 2, 8, 160, 4, 16, 0), ("resize", 1, 2, 90, 3, 4, 180, 0),
               ("resize", 2, 3, 5, 8, 6, 10, 1), ("resize", 1, 2, 90, 3, 6, 180, 0)]       # (the last: bpr = 2 in the general transpose)
D2S_ROWS = [("d2s", 2, 3, 5, 4, 2, 0), ("d2s", 1, 2, 40, 64, 2, 0), ("d2s", 1, 2, 40, 64, 2, 1)]
PAD_ROWS = [("pad", 2, 5, 7, 3, 0), ("pad", 2, 5, 7, 3, 1), ("pad", 2, 5, 7, 3, 5), ("pad", 8, 126, 126, 5, 1), ("pad", 8, 128, 130, 5, 2)]
ACT_BWD_N = (1, 2, 3, 4, 5, 7, 1024, 2097152 + 7)
ACT_BWD_ROWS = [("act_bwd", n, a) for n in ACT_BWD_N for a in (None, "leaky_relu", "relu", "tanh")]

CASES = BN_ROWS + REFUSE_ROWS + COLSTATS_ROWS + STAGE2_ROWS + IN_ROWS + RESIZE_ROWS + D2S_ROWS + PAD_ROWS + ACT_BWD_ROWS
MAX_ELEMS = 4 << 20                                   # per tensor of a row: the float64 references stay cheap on the host


def case_id(row):
    return "-".join("none" if v is None else str(v) for v in row)


# ------------------------------------------------------------------------------------------------------- host decisions of csrc/norm.hip, ported
def ew_grid(items):
    return max(1, min((items + 255) // 256, 256 * 8))


def sweeps(items):
    """Iterations of the grid-stride loop in thread 0 of workgroup 0 over `items` work items (0: it never enters)."""
    return -(-items // (ew_grid(items) * 256))


def stats_nblk(rows):
    return max(1, min((rows + 1023) // 1024, 512))


def rows_per_blk(rows):
    return -(-rows // stats_nblk(rows))


def in_split(N, HW, C):
    groups = N * ((C + 63) // 64)
    return max(1, min((2048 + groups - 1) // groups, (HW + 63) // 64))


def stage1_loops(rows, V):
    """colstats_stage1<Row, V>: which of the batched 8-row loop and its one-row tail run, over every row lane of every block."""
    RL = 16 if V == 4 else 4
    nblk, per = stats_nblk(rows), rows_per_blk(rows)
    lens = sorted({max(0, min(rows, (b + 1) * per) - b * per) for b in range(nblk)})
    batch = tail = both = tail_only = False
    for n in lens:
        for rl in range(RL):
            r, nb = rl, 0
            while r + 7 * RL < n:
                r, nb = r + 8 * RL, nb + 1
            nt = -(-(n - r) // RL) if r < n else 0
            batch, tail, both, tail_only = batch or nb > 0, tail or nt > 0, both or (nb > 0 and nt > 0), tail_only or (nb == 0 and nt > 0)
    return dict(nblk=nblk, per=per, last=rows - (nblk - 1) * per, batch=batch, tail=tail, both=both, tail_only=tail_only, idle_lane=rows < RL)


def stage2_loops(RL, NACC, nblk):
    """colstats_stage2<CL, RL, NACC>: iterations of the NACC-wide loop and of the remainder loop (leftover strides), as sets over the row lanes."""
    main, left = set(), set()
    for rl in range(RL):
        b = rl
        m = k = 0
        while b + (NACC - 1) * RL < nblk:
            b, m = b + NACC * RL, m + 1
        if NACC > 1:
            while b < nblk:
                b, k = b + RL, k + 1
        main.add(m)
        left.add(k)
    return dict(main=main, left=left, side=(nblk > RL) - (nblk < RL))


def _stage2_of_stage1(nblk):
    return "colstats_stage2<64,16,1>", stage2_loops(16, 1, nblk)


def features(row):
    """What the row reaches: `kernels` (the set of kernels launched, with their template arguments) and the loop / route facts the CPU test asserts."""
    e = row[0]
    if e == "bn":
        _, rows, C, act, var = row
        n = rows * C
        x_al, y_al, rec, has_dx = var != "shift_x", var != "shift_y", var == "absmax", var != "pgrad_only"
        v4f = C % 4 == 0 and x_al and y_al
        fixed = (ew_grid(n // 4) * 256 * 4) % C == 0
        fold = v4f and not rec and fixed and var != "planes"
        vs = 4 if (C % 4 == 0 and x_al) else 1                  # both statistics passes: vec4_ok(C, x) / vec4_ok(C, x, dy), dy aligned
        k = {"colstats_stage2<64,16,1>", "colstats_stage1<BnBwdRow,%d>" % vs}
        if var == "planes":
            assert v4f and n % 8 == 0
            k |= {"colstats_stage1<MomentsRow<true>,4>", "bn_finalize_minmax_kernel", "bn_apply_planes_kernel"}
        else:
            k |= {"colstats_stage1<MomentsRow<false>,%d>" % vs}
            k |= {"bn_apply_fin_kernel"} if fold else {"bn_finalize_kernel", "bn_apply_kernel" if v4f else "bn_apply_scalar_kernel"}
        v4b = has_dx and v4f
        rides = v4b and not rec
        if not rides:
            k.add("bn_param_grad_kernel")
        if has_dx:
            k.add("bn_bwd_apply_v4_kernel" if v4b else "bn_bwd_apply_kernel")
        return dict(kernels=k, elems=n, v4_fwd=v4f, v4_bwd=v4b, fixed=fixed, fold=fold, pgrad_rides=rides, has_dx=has_dx, record=rec,
                    sweeps_fwd=sweeps(n // 4 if v4f else n), sweeps_bwd=(sweeps(n // 4 if v4b else n) if has_dx else 0),
                    idle_lanes=(-C) % 64, nblk=stats_nblk(rows), shifted=not (x_al and y_al), c4=C % 4 == 0)
    if e == "refuse":
        return dict(kernels=set(), elems=0)
    if e == "colstats":
        _, rows, C, shift = row
        V = 4 if (C % 4 == 0 and not shift) else 1
        f = stage1_loops(rows, V)
        name, s2 = _stage2_of_stage1(f["nblk"])
        k = {"colstats_stage1<MomentsRow<false>,%d>" % V, "colstats_stage1<BnBwdRow,%d>" % V, name}
        minmax = C % 4 == 0 and not shift
        if minmax:
            k.add("colstats_stage1<MomentsRow<true>,4>")
        f.update(kernels=k, elems=rows * C, V=V, minmax=minmax, stage2=s2, shifted=bool(shift), c4=C % 4 == 0, idle_lanes=(-C) % 64)
        return f
    if e == "stage2":
        _, minmax, nblk, C = row
        RL, NACC = (64, 4) if minmax else (16, 1)
        return dict(kernels={"colstats_stage2<16,%d,%d>" % (RL, NACC)}, elems=nblk * (4 if minmax else 2) * C, stage2=stage2_loops(RL, NACC, nblk),
                    dead_columns=(-(4 if minmax else 2) * C) % 16, RL=RL)
    if e == "in":
        _, N, H, W, C, data = row
        HW = H * W
        sp = in_split(N, HW, C)
        per = -(-HW // sp)
        k = {"in_style_fwd_kernel", "in_style_bwd_kernel"}                    # the ws == NULL and the x-shifted routes of every row
        vec = C % 4 == 0
        if vec:
            k |= {"in_stats_kernel", "in_finalize_kernel", "in_apply_kernel", "in_bwd_stats_kernel", "in_bwd_finalize_kernel", "in_bwd_apply_kernel",
                  "in_apply_resize2x_kernel"}
        groups = N * ((C + 63) // 64)
        return dict(kernels=k, elems=N * HW * C * (4 if vec else 1), vec=vec, split=sp, per=per, last_split=HW - (sp - 1) * per, HW=HW,
                    pivots=min(16, HW), split_limit="hw" if (2048 + groups - 1) // groups > (HW + 63) // 64 else "groups",
                    idle_quads=((-C) % 64) // 4 if vec else 0, record=data == "absmax", square=H == W, ws_bytes=N * sp * 2 * C * 4, shifted=True)
    if e == "resize":
        _, N, H, W, C, OH, OW, shift = row
        v4 = C % 4 == 0 and not shift
        V, CV = (4, C // 4) if v4 else (1, C)
        bpr = (W * CV + 255) // 256
        fy, fx = OH // H, OW // W
        x2 = (fy, fx) == (2, 2)
        k = {"resize_fwd_kernel<%d>" % V, ("resize_bwd_x2_kernel<%d>" if x2 else "resize_bwd_kernel<%d>") % V}
        return dict(kernels=k, elems=N * OH * OW * C, V=V, bpr=bpr, fy=fy, fx=fx, x2=x2, gated=x2, ragged=(W * CV) % 256 != 0, shifted=bool(shift),
                    c4=C % 4 == 0, grid=bpr * N * H)
    if e == "d2s":
        _, N, H, W, C, r, shift = row
        seg = C // r
        v4 = seg % 4 == 0 and not shift
        per_row = W * seg // (4 if v4 else 1)
        return dict(kernels={"d2s_kernel<%d>" % (4 if v4 else 1)}, elems=N * H * W * C, seg=seg, V=4 if v4 else 1, bpr=(per_row + 255) // 256,
                    shifted=bool(shift), seg4=seg % 4 == 0)
    if e == "pad":
        _, N, H, W, C, p = row
        out = N * (H + 2 * p) * (W + 2 * p) * C
        return dict(kernels={"pad_sym_kernel", "pad_sym_bwd_kernel"}, elems=out, sweeps_fwd=sweeps(out), sweeps_bwd=sweeps(N * H * W * C), p=p, H=H, W=W)
    if e == "act_bwd":
        _, n, act = row
        grid = ew_grid(n // 4 + 1)
        return dict(kernels={"act_bwd_kernel"}, elems=n, sweeps4=-(-(n // 4) // (grid * 256)), tail=n % 4)
    raise ValueError(row)


# ----------------------------------------------------------------------------------------------------------------------------- metric and bars
def chan_err(got, ref):
    """Largest error of a channel (the last axis) over that channel's largest |reference|, maximised over the channels."""
    C = ref.shape[-1]
    g, r = np.asarray(got, np.float64).reshape(-1, C), np.asarray(ref, np.float64).reshape(-1, C)
    return float((np.abs(g - r).max(0) / np.maximum(np.abs(r).max(0), 1e-300)).max())


def vec_err(got, ref):
    r = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64).reshape(r.shape) - r).max() / max(np.abs(r).max(), 1e-300))


def row_bar(stated, restatement_err):
    """The project's stated bar, unless the fp32 restatement alone uses more than a quarter of it: then four times the restatement's error."""
    return stated if restatement_err <= 0.25 * stated else 4.0 * restatement_err


def _seed(row):
    return int.from_bytes(case_id(row).encode(), "little") % (2 ** 63)


def _colsum32(a):
    """fp32 column sums of [rows, C], pairwise (numpy's reduction along a contiguous axis)."""
    return np.ascontiguousarray(a.T).sum(axis=1, dtype=np.float32)


def _leaky_grad(pre, act):
    if act == "leaky_relu":
        return np.where(pre > 0, 1.0, 0.2).astype(pre.dtype)
    if act == "relu":
        return np.where(pre > 0, 1.0, 0.0).astype(pre.dtype)
    assert act is None
    return np.ones_like(pre)


KINK_MARGIN = 1e-5


def _clear_kinks(x, pre_of, sd, scale, act):
    """Move the elements whose float64 pre-activation lies within 3e-5 of zero by 1e-3 sd of their channel, away from zero (|scale| >= 0.1), until none
    lies within KINK_MARGIN: no leaky / relu mask then depends on fp32 rounding."""
    if act is None:
        return x
    for _ in range(8):
        pre = pre_of(x)
        bad = np.abs(pre) < 3e-5
        if not bad.any():
            break
        x = np.where(bad, x + np.float32(1e-3) * np.broadcast_to(sd, x.shape).astype(np.float32) * np.where((pre >= 0) == (scale > 0), 1, -1), x).astype(np.float32)
    assert np.abs(pre_of(x)).min() > KINK_MARGIN
    return x


def _gammas(rng, C):
    g = 1 + 0.3 * rng.standard_normal(C)
    g = np.where(np.abs(g) < 0.1, 0.1, g) * np.where(rng.random(C) < 0.25, -1.0, 1.0)
    g[0] = 0.1                                        # a small gamma: invisible under a per-tensor scale
    if C > 1:
        g[1] = -0.1
    return g.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------- batch-norm reference
@functools.lru_cache(maxsize=1)                       # the variants of a shape are neighbours in the table and share data and reference (never modified)
def bn_reference(rows, C, act):
    import torch
    from oracle import ladder_oracle as O
    rng = np.random.default_rng(rows * 1009 + C * 17 + ACT[act])
    sd = 0.5 + rng.random(C)
    mean = sd * rng.standard_normal(C)
    x = (rng.standard_normal((rows, C)) * sd + mean).astype(np.float32)
    g, be = _gammas(rng, C), (0.2 * rng.standard_normal(C)).astype(np.float32)
    dy = rng.standard_normal((rows, C)).astype(np.float32)

    def pre_of(xx):
        x64 = xx.astype(np.float64)
        return g * (x64 - x64.mean(0)) / np.sqrt(x64.var(0) + BN_EPS) + be
    x = _clear_kinks(x, pre_of, sd, g, act)
    xt, gt, bt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, g, be))
    yr = O.act(O.batch_norm_train(xt, gt, bt), act)
    yr.backward(torch.tensor(dy, dtype=torch.float64))
    ref = dict(y=yr.detach().numpy(), dx=xt.grad.numpy(), dgamma=gt.grad.numpy(), dbeta=bt.grad.numpy())
    # fp32 restatement: mean and 1 / sd rounded to fp32, the expression of csrc/norm_util.h
    x64 = x.astype(np.float64)
    mu, rs = x64.mean(0).astype(np.float32), (1.0 / np.sqrt(x64.var(0) + BN_EPS)).astype(np.float32)
    xh = (x - mu) * rs
    pre = g * xh + be
    y32 = np.where(pre > 0, pre, np.float32(0.2) * pre) if act == "leaky_relu" else pre
    dp = dy * _leaky_grad(pre, act)
    s1, s2 = _colsum32(dp), _colsum32(dp * xh)
    inv = np.float32(1.0 / rows)
    dx32 = (g * rs) * (dp - s1 * inv - xh * (s2 * inv))
    rest = dict(y=chan_err(y32, ref["y"]), dx=chan_err(dx32, ref["dx"]), dgamma=vec_err(s2, ref["dgamma"]), dbeta=vec_err(s1, ref["dbeta"]))
    for a in list(ref.values()) + [x, g, be, dy]:
        a.setflags(write=False)
    return dict(x=x, g=g, be=be, dy=dy, ref=ref, rest=rest)


def bn_bars(rest):
    return dict(y=row_bar(BAR_Y, rest["y"]), dx=row_bar(BAR_DX_BN, rest["dx"]), dgamma=row_bar(BAR_PARAM, rest["dgamma"]), dbeta=row_bar(BAR_PARAM, rest["dbeta"]))


# ---------------------------------------------------------------------------------------------------------------------- instance-norm reference
@functools.lru_cache(maxsize=1)
def in_reference(N, H, W, C, data):
    import torch
    from oracle import ladder_oracle as O
    rng = np.random.default_rng(N * 7919 + H * 1009 + W * 101 + C * 7 + (data == "off_corner"))
    sd = 0.5 + rng.random((N, 1, 1, C))
    mean = 50.0 * sd * np.where(rng.random((N, 1, 1, C)) < 0.5, -1.0, 1.0)              # the construction of test_batch_norm_far_off_centre_channels
    x = (rng.standard_normal((N, H, W, C)) * sd + mean).astype(np.float32)
    if data == "off_corner":
        x[:, 0, 0, :] = 0.0                           # the zero-padded corner of the producing convolution (csrc/norm.hip, in_pivot)
    sty = (0.5 * rng.standard_normal((N, 2 * C))).astype(np.float32)
    sc = sty[:, :C] + 1
    sty[:, :C] = np.where(np.abs(sc) < 0.1, 0.1, sc) - 1                               # |scale| >= 0.1
    dy = rng.standard_normal((N, H, W, C)).astype(np.float32)
    s0, s1 = (sty[:, :C].astype(np.float32) + np.float32(1)).reshape(N, 1, 1, C), sty[:, C:].reshape(N, 1, 1, C)

    def pre_of(xx):
        x64 = xx.astype(np.float64)
        return s0 * (x64 - x64.mean((1, 2), keepdims=True)) / np.sqrt(x64.var((1, 2), keepdims=True) + IN_EPS) + s1
    x = _clear_kinks(x, pre_of, sd, s0, "leaky_relu")
    xt, stt = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, sty))
    yr = O.leaky_relu(O.style_mod(O.instance_norm(xt), stt))
    yr.backward(torch.tensor(dy, dtype=torch.float64))
    ref = dict(y=yr.detach().numpy(), dx=xt.grad.numpy(), dstyle=stt.grad.numpy())
    if C % 4 == 0:
        ref["up"] = O.resize_bilinear_legacy(yr.detach(), 2 * H, 2 * W).numpy()
    x64 = x.astype(np.float64)
    mu = x64.mean((1, 2), keepdims=True).astype(np.float32)
    rs = (1.0 / np.sqrt(x64.var((1, 2), keepdims=True) + IN_EPS)).astype(np.float32)
    xh = (x - mu) * rs
    pre = s0 * xh + s1
    y32 = np.where(pre > 0, pre, np.float32(0.2) * pre)
    dp = dy * _leaky_grad(pre, "leaky_relu")
    a1 = np.stack([_colsum32(v.reshape(H * W, C)) for v in dp]).reshape(N, 1, 1, C)
    a0 = np.stack([_colsum32(v.reshape(H * W, C)) for v in dp * xh]).reshape(N, 1, 1, C)
    inv = np.float32(1.0 / (H * W))
    dx32 = (rs * s0) * (dp - a1 * inv - xh * (a0 * inv))
    rest = dict(y=chan_err(y32, ref["y"]), dx=chan_err(dx32, ref["dx"]), dstyle=vec_err(np.concatenate([a0.reshape(N, C), a1.reshape(N, C)], 1), ref["dstyle"]))
    for a in list(ref.values()) + [x, sty, dy]:
        a.setflags(write=False)
    return dict(x=x, sty=sty, dy=dy, ref=ref, rest=rest)


def in_bars(rest):
    return dict(y=row_bar(BAR_Y, rest["y"]), up=row_bar(BAR_Y, rest["y"]), dx=row_bar(BAR_DX_IN, rest["dx"]), dstyle=row_bar(BAR_PARAM, rest["dstyle"]))


# -------------------------------------------------------------------------------------------------------------------------------- the runner
class _Bufs:
    """The guarded device buffers of one row: inputs, NaN-filled outputs, 0xFF-filled workspaces; `check` compares every band."""

    def __init__(self):
        self.all = []

    def _new(self, n, fill, shift, what):
        g = _Guarded(n, fill, shift)
        self.all.append((what, g))
        return g

    def inp(self, a, what, shift=0):
        import torch
        a = np.ascontiguousarray(a, np.float32)
        g = self._new(a.size, 0, shift, what)
        g.t.copy_(torch.from_numpy(a.reshape(-1)))
        return g

    def out(self, n, what, shift=0):
        return self._new(n, _NAN_BITS, shift, what)

    def ws(self, nbytes, what):
        assert nbytes % 4 == 0
        return self._new(max(nbytes // 4, 4), _FF_BITS, 0, what)

    def check(self, after):
        import torch
        torch.cuda.synchronize()
        for what, g in self.all:
            assert g.guards_intact(), "%s: guard band overwritten (after %s)" % (what, after)


def _host(g, shape, what):
    """The interior of a guarded output on the host: bands intact, no NaN left (every output starts as NaN), every element finite."""
    assert g.guards_intact(), "%s: guard band overwritten" % what
    a = g.t.cpu().numpy().reshape(shape)
    assert not np.isnan(a).any(), "%s: NaN left (an element the kernel never wrote)" % what
    assert np.isfinite(a).all(), "%s: not finite" % what
    return a


def _host_record(g, C, what):
    """A statistics record on the host: 2C doubles (read as doubles: half a double may carry the bits of a float NaN) and, behind them, floats."""
    assert g.guards_intact(), "%s: guard band overwritten" % what
    a = g.t.cpu().numpy()
    d, rest = a[:4 * C].view(np.float64), a[4 * C:]
    assert not np.isnan(d).any() and not np.isnan(rest).any(), "%s: NaN left (an element the kernel never wrote)" % what
    assert np.isfinite(d).all() and np.isfinite(rest).all(), "%s: not finite" % what
    return d, rest


def _untouched(g):
    return g.guards_intact() and bool((g.bits[g.lo:g.lo + g.n] == _NAN_BITS).all().item())


def _p(g):
    return None if g is None else (g.t.data_ptr() if isinstance(g, _Guarded) else g.data_ptr())


def _recmax(rec):
    from test_gpu_split import recmax
    return recmax(rec.t)


def run_bn(L, row, st):
    """-> (errs, bars, restatement errors) of y, dx, dgamma, dbeta against the oracle."""
    import torch
    from test_gpu_split import presplit
    _, rows, C, act, var = row
    f = features(row)
    d = bn_reference(rows, C, act)
    ref, a, n = d["ref"], ACT[act], rows * C
    B = _Bufs()
    sx, sy = int(var == "shift_x"), int(var == "shift_y")
    x, dy, g, be = B.inp(d["x"], "x", sx), B.inp(d["dy"], "dy"), B.inp(d["g"], "gamma"), B.inp(d["be"], "beta")
    minmax = var == "planes"
    nblk = f["nblk"]
    wsb = L.query("ladder_bn_workspace_bytes", rows, C)
    assert wsb == nblk * 2 * C * 8
    ws = B.ws(nblk * C * 24 if minmax else wsb, "workspace")
    sums, mr, y = B.out(6 * C if minmax else 4 * C, "sums"), B.out(2 * C, "mean_rstd"), B.out(n, "y", sy)
    rec = B.out(ABSMAX_FLOATS, "record") if var in ("absmax", "planes") else None
    L.call("ladder_bn_fwd_stats_minmax" if minmax else "ladder_bn_fwd_stats", _p(x), _p(sums), rows, C, _p(ws), ws.n * 4, st)
    B.check("forward statistics")
    errs = {}
    if var == "planes":
        nb = L.query("ladder_presplit_bytes", n, 4)
        planes = B.ws(nb, "planes")
        L.call("ladder_bn_fwd_apply_planes", _p(x), _p(sums), float(rows), _p(g), _p(be), _p(y), _p(planes), _p(mr), rows, C, BN_EPS, a, _p(rec), st)
        B.check("apply with planes")
        yh = _host(y, (rows, C), "y")
        assert _recmax(rec) == float(np.abs(yh).max()), "record of max|y|"                 # (checked as test_bn_apply_emits_planes checks them)
        want = presplit(L, y.t, rec.t, 4, st)
        assert torch.equal(planes.t.view(torch.uint8)[:nb], want), "planes differ from ladder_presplit of y"
        planes2 = B.ws(nb, "planes (y == NULL)")
        L.call("ladder_bn_fwd_apply_planes", _p(x), _p(sums), float(rows), _p(g), _p(be), None, _p(planes2), _p(mr), rows, C, BN_EPS, a, _p(rec), st)
        B.check("apply with planes, y == NULL")
        assert torch.equal(planes2.t.view(torch.uint8)[:nb], want)
    elif var == "absmax":
        L.call("ladder_bn_fwd_apply_absmax", _p(x), _p(sums), float(rows), _p(g), _p(be), _p(y), _p(mr), rows, C, BN_EPS, a, _p(rec), st)
        B.check("apply with record")
        yh = _host(y, (rows, C), "y")
        assert _recmax(rec) == float(np.abs(yh).max()), "record of max|y|"
    else:
        L.call("ladder_bn_fwd_apply", _p(x), _p(sums), float(rows), _p(g), _p(be), _p(y), _p(mr), rows, C, BN_EPS, a, st)
        B.check("apply")
        yh = _host(y, (rows, C), "y")
    _host(mr, (2 * C,), "mean_rstd")
    errs["y"] = chan_err(yh, ref["y"])
    ds, dg, db = B.out(2 * C, "dsums"), B.out(C, "dgamma"), B.out(C, "dbeta")
    wsd = B.ws(nblk * 2 * C * 4, "backward workspace")
    L.call("ladder_bn_bwd_stats", _p(dy), _p(x), _p(mr), _p(g), _p(be), _p(ds), rows, C, a, _p(wsd), wsd.n * 4, st)
    B.check("backward statistics")
    dx = B.out(n, "dx", sy) if f["has_dx"] else None
    if var == "absmax":
        rec.bits[rec.lo:rec.lo + rec.n] = _NAN_BITS                                       # bn_param_grad_kernel must clear it
        L.call("ladder_bn_bwd_apply_absmax", _p(dy), _p(x), _p(mr), _p(g), _p(be), _p(ds), float(rows), _p(dx), _p(dg), _p(db), rows, C, a, _p(rec), st)
    else:
        L.call("ladder_bn_bwd_apply", _p(dy), _p(x), _p(mr), _p(g), _p(be), _p(ds), float(rows), _p(dx), _p(dg), _p(db), rows, C, a, st)
    B.check("backward apply")
    dgh, dbh = _host(dg, (C,), "dgamma"), _host(db, (C,), "dbeta")
    errs["dgamma"], errs["dbeta"] = vec_err(dgh, ref["dgamma"]), vec_err(dbh, ref["dbeta"])
    if f["has_dx"]:
        dxh = _host(dx, (rows, C), "dx")
        errs["dx"] = chan_err(dxh, ref["dx"])
        if var == "absmax":
            assert _recmax(rec) == float(np.abs(dxh).max()), "record of max|dx|"
    else:                                             # parameter gradients alone: the same bits as the call that also writes dx
        dx2, dg2, db2 = B.out(n, "dx (second call)"), B.out(C, "dgamma (second call)"), B.out(C, "dbeta (second call)")
        L.call("ladder_bn_bwd_apply", _p(dy), _p(x), _p(mr), _p(g), _p(be), _p(ds), float(rows), _p(dx2), _p(dg2), _p(db2), rows, C, a, st)
        B.check("backward apply with dx")
        assert np.array_equal(_host(dg2, (C,), "dgamma").view(np.int32), dgh.view(np.int32)) and np.array_equal(_host(db2, (C,), "dbeta").view(np.int32), dbh.view(np.int32))
        errs["dx"] = chan_err(_host(dx2, (rows, C), "dx"), ref["dx"])
    return errs, bn_bars(d["rest"]), d["rest"]


def run_refuse(L, row, st):
    """The documented refusals of the batch-norm entries: the documented code, and every output keeps its NaN bits."""
    import torch
    what = row[1]
    B = _Bufs()
    z = lambda n, s=0: B.inp(np.ones(n, np.float32), "input", s)  # noqa: E731
    if what == "record_on_scalar_route":
        for rows, C, sx in ((8, 10, 0), (8, 8, 1)):                                       # C % 4 != 0; a C % 4 == 0 tensor one float past the boundary
            n = rows * C
            x, y, mr, rec, dx, dg, db = z(n, sx), B.out(n, "y"), B.out(2 * C, "mean_rstd"), B.out(ABSMAX_FLOATS, "record"), B.out(n, "dx"), B.out(C, "dg"), B.out(C, "db")
            sums = B.inp(np.zeros(4 * C, np.float32), "sums")
            rc = L.query("ladder_bn_fwd_apply_absmax", _p(x), _p(sums), float(rows), _p(z(C)), _p(z(C)), _p(y), _p(mr), rows, C, BN_EPS, 1, _p(rec), st)
            rc2 = L.query("ladder_bn_bwd_apply_absmax", _p(z(n)), _p(x), _p(z(2 * C)), _p(z(C)), _p(z(C)), _p(z(2 * C)), float(rows), _p(dx), _p(dg), _p(db),
                          rows, C, 1, _p(rec), st)
            torch.cuda.synchronize()
            assert (rc, rc2) == (E_SHAPE, E_SHAPE), (rc, rc2)
            assert all(_untouched(o) for o in (y, mr, rec, dx, dg, db)), "a refused call wrote to an output"
    elif what == "minmax_misaligned_x":
        rows, C = 8, 8
        x, s4, ws = z(rows * C, 1), B.out(6 * C, "sums4"), B.out(4 * C * 24, "workspace")
        rc = L.query("ladder_bn_fwd_stats_minmax", _p(x), _p(s4), rows, C, _p(ws), ws.n * 4, st)
        torch.cuda.synchronize()
        assert rc == E_ALIGN, rc
        assert _untouched(s4) and _untouched(ws)
    elif what == "minmax_planes_c_not_4":
        rows, C = 8, 6
        n = rows * C
        x, s4, ws = z(n), B.out(6 * C, "sums4"), B.out(4 * C * 24, "workspace")
        y, pl, mr, rec = B.out(n, "y"), B.out(n + 8, "planes"), B.out(2 * C, "mean_rstd"), B.out(ABSMAX_FLOATS, "record")
        rc = L.query("ladder_bn_fwd_stats_minmax", _p(x), _p(s4), rows, C, _p(ws), ws.n * 4, st)
        rc2 = L.query("ladder_bn_fwd_apply_planes", _p(x), _p(z(6 * C)), float(rows), _p(z(C)), _p(z(C)), _p(y), _p(pl), _p(mr), rows, C, BN_EPS, 1, _p(rec), st)
        torch.cuda.synchronize()
        assert (rc, rc2) == (E_SHAPE, E_SHAPE), (rc, rc2)
        assert all(_untouched(o) for o in (s4, ws, y, pl, mr, rec))
    else:
        assert what == "planes_n_not_8"
        rows, C = 3, 4
        n = rows * C
        y, pl, mr, rec = B.out(n, "y"), B.out(n + 8, "planes"), B.out(2 * C, "mean_rstd"), B.out(ABSMAX_FLOATS, "record")
        rc = L.query("ladder_bn_fwd_apply_planes", _p(z(n)), _p(z(6 * C)), float(rows), _p(z(C)), _p(z(C)), _p(y), _p(pl), _p(mr), rows, C, BN_EPS, 1, _p(rec), st)
        torch.cuda.synchronize()
        assert rc == E_SHAPE, rc
        assert all(_untouched(o) for o in (y, pl, mr, rec))
    B.check("refusals")
    return {}, {}, {}


def _sum_bound(terms, rows):
    """Worst case of an fp64 sum of `rows` terms per channel in any order: rows * 2^-52 * sum |term|."""
    return rows * 2.0 ** -52 * np.abs(terms).sum(0, dtype=np.longdouble).astype(np.float64)


def _exact_colsum(a):
    return a.sum(0, dtype=np.longdouble)


def run_colstats(L, row, st):
    _, rows, C, shift = row
    f = features(row)
    rng = np.random.default_rng(_seed(row))
    sd = 0.5 + rng.random(C)
    x = (rng.standard_normal((rows, C)) * sd + 3.0 * sd * np.where(rng.random(C) < 0.5, -1.0, 1.0)).astype(np.float32)
    g, be = _gammas(rng, C), (0.2 * rng.standard_normal(C)).astype(np.float32)
    x64 = x.astype(np.float64)
    mr = np.concatenate([x64.mean(0), 1.0 / np.sqrt(x64.var(0) + BN_EPS)]).astype(np.float32)
    mu64, rs64, g64, be64 = mr[:C].astype(np.float64), mr[C:].astype(np.float64), g.astype(np.float64), be.astype(np.float64)
    x = _clear_kinks(x, lambda xx: g64 * ((xx.astype(np.float64) - mu64) * rs64) + be64, sd, g, "leaky_relu")
    x64 = x.astype(np.float64)
    dy = rng.standard_normal((rows, C)).astype(np.float32)
    B = _Bufs()
    xd, dyd, mrd, gd, bd = B.inp(x, "x", shift), B.inp(dy, "dy"), B.inp(mr, "mean_rstd"), B.inp(g, "gamma"), B.inp(be, "beta")
    nblk = f["nblk"]
    assert L.query("ladder_bn_workspace_bytes", rows, C) == nblk * 2 * C * 8
    errs, bars = {}, {}
    t0, t1 = x64, x64 * x64
    want = np.concatenate([_exact_colsum(t0), _exact_colsum(t1)]).astype(np.longdouble)
    bound = np.concatenate([_sum_bound(t0, rows), _sum_bound(t1, rows)])
    for name, minmax in (("ladder_bn_fwd_stats", False), ("ladder_bn_fwd_stats_minmax", True)):
        if minmax and not f["minmax"]:
            continue
        rec = B.out(6 * C if minmax else 4 * C, "record of " + name)
        ws = B.ws(nblk * C * (24 if minmax else 16), "workspace of " + name)
        L.call(name, _p(xd), _p(rec), rows, C, _p(ws), ws.n * 4, st)
        B.check(name)
        got, r = _host_record(rec, C, name)
        dev = np.abs(got.astype(np.longdouble) - want).astype(np.float64)
        assert (dev <= bound).all(), "%s: fp64 sums off by %s of the worst-case bound" % (name, (dev / np.maximum(bound, 1e-300)).max())
        errs[name] = float((dev / np.maximum(bound, 1e-300)).max())
        bars[name] = 1.0 + 1e-12
        if minmax:
            assert np.array_equal(r[:C].view(np.int32), x.min(0).view(np.int32)) and np.array_equal(r[C:].view(np.int32), x.max(0).view(np.int32)), "extremes"
    xh = (x64 - mu64) * rs64
    dp = dy.astype(np.float64) * np.where(g64 * xh + be64 > 0, 1.0, 0.2)
    ds = B.out(2 * C, "dsums")
    wsd = B.ws(nblk * 2 * C * 4, "backward workspace")
    L.call("ladder_bn_bwd_stats", _p(dyd), _p(xd), _p(mrd), _p(gd), _p(bd), _p(ds), rows, C, 1, _p(wsd), wsd.n * 4, st)
    B.check("ladder_bn_bwd_stats")
    got = _host(ds, (2, C), "dsums").astype(np.float64)
    for i, (nm, t) in enumerate((("sum_dp", dp), ("sum_dp_xhat", dp * xh))):
        errs[nm] = float((np.abs(got[i] - t.sum(0)) / np.maximum(np.abs(t).sum(0), 1e-300)).max())            # (one row: xhat == 0, every term is 0)
        bars[nm] = BAR_BWD_SUMS
    return errs, bars, {}


def run_stage2(L, row, st):
    _, minmax, nblk, C = row
    k = 4 if minmax else 2
    rng = np.random.default_rng(_seed(row))
    scale = 10.0 ** rng.uniform(-3, 3, C)                                                 # per-channel scales over 1e-3 .. 1e3, both signs
    part = (rng.standard_normal((nblk, k, C)) * scale).astype(np.float32)
    B = _Bufs()
    pd, rec = B.inp(part, "partials"), B.out((6 if minmax else 4) * C, "record")
    L.call("ladder_bn_stats_minmax_from_partials" if minmax else "ladder_bn_stats_from_partials", _p(pd), nblk, _p(rec), C, st)
    B.check("second stage")                                                               # nothing past 6C (4C) floats of the record
    got, r = _host_record(rec, C, "record")
    got = got.reshape(2, C)
    p64 = part.astype(np.float64)
    worst = 0.0
    for i in range(2):
        dev = np.abs(got[i].astype(np.longdouble) - _exact_colsum(p64[:, i])).astype(np.float64)
        bound = _sum_bound(p64[:, i], nblk)
        assert (dev <= bound).all(), "sum %d off by %s of the worst-case bound" % (i, (dev / bound).max())
        worst = max(worst, float((dev / np.maximum(bound, 1e-300)).max()))
    if minmax:
        assert np.array_equal(r[:C].view(np.int32), part[:, 2].min(0).view(np.int32)), "minima"
        assert np.array_equal(r[C:].view(np.int32), part[:, 3].max(0).view(np.int32)), "maxima"
    return {"sums_of_bound": worst}, {"sums_of_bound": 1.0 + 1e-12}, {}


def run_in(L, row, st):
    from test_gpu_split import recmax, rec_sample
    _, N, H, W, C, data = row
    f = features(row)
    d = in_reference(N, H, W, C, "off" if data == "absmax" else data)
    ref, HW, n = d["ref"], H * W, N * H * W * C
    bars = in_bars(d["rest"])
    B = _Bufs()
    wsb = L.query("ladder_in_style_workspace_bytes", N, HW, C)
    assert wsb == f["ws_bytes"]
    sty, dy = B.inp(d["sty"], "style"), B.inp(d["dy"], "dy")
    errs = {}

    for route in ("ws", "nows", "shift"):                                                 # (quantity/route: every route is held to the bar on its own)
        def upd(k, v, route=route):
            errs["%s/%s" % (k, route)] = max(errs.get("%s/%s" % (k, route), 0.0), v)
        x = B.inp(d["x"], "x (%s)" % route, int(route == "shift"))
        ws = B.ws(wsb, "workspace (%s)" % route) if route != "nows" else None
        wsn = 0 if ws is None else wsb
        y, mr, dx, dst = B.out(n, "y"), B.out(N * 2 * C, "mean_rstd"), B.out(n, "dx"), B.out(N * 2 * C, "dstyle")
        L.call("ladder_in_style_fwd", _p(x), _p(sty), _p(y), _p(mr), N, HW, C, IN_EPS, 1, _p(ws), wsn, st)
        B.check("forward, route " + route)
        _host(mr, (N, 2 * C), "mean_rstd")
        yh = _host(y, (N, H, W, C), "y")
        upd("y", chan_err(yh, ref["y"]))
        L.call("ladder_in_style_bwd", _p(dy), _p(x), _p(sty), _p(mr), _p(dx), _p(dst), N, HW, C, 1, _p(ws), wsn, st)
        B.check("backward, route " + route)
        dxh = _host(dx, (N, H, W, C), "dx")
        upd("dx", chan_err(dxh, ref["dx"]))
        upd("dstyle", vec_err(_host(dst, (N, 2 * C), "dstyle"), ref["dstyle"]))
        if route == "ws" and f["vec"]:
            up, yk, mr2 = B.out(4 * n, "up"), B.out(n, "y (kept)"), B.out(N * 2 * C, "mean_rstd (fused)")
            L.call("ladder_in_style_fwd_resize2x_keep", _p(x), _p(sty), _p(up), _p(yk), _p(mr2), N, H, W, C, IN_EPS, 1, _p(ws), wsn, None, st)
            B.check("fused resize")
            upd("up", chan_err(_host(up, (N, 2 * H, 2 * W, C), "up"), ref["up"]))
            upd("y", chan_err(_host(yk, (N, H, W, C), "y (kept)"), ref["y"]))
            _host(mr2, (N, 2 * C), "mean_rstd (fused)")
            if f["record"]:
                rec, y2, dx2, dst2 = B.out(ABSMAX_FLOATS, "record"), B.out(n, "y (record)"), B.out(n, "dx (record)"), B.out(N * 2 * C, "dstyle (record)")
                L.call("ladder_in_style_fwd_absmax", _p(x), _p(sty), _p(y2), _p(mr2), N, HW, C, IN_EPS, 1, _p(ws), wsn, _p(rec), st)
                B.check("forward with record")
                y2h = _host(y2, (N, H, W, C), "y (record)")
                assert np.array_equal(y2h.view(np.int32), yh.view(np.int32))
                assert recmax(rec.t) == float(np.abs(y2h).max()) and all(rec_sample(rec.t, i) == float(np.abs(y2h[i]).max()) for i in range(N)), "record of max|y|"
                L.call("ladder_in_style_bwd_absmax", _p(dy), _p(x), _p(sty), _p(mr), _p(dx2), _p(dst2), N, HW, C, 1, _p(ws), wsn, _p(rec), st)
                B.check("backward with record")
                d2h = _host(dx2, (N, H, W, C), "dx (record)")
                assert np.array_equal(d2h.view(np.int32), dxh.view(np.int32))
                assert recmax(rec.t) == float(np.abs(d2h).max()) and all(rec_sample(rec.t, i) == float(np.abs(d2h[i]).max()) for i in range(N)), "record of max|dx|"
    return errs, {k: bars[k.split("/")[0]] for k in errs}, d["rest"]


def run_resize(L, row, st):
    import torch
    from oracle import ladder_oracle as O
    _, N, H, W, C, OH, OW, shift = row
    f = features(row)
    rng = np.random.default_rng(_seed(row))
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    dy = rng.standard_normal((N, OH, OW, C)).astype(np.float32)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yr = O.resize_bilinear_legacy(xt, OH, OW)
    (yr * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    B = _Bufs()
    xd, dyd = B.inp(x, "x", shift), B.inp(dy, "dy", shift)
    y, dx = B.out(dy.size, "y"), B.out(x.size, "dx")
    L.call("ladder_resize_bilinear_fwd", _p(xd), _p(y), N, H, W, C, OH, OW, st)
    L.call("ladder_resize_bilinear_bwd", _p(dyd), _p(dx), N, H, W, C, OH, OW, st)
    B.check("resize")
    dxh = _host(dx, x.shape, "dx")
    errs = dict(y=vec_err(_host(y, dy.shape, "y"), yr.detach().numpy()), dx=vec_err(dxh, xt.grad.numpy()))
    gate = rng.standard_normal((N, H, W, C)).astype(np.float32)
    gd, dxg = B.inp(gate, "gate", shift), B.out(x.size, "dx (gated)")
    rc = L.query("ladder_resize_bilinear_bwd_gated", _p(dyd), _p(dxg), N, H, W, C, OH, OW, _p(gd), 1, st)
    B.check("gated transpose")
    if f["gated"]:                                    # bit-identical to the ungated form times leaky'
        assert rc == 0, rc
        want = dxh * np.where(gate > 0, np.float32(1.0), np.float32(0.2))
        assert np.array_equal(_host(dxg, x.shape, "dx (gated)").view(np.int32), want.view(np.int32)), "gated form"
    else:
        assert rc == E_SHAPE and _untouched(dxg), rc
    return errs, dict(y=BAR_COPY, dx=BAR_COPY), {}


def run_d2s(L, row, st):
    import torch
    from oracle import ladder_oracle as O
    _, N, H, W, C, r, shift = row
    rng = np.random.default_rng(_seed(row))
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    yr = O.depth_to_space(torch.tensor(x), r).numpy()
    B = _Bufs()
    xd, y, back = B.inp(x, "x", shift), B.out(x.size, "y", shift), B.out(x.size, "back", shift)
    L.call("ladder_depth_to_space", _p(xd), _p(y), N, H, W, C, r, 0, st)
    L.call("ladder_depth_to_space", _p(y), _p(back), N, H, W, C, r, 1, st)
    B.check("depth to space")
    assert np.array_equal(_host(y, yr.shape, "y").view(np.int32), np.ascontiguousarray(yr).view(np.int32)), "forward"
    assert np.array_equal(_host(back, x.shape, "back").view(np.int32), x.view(np.int32)), "inverse"
    return {}, {}, {}


def run_pad(L, row, st):
    import torch
    from oracle import ladder_oracle as O
    _, N, H, W, C, p = row
    rng = np.random.default_rng(_seed(row))
    x = rng.standard_normal((N, H, W, C)).astype(np.float32)
    dy = rng.standard_normal((N, H + 2 * p, W + 2 * p, C)).astype(np.float32)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    yr = O.pad_symmetric(xt, p)
    (yr * torch.tensor(dy, dtype=torch.float64)).sum().backward()
    assert np.array_equal(yr.detach().numpy(), np.pad(x.astype(np.float64), ((0, 0), (p, p), (p, p), (0, 0)), mode="symmetric"))
    B = _Bufs()
    xd, dyd, y, dx = B.inp(x, "x"), B.inp(dy, "dy"), B.out(dy.size, "y"), B.out(x.size, "dx")
    L.call("ladder_pad_symmetric", _p(xd), _p(y), N, H, W, C, p, st)
    L.call("ladder_pad_symmetric_bwd", _p(dyd), _p(dx), N, H, W, C, p, st)
    B.check("symmetric pad")
    assert np.array_equal(_host(y, dy.shape, "y").view(np.int32), yr.detach().numpy().astype(np.float32).view(np.int32)), "forward"
    return dict(dx=vec_err(_host(dx, x.shape, "dx"), xt.grad.numpy())), dict(dx=BAR_COPY), {}


def run_act_bwd(L, row, st):
    """Against float64 dy * act'(y), the derivative through the OUTPUT (ladder_act_grad_from_out).  fp32 forms y * y, 1 - y * y and the product with at most
    three roundings: |error| <= 3 * 2^-24 * |dy| * (1 + y^2) <= 2^-22 |dy| (1 + y^2), which also covers 0.2f against 0.2.  In place: the same bits."""
    _, n, act = row
    rng = np.random.default_rng(_seed(row))
    pre = rng.standard_normal(n)
    y = (np.tanh(pre) if act == "tanh" else pre).astype(np.float32)
    if n > 4:
        y[::5] = 0.0                                  # y == 0 goes with the negative side
    dy = rng.standard_normal(n).astype(np.float32)
    y64, dy64 = y.astype(np.float64), dy.astype(np.float64)
    grad = {None: np.ones(n), "leaky_relu": np.where(y64 > 0, 1.0, 0.2), "relu": np.where(y64 > 0, 1.0, 0.0), "tanh": 1.0 - y64 * y64}[act]
    ref = dy64 * grad
    B = _Bufs()
    yd, dyd, dx, inpl = B.inp(y, "y"), B.inp(dy, "dy"), B.out(n, "dx"), B.inp(dy, "dy (in place)")
    L.call("ladder_act_bwd", _p(dyd), _p(yd), _p(dx), n, ACT[act], st)
    L.call("ladder_act_bwd", _p(inpl), _p(yd), _p(inpl), n, ACT[act], st)
    B.check("activation backward")
    got, got2 = _host(dx, (n,), "dx"), _host(inpl, (n,), "dx (in place)")
    bound = 2.0 ** -22 * np.abs(dy64) * (1.0 + y64 * y64)
    assert (np.abs(got - ref) <= bound).all(), "against float64: %s of the bound" % (np.abs(got - ref) / np.maximum(bound, 1e-300)).max()
    assert np.array_equal(got.view(np.int32), got2.view(np.int32)), "in place (dx == dy) differs from out of place"
    return {"of_bound": float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())}, {"of_bound": 1.0 + 1e-12}, {}


RUNNERS = dict(bn=run_bn, refuse=run_refuse, colstats=run_colstats, stage2=run_stage2, resize=run_resize, d2s=run_d2s, pad=run_pad, act_bwd=run_act_bwd)
RUNNERS["in"] = run_in


def run_row(L, row, stream):
    """-> (errors, bars, restatement errors), dicts by quantity; exact comparisons and guard checks are asserted inside."""
    return RUNNERS[row[0]](L, row, stream)
