"""Shared by tests/test_upproj_fused_cases_cpu.py and tests/test_gpu_upproj_fused_matrix.py: the case table of the fused pair forward
(csrc/upproj.hip: up2proj_fused_fwd_kernel, up2proj_fused2_fwd_kernel behind ladder_up2proj_fused_fwd / _variant), what each case reaches in the
kernels (`features`: pure arithmetic on the tuple, mirrored against the library's own routing queries by the CPU test), the float64 reference -- the
oracle's resize_bilinear_legacy + conv2d_tf and nothing else -- and a runner that launches the library into guarded, poisoned buffers.

A case is (N, H, W, Cin, Cout, pco, keep_y, act, has_bias, has_proj_bias, proj_out_misaligned).  With total = H * Cin / 32 chunks a workgroup, the
64-pixel kernel's MFMA loop is unrolled by 3, its x staging by 8 (resident slab, Cin <= 128: 7 loads ahead) or by 4 (streamed slab: 3 ahead); the
128-pixel kernel unrolls its MFMA loop by 2 and its staging by 3.  Every remainder of each, both workgroup -> (group, slab) mappings, every width and
every projection form (pco 1 .. 4 with and without the map, without either bias, without activation, into a proj_out that is only 4-byte aligned:
the scalar reduction) appears below; tests/test_upproj_fused_cases_cpu.py proves that from the table, so it cannot shrink unnoticed.

`python tests/upproj_fused_ref.py <group>` runs one group (resident / streamed / wide) against float64 in a fresh process and exits 0 or 1: the
process-wide switches LADDER_UP2FUSE_NO_WRES (a resident-slab shape streams its slab: `total` down to 4 on the streamed path) and
LADDER_UP2FUSE_NO_PT2 (a wide shape runs the 64-pixel kernel) are read once per process and are tested that way."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from guarded import GUARD, GUARD_BITS, _FF_BITS, _Guarded, _NAN_BITS  # noqa: E402,F401  (tests/guarded.py: shared with tests/convf32_cases.py)

TOL32 = 3e-6                # of the reference's scale: the bar of tests/test_gpu_upproj.py (fp32 accumulation of K = Cin <= 512 products + <= 16 additions)
MASKS = (3, 2, 1, 0, None)  # ladder_up2proj_fused_fwd_variant: bit 0 = first wave tiling, bit 1 = first quad exchange (3 gives the reference bits); None = ladder_up2proj_fused_fwd

# (N, H, W, Cin, Cout) -> total
RESIDENT = [(8, 2, 8, 64, 16), (8, 2, 8, 96, 16), (4, 2, 16, 128, 32), (4, 3, 16, 96, 48), (1, 5, 64, 64, 16), (2, 5, 32, 96, 32), (8, 7, 8, 96, 16),
            (16, 9, 8, 96, 16), (2, 3, 32, 128, 16), (4, 7, 16, 64, 32), (8, 4, 64, 128, 16)]                 # 4 6 8 9 10 15 21 27 12 14 16
STREAMED = [(8, 2, 8, 160, 16), (4, 2, 16, 192, 32), (2, 2, 32, 224, 16), (4, 3, 16, 160, 48), (8, 3, 64, 224, 16), (2, 5, 32, 160, 32),
            (8, 5, 8, 224, 16), (64, 2, 8, 256, 16)]                                                          # 10 12 14 15 21 25 35 16
WIDE = [(16, 3, 32, 160, 1024), (32, 5, 32, 224, 512), (64, 7, 16, 224, 512), (72, 2, 16, 160, 512), (64, 3, 16, 160, 512)]   # 15 35 49 10 15

# per shape: (act, has_bias) of the row without projection, then (pco, keep_y, act, has_bias, has_proj_bias, proj_out_misaligned) of the row with it
_RES_FLAGS = [((0, 1), (3, 1, 1, 1, 1, 0)), ((1, 0), (1, 0, 1, 1, 1, 1)), ((1, 1), (2, 1, 0, 1, 1, 0)), ((1, 1), (3, 0, 1, 1, 1, 1)),
              ((0, 1), (4, 1, 1, 0, 1, 0)), ((1, 1), (4, 0, 1, 1, 0, 0)), ((1, 1), (1, 1, 1, 1, 1, 0)), ((0, 0), (2, 0, 1, 1, 1, 0)),
              ((1, 1), (3, 1, 0, 0, 0, 0)), ((1, 1), (3, 0, 1, 1, 1, 0)), ((1, 1), (3, 1, 1, 1, 1, 0))]
_STR_FLAGS = [((1, 1), (1, 1, 1, 1, 1, 0)), ((0, 1), (1, 0, 1, 1, 1, 1)), ((1, 1), (2, 1, 0, 0, 1, 0)), ((1, 0), (2, 0, 1, 1, 1, 0)),
              ((1, 1), (3, 1, 1, 1, 1, 1)), ((1, 1), (3, 0, 1, 1, 0, 0)), ((0, 0), (4, 1, 1, 1, 1, 0)), ((1, 1), (4, 0, 0, 1, 1, 0))]
_WIDE_FLAGS = [(1, 0), (0, 1), (1, 1), (1, 1), (1, 1)]                                 # (act, has_bias); no projection, y kept


def _rows(shapes, flags):
    out = []
    for s, (plain, proj) in zip(shapes, flags):
        out.append(s + (0, 1) + plain + (0, 0))
        out.append(s + proj)
    return out


GROUPS = {"resident": _rows(RESIDENT, _RES_FLAGS), "streamed": _rows(STREAMED, _STR_FLAGS),
          "wide": [s + (0, 1) + f + (0, 0) for s, f in zip(WIDE, _WIDE_FLAGS)]}
CASES = GROUPS["resident"] + GROUPS["streamed"] + GROUPS["wide"]


def case_id(c):
    return "n%d_%dx%d_c%d_co%d_p%d_y%d_a%d_b%d_pb%d_m%d" % c


def features(case):
    """What a case reaches in csrc/upproj.hip under the library's default switches, from the tuple alone."""
    N, H, W, cin, cout, pco = case[:6]
    nslab, total = cout // 16, H * cin // 32
    wide = pco == 0 and cin > 128 and W in (16, 32) and N % (128 // W) == 0 and (N // (128 // W)) * nslab >= 256
    ngroups = N // ((128 if wide else 64) // W)
    f = dict(kernel="wide" if wide else "px64", resident=cin <= 128, total=total, mod3=total % 3, W=W, xcd=ngroups % 8 == 0, ngroups=ngroups, nslab=nslab)
    if wide:
        f["mod2"] = total % 2
    else:
        f["stage_mod"] = total % 8 if cin <= 128 else total % 4
    return f


def _rel(got, ref):
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


@functools.lru_cache(maxsize=2)                       # the rows of one shape are neighbours in CASES: its convolution is computed once
def _shape_data(shape):
    """x, w, b, pw [Cout][4], pb [4] (float32) of a shape and the float64 oracle's resize -> 3x3 / SAME convolution of x and w (no bias, no activation)."""
    import torch
    from oracle import ladder_oracle as O
    N, H, W, cin, cout = shape
    rng = np.random.default_rng(N * 1000003 + H * 10007 + W * 101 + cin * 7 + cout)
    x = rng.standard_normal((N, H, W, cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    pw = (rng.standard_normal((cout, 4)) / np.sqrt(cout)).astype(np.float32)
    pb = (rng.standard_normal(4) * 0.1).astype(np.float32)
    up = O.resize_bilinear_legacy(torch.as_tensor(x, dtype=torch.float64), 2 * H, 2 * W)
    pre = O.conv2d_tf(up, torch.as_tensor(w, dtype=torch.float64), None, 1, "same").numpy()
    pre.setflags(write=False)                         # shared by the rows of the shape
    return x, w, b, pw, pb, pre


def reference(case):
    """(inputs, float64 map, float64 projection or None) of a case."""
    cout, pco, _, act, has_bias, has_pb = case[4:10]
    x, w, b, pw, pb, pre = _shape_data(case[:5])
    ref = pre + b.astype(np.float64) if has_bias else pre
    if act:
        ref = np.where(ref > 0, ref, 0.2 * ref)
    pw_ = np.ascontiguousarray(pw[:, :pco]) if pco else None
    pb_ = np.ascontiguousarray(pb[:pco]) if pco and has_pb else None
    pref = None
    if pco:
        pref = ref @ pw_.astype(np.float64)
        if has_pb:
            pref = pref + pb_.astype(np.float64)
    return (x, w, b if has_bias else None, pw_, pb_), ref, pref


def launch(L, case, inputs, stream, variant):
    """One launch of the case (variant None: ladder_up2proj_fused_fwd, the default entry) -> (y or None, proj_out or None) as host float32 arrays.
    Asserts the guard bands of y, proj_out and the workspace bitwise, and that nothing NaN is left in an output."""
    import torch
    N, H, W, cin, cout, pco, keep_y, act, _, _, mis = case
    xd, wcatT, bd, pwd, pbd = inputs
    P = N * 4 * H * W
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    y = _Guarded(P * cout, _NAN_BITS) if keep_y else None
    out = ws = None
    ws_bytes = 0
    if pco:
        out = _Guarded(P * pco, _NAN_BITS, shift=1 if mis else 0)
        ws_bytes = int(L.query("ladder_up2proj_fused_workspace_bytes", N, H, W, cout, pco))
        assert ws_bytes == (cout // 16) * P * pco * 4
        ws = _Guarded(ws_bytes // 4, _FF_BITS)
    args = (ptr(xd), ptr(wcatT), ptr(bd), y.t.data_ptr() if y else None, ptr(pwd), ptr(pbd), out.t.data_ptr() if out else None, pco, N, H, W, cin, cout, act,
            ws.t.data_ptr() if ws else None, ws_bytes)
    if variant is None:
        L.call("ladder_up2proj_fused_fwd", *args, stream)
    else:
        L.call("ladder_up2proj_fused_fwd_variant", *args, variant, stream)
    torch.cuda.synchronize()
    res = []
    for name, g in (("y", y), ("proj_out", out), ("workspace", ws)):
        if g is not None:
            assert g.guards_intact(), "%s: guard band overwritten (variant %s)" % (name, variant)
        if name == "workspace" and g is not None:
            assert not bool((g.bits[g.lo:g.lo + g.n] == _FF_BITS).any().item()), "workspace: a partial was never written (variant %s)" % variant
        if g is None or name == "workspace":
            continue
        a = g.t.cpu().numpy()
        assert not np.isnan(a).any(), "%s: NaN left (unwritten element, or a poisoned partial summed), variant %s" % (name, variant)
        assert np.isfinite(a).all(), "%s: not finite, variant %s" % (name, variant)
        res.append(a)
    it = iter(res)
    return (next(it).reshape(N, 2 * H, 2 * W, cout) if keep_y else None), (next(it).reshape(N, 2 * H, 2 * W, pco) if pco else None)


def run_case(L, case, stream, masks=MASKS):
    """Launches the case once per entry of `masks` (None: the default entry), compares the first launch with float64 and every other launch bit for
    bit with the first.  Returns {"map": worst relative error or None, "proj": ... or None}; the caller holds them to TOL32."""
    import torch
    N, H, W, cin, cout, pco, keep_y = case[:7]
    (x, w, b, pw_, pb_), ref, pref = reference(case)
    dev = lambda a: None if a is None else torch.as_tensor(a).cuda()  # noqa: E731
    wd = dev(w)
    wcatT = torch.full((9 * cout, cin), float("nan"), device="cuda")
    L.call("ladder_filter_pack_split", wd.data_ptr(), wcatT.data_ptr(), 1, 9 * cout, cin, 7, 0, stream)
    inputs = (dev(x), wcatT, dev(b), dev(pw_), dev(pb_))
    first = None
    for variant in masks:
        y, out = launch(L, case, inputs, stream, variant)
        if first is None:
            first = (y, out)
            continue
        if keep_y:
            assert np.array_equal(y, first[0]), "map: variant %s differs from variant %s" % (variant, masks[0])
        if pco:
            assert np.array_equal(out, first[1]), "projection: variant %s differs from variant %s" % (variant, masks[0])
    return dict(map=_rel(first[0].astype(np.float64), ref) if keep_y else None, proj=_rel(first[1].astype(np.float64), pref) if pco else None)


def worst(errs):
    """{"map": ..., "proj": ...}: the largest of each over a list of run_case results (None where no case had one)."""
    return {k: max([e[k] for e in errs if e[k] is not None], default=None) for k in ("map", "proj")}


def main(argv):
    if len(argv) != 2 or argv[1] not in GROUPS:
        print("usage: python tests/upproj_fused_ref.py {%s}" % "|".join(GROUPS))
        return 2
    import torch
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    L.load()
    stream = torch.cuda.current_stream().cuda_stream
    errs, bad = [], 0
    for case in GROUPS[argv[1]]:
        assert L.query("ladder_up2proj_fused_eligible", *case[:5]) == 1, case
        e = run_case(L, case, stream)
        errs.append(e)
        ok = all(v is None or v < TOL32 for v in e.values())
        bad += not ok
        print("%s %s wide_tile=%d map=%s proj=%s" % ("ok  " if ok else "FAIL", case_id(case), L.query("ladder_up2proj_fused_wide_tile", *case[:5]), e["map"], e["proj"]),
              flush=True)
    w = worst(errs)
    print("group %s: %d cases, %d failed; worst relative error map %s projection %s (bar %.1e)" % (argv[1], len(errs), bad, w["map"], w["proj"], TOL32))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
