"""The forms of the 64-pixel fused forward kernel (csrc/upproj.hip: up2proj_fused_fwd_kernel) through ladder_up2proj_fused_fwd_variant.

Variant 0: an MFMA wave owns 2 pixel tiles x 4 taps + 1 cell, and the projection sums a pixel's four lanes with quad-perm DPP (three outputs wide where
proj_cout == 3).  Bit 0 of the mask selects the first wave tiling (1 tile x 9 taps), bit 1 the first exchange (LDS-queue lane exchanges, four outputs
wide); ladder_up2proj_fused_fwd runs the library's default mask.  Every accumulator sums the same products in the same order and the quad sum keeps
its association (a + a^1) + (a^2 + a^3), so the variants must agree BIT FOR BIT -- torch.equal, no tolerance -- on the map and on the projection.

Cases (N, H, W, Cin, Cout, proj_cout, keep_y), the smallest that reach every branch of the kernel:
  W = 8, one group, resident slab, no projection | W = 16, three slabs, odd H, proj_cout = 3 | W = 32, projection without y, generic proj_cout = 4 |
  W = 64, 8 groups (the XCD tile order), proj_cout = 1 | streamed slab (Cin > 128), 5 chunks a row (not a multiple of the 3 stages) |
  streamed slab with projection, without y.
None is routed to the 128-pixel row step kernel, which has one form."""
import numpy as np
import pytest
import torch

from test_gpu_split import _lib, close, dev, p
from test_gpu_upproj import TOL32, _pack, _ref_fwd, _ws

pytestmark = pytest.mark.gpu

CASES = [(8, 2, 8, 64, 16, 0, 1), (4, 3, 16, 96, 48, 3, 1), (2, 3, 32, 128, 32, 4, 0), (8, 2, 64, 64, 16, 1, 1), (2, 5, 32, 160, 32, 0, 1), (1, 2, 64, 192, 16, 3, 0)]
ALL_MASKS = {(4, 3, 16, 96, 48, 3, 1), (1, 2, 64, 192, 16, 3, 0)}          # masks 1 and 2 as well: resident and streamed slab, both with proj_cout = 3
ORACLE_CASE = (4, 3, 16, 96, 48, 3, 1)                                     # the default form against float64 as well


def _run(L, variant, xd, wcatT, bd, pwd, pbd, case, st):
    N, H, W, cin, cout, pco, keep_y = case
    y = torch.full((N, 2 * H, 2 * W, cout), float("nan"), device="cuda") if keep_y else None
    out = ws = None
    if pco:
        out = torch.full((N, 2 * H, 2 * W, pco), float("nan"), device="cuda")
        ws = _ws(L.query("ladder_up2proj_fused_workspace_bytes", N, H, W, cout, pco))
    args = (p(xd), p(wcatT), p(bd), p(y), p(pwd) if pco else None, p(pbd) if pco else None, p(out), pco, N, H, W, cin, cout, 1, p(ws), ws.numel() if pco else 0)
    if variant is None:                                                     # the default path
        L.call("ladder_up2proj_fused_fwd", *args, st)
    else:
        L.call("ladder_up2proj_fused_fwd_variant", *args, variant, st)
    return y, out


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_%dx%d_c%d_co%d_p%d_y%d" % c)
def test_upproj_fused_variants_are_bit_identical(gpu_ctx, case):
    L = _lib()
    N, H, W, cin, cout, pco, keep_y = case
    st = gpu_ctx.stream
    assert L.query("ladder_up2proj_fused_eligible", N, H, W, cin, cout) == 1
    assert L.query("ladder_up2proj_fused_wide_tile", N, H, W, cin, cout) == 0
    rng = np.random.default_rng(H * 100 + cin + cout + N)
    x = rng.standard_normal((N, H, W, cin)).astype(np.float32)
    w = (rng.standard_normal((3, 3, cin, cout)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) * 0.1
    pw_ = (rng.standard_normal((cout, max(pco, 1))) / np.sqrt(cout)).astype(np.float32)
    pb_ = rng.standard_normal(max(pco, 1)).astype(np.float32) * 0.1
    _, wcatT = _pack(L, w, st)
    xd, bd, pwd, pbd = dev(x), dev(b), dev(pw_), dev(pb_)
    y3, out3 = _run(L, 3, xd, wcatT, bd, pwd, pbd, case, st)               # the first forms of both: the reference bits
    for variant in ((0, 1, 2) if case in ALL_MASKS else (0,)):
        y, out = _run(L, variant, xd, wcatT, bd, pwd, pbd, case, st)
        if keep_y:
            assert torch.equal(y, y3), "map, variant %d" % variant
        if pco:
            assert torch.equal(out, out3), "projection, variant %d" % variant
    if case == ORACLE_CASE:
        y, out = _run(L, None, xd, wcatT, bd, pwd, pbd, case, st)
        assert torch.equal(y, y3) and torch.equal(out, out3)
        ref = _ref_fwd(x, w, b, "leaky_relu")
        close(y, ref, TOL32, "map against float64")
        close(out, ref @ pw_.astype(np.float64) + pb_.astype(np.float64), TOL32, "projection against float64")


def test_upproj_fused_variant_mask_is_checked(gpu_ctx):
    L = _lib()
    from ladder_latent_data_distribution_modelling_amd._lib import LadderHipError
    x = torch.zeros(8, 2, 8, 64, device="cuda")
    wT = torch.zeros(9 * 16, 64, device="cuda")
    y = torch.zeros(8, 4, 16, 16, device="cuda")
    for bad in (-1, 4):
        with pytest.raises(LadderHipError, match="LADDER_E_SHAPE"):
            L.call("ladder_up2proj_fused_fwd_variant", p(x), p(wT), None, p(y), None, None, None, 0, 8, 2, 8, 64, 16, 0, None, 0, bad, gpu_ctx.stream)
