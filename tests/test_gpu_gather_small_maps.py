"""The forms of the small-tile gather kernel (csrc/igemm.hip: igemm_fwd_kernel<64,64,...> / <32,128,...>) through ladder_conv2d_fwd_variant,
ladder_conv2d_bwd_data_variant and ladder_dense_fwd_variant: variant bit 0 = position-major rows + padding-tap skipping on small maps, bits 1-2 =
prefetch depth - 1.

Every case is checked two ways: every variant is bit-equal to variant 0 (y and dx, with and without the split-K workspace, backward-data with
and without the gate), and variant 0 and the default entry point hold the float64 bars of tests/test_gpu_kernels.py::test_conv2d_fwd_bwd
(2e-5 forward, 3e-5 backward-data, relative to the output scale).  The shapes are the smallest that reach each path.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ladder_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = tuple(range(8))

# N, H, W, Cin, Cout, k, stride, padding
SMALL_MAP_CASES = [
    (64, 2, 2, 16, 64, 3, 1, "same"),       # one position per tile
    (128, 2, 2, 16, 64, 3, 1, "same"),      # two tiles per position
    (96, 2, 2, 16, 64, 3, 1, "same"),       # a tile straddles two positions: the union mask applies
    (3, 2, 2, 16, 64, 3, 1, "same"),        # N < BM: image-major stays, nothing skipped
    (64, 4, 4, 16, 16, 3, 1, "valid"),      # backward-data: a full correlation over the 2x2 gradient, 1 / 2 / 4 live taps
    (64, 8, 8, 16, 32, 3, 2, "same"),       # dead bottom / right tap line in the forward; parity-class backward-data
    (64, 2, 2, 16, 16, 5, 1, "same"),       # 25 taps in the 32-bit mask
    (2, 8, 8, 16, 48, 1, 2, "same"),        # backward-data classes without a tap: zeros
    (128, 2, 2, 256, 256, 3, 1, "same"),    # split-K together with skipping
    (32, 1, 1, 16, 128, 3, 1, "same"),      # the 32x128 tile, position-major: only the centre tap is live
    # (tile selection sends a GEMM of at most 32 columns to the 128x32 tile, which walks every tap: the same geometries with 64 channels on both
    # sides, so that forward and backward-data both run the 64x64 tile)
    (64, 4, 4, 64, 64, 3, 1, "valid"),
    (64, 8, 8, 64, 64, 3, 2, "same"),
    (64, 2, 2, 64, 64, 5, 1, "same"),
]
DEPTH_CASES = [
    (8, 4, 4, 16, 64, 1, 1, "same"),        # 1, 2, 3 and 5 chunks
    (8, 4, 4, 32, 64, 1, 1, "same"),
    (8, 4, 4, 48, 64, 1, 1, "same"),
    (8, 4, 4, 80, 64, 1, 1, "same"),
    (32, 2, 2, 256, 256, 3, 1, "same"),     # with workspace: split ranges shorter than the depth
    (4, 8, 8, 3, 64, 3, 1, "same"),         # scalar A path
    (4, 8, 8, 20, 64, 3, 1, "same"),
    (8, 4, 4, 32, 160, 3, 1, "same"),       # ragged N tile (160 = 2 * 64 + 32)
    (2, 4, 4, 32, 128, 3, 1, "same"),       # the 32x128 tile (M = 32)
]


def _lib():
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    return L


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def rel_err(got, ref):
    got = got.detach().cpu().numpy().astype(np.float64)
    ref = ref.detach().numpy().astype(np.float64)
    assert got.shape == ref.shape and np.isfinite(got).all()
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.mark.parametrize("case", SMALL_MAP_CASES + DEPTH_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_conv_variants_bit_equal_and_float64(gpu_ctx, case):
    L = _lib()
    from ladder_latent_data_distribution_modelling_amd import arch
    N, H, W, Cin, Cout, k, s, pad = case
    rng = np.random.default_rng(sum(v * 31 ** i for i, v in enumerate(case[:7])) % 2**31)
    x = rng.standard_normal((N, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)).astype(np.float32)
    b = rng.standard_normal(Cout).astype(np.float32)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    wt = torch.tensor(w, dtype=torch.float64)
    bt = torch.tensor(b, dtype=torch.float64)
    yr = O.conv2d_tf(xt, wt, bt, s, pad)
    dy = rng.standard_normal(tuple(yr.shape)).astype(np.float32)
    yr.backward(torch.tensor(dy, dtype=torch.float64))
    pt, Ho = arch.conv_out(H, k, s, pad)
    pl, Wo = arch.conv_out(W, k, s, pad)
    assert (Ho, Wo) == tuple(yr.shape[1:3])

    st = gpu_ctx.stream
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    fws = torch.empty(max(L.query("ladder_igemm_fwd_workspace_bytes", N * Ho * Wo, k * k * Cin, Cout), 16), dtype=torch.uint8, device="cuda")
    dws = torch.empty(max(L.query("ladder_igemm_fwd_workspace_bytes", N * H * W, k * k * Cout, Cin), 16), dtype=torch.uint8, device="cuda")
    wT = torch.empty(wd.numel(), device="cuda")
    L.call("ladder_filter_flip_transpose", p(wd), p(wT), k, k, Cin, Cout, st)
    geo = (N, H, W, Cin, Ho, Wo, Cout, k, k, s, pt, pl)

    def fwd(variant, ws):
        y = torch.full((N, Ho, Wo, Cout), float("nan"), device="cuda")
        tail = (p(ws), ws.numel()) if ws is not None else (None, 0)
        if variant is None:
            L.call("ladder_conv2d_fwd", p(xd), p(wd), p(bd), p(y), *geo, 0, *tail, st)
        else:
            L.call("ladder_conv2d_fwd_variant", p(xd), p(wd), p(bd), p(y), *geo, 0, *tail, variant, st)
        return y

    def bwd(variant, ws, gate):
        dx = torch.full((N, H, W, Cin), float("nan"), device="cuda")
        tail = (p(ws), ws.numel()) if ws is not None else (None, 0)
        g = (p(xd), 1) if gate else (None, 0)
        if variant is None:
            L.call("ladder_conv2d_bwd_data", p(dyd), p(wT), p(dx), *geo, *g, *tail, st)
        else:
            L.call("ladder_conv2d_bwd_data_variant", p(dyd), p(wT), p(dx), *geo, *g, *tail, variant, st)
        return dx

    for ws in (fws, None):
        y0 = fwd(0, ws)
        for v in VARIANTS[1:] + (None,):
            assert torch.equal(fwd(v, ws), y0), "fwd: variant %s differs from variant 0 (workspace %s)" % (v, ws is not None)
        e0, ed = rel_err(y0, yr), rel_err(fwd(None, ws), yr)
        print("fwd rel err vs float64: variant 0 %.3e, default %.3e (workspace %s)" % (e0, ed, ws is not None))
        assert e0 < 2e-5 and ed < 2e-5
    for ws in (dws, None):
        for gate in (False, True):
            d0 = bwd(0, ws, gate)
            for v in VARIANTS[1:] + (None,):
                assert torch.equal(bwd(v, ws, gate), d0), "bwd_data: variant %s differs from variant 0 (workspace %s, gate %s)" % (v, ws is not None, gate)
            if not gate:
                e0, ed = rel_err(d0, xt.grad), rel_err(bwd(None, ws, gate), xt.grad)
                print("dx rel err vs float64: variant 0 %.3e, default %.3e (workspace %s)" % (e0, ed, ws is not None))
                assert e0 < 3e-5 and ed < 3e-5
            else:
                assert torch.equal(d0, bwd(0, ws, False) * torch.where(xd > 0, 1.0, 0.2))


@pytest.mark.parametrize("M,K,N", [(512, 512, 4608), (100, 33, 2)])
def test_dense_variants_bit_equal_and_float64(gpu_ctx, M, K, N):
    L = _lib()
    rng = np.random.default_rng(M * 7 + K * 3 + N)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(N).astype(np.float32)
    yr = torch.tensor(x, dtype=torch.float64) @ torch.tensor(w, dtype=torch.float64) + torch.tensor(b, dtype=torch.float64)
    xd, wd, bd = dev(x), dev(w), dev(b)
    wsb = torch.empty(max(L.query("ladder_igemm_fwd_workspace_bytes", M, K, N), 16), dtype=torch.uint8, device="cuda")

    def run(variant, ws):
        y = torch.full((M, N), float("nan"), device="cuda")
        tail = (p(ws), ws.numel()) if ws is not None else (None, 0)
        if variant is None:
            L.call("ladder_dense_fwd", p(xd), p(wd), p(bd), p(y), M, K, N, 0, *tail, gpu_ctx.stream)
        else:
            L.call("ladder_dense_fwd_variant", p(xd), p(wd), p(bd), p(y), M, K, N, 0, *tail, variant, gpu_ctx.stream)
        return y

    for ws in (wsb, None):
        y0 = run(0, ws)
        for v in VARIANTS[1:] + (None,):
            assert torch.equal(run(v, ws), y0), "dense: variant %s differs from variant 0 (workspace %s)" % (v, ws is not None)
        assert rel_err(y0, yr) < 2e-5


def test_variant_out_of_range_is_refused(gpu_ctx):
    L = _lib()
    x, w, y = torch.zeros(64, 16, device="cuda"), torch.zeros(16, 64, device="cuda"), torch.zeros(64, 64, device="cuda")
    for bad in (-1, 8):
        with pytest.raises(Exception):
            L.call("ladder_dense_fwd_variant", p(x), p(w), None, p(y), 64, 16, 64, 0, None, 0, bad, gpu_ctx.stream)


def _engine_child(variant, out):
    env = dict(os.environ)
    env.pop("LADDER_IGEMM_VARIANT", None)
    if variant is not None:
        env["LADDER_IGEMM_VARIANT"] = str(variant)
    return subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(ROOT, "tests", "gather_small_maps_child.py"), out],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)


def test_engine_iteration_is_bit_equal_under_variant_0_and_the_default(tmp_path):
    """One full four-run iteration (RUN#1 ... RUN#4) of the CelebA-shaped strict-fp32 engine at batch 16, in fresh child processes (the switch is
    read once per process): the fetched scalars and every parameter are bit-equal between LADDER_IGEMM_VARIANT=0 and the default."""
    assert 'getenv("LADDER_IGEMM_VARIANT")' in open(os.path.join(ROOT, "ladder_latent_data_distribution_modelling_amd", "csrc", "igemm.hip")).read()
    outs = {}
    for variant in (0, None):
        out = str(tmp_path / ("v%s.npz" % variant))
        proc = _engine_child(variant, out)
        assert proc.returncode == 0, "exit status %d under LADDER_IGEMM_VARIANT=%s:\n%s" % (proc.returncode, variant, proc.stdout[-4000:])
        outs[variant] = np.load(out)
    a, b = outs[0], outs[None]
    assert sorted(a.files) == sorted(b.files) and len(a.files) > 20
    diff = [k for k in a.files if a[k].tobytes() != b[k].tobytes()]
    assert not diff, "not bit-equal: %s" % diff[:10]
