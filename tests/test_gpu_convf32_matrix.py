"""The strict-fp32 3x3 halo convolutions (csrc/convf32s.hip: conv3x3_halo_f32s_kernel in all 21 instantiations; csrc/convf32.hip: the 8x32-pixel kernel at
the route boundary and in its class launches) against the float64 oracle on EVERY row of tests/convf32_cases.py, through the public entry points with
prec = LADDER_PREC_F32: every tiling in every entry, 1 / 2 / 3 live images of four and 1 of two in the last workgroup, ragged channel tiles with one and
two 64-channel tiles per workgroup and below 64 channels, 2 and 3 sub-patches per image row / column, and the shapes on either side of the 512- and the
256-workgroup thresholds.  tests/test_convf32_cases_cpu.py proves that the table reaches all of this.

Every output is the 16-byte-aligned interior of a larger buffer whose 8 KiB guard bands are compared bitwise afterwards, and starts as NaN: an element
never written, or one written outside its tensor, fails the row.  The bar is TOL32 of tests/test_gpu_f32_fused.py (fp32 accumulation of <= 2304
products); the gather kernels' comparison uses the contraction bar of tests/test_gpu_kernels.py.

LADDER_CLASS_LOOP is read once per process: a fresh child per setting runs the class launches of the 8x32-pixel kernel (upsample-fused forward with
and without the fused 1x1 projection, stride-2 backward-data with 128-channel classes); both settings accumulate every output element in the same
order, so their outputs are also compared bit for bit.

Largest relative errors measured on the MI355X (of the reference's scale; the bar is 3e-6), 56 rows:
  plain 7.6e-7   s2bwd 4.8e-7   up2fwd 6.9e-7   up2fwd_ups 6.4e-7   up2bwd 1.0e-6   s2fwd 6.5e-7
  class launches of the 8x32-pixel kernel, either setting of LADDER_CLASS_LOOP: map 4.6e-7, projection 2.7e-7, stride-2 backward-data 3.2e-7 (same bits)
  ladder_conv2d_fwd on the 20 plain rows: 7.6e-7 (bar 2e-5)
Time: the file takes 27 s (12 s of it the two children); the slowest row, up2bwd_n128_32x16_c16_co160, 1.9 - 2.0 s -- its float64 autograd on the host."""
import functools
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import convf32_cases as R
from test_gpu_f32_fused import TOL32
from test_gpu_split import _lib

pytestmark = pytest.mark.gpu

GATHER_TOL = 2e-5                                     # tests/test_gpu_kernels.py: fp32 kernels against float64, contractions
_worst = {}


def _report(row, errs, seconds):
    e = max(errs.values())
    _worst[row[0]] = max(_worst.get(row[0], 0.0), e)
    print("%s: %s; %.2f s; worst per entry so far: %s" % (R.case_id(row), " ".join("%s=%.3e" % kv for kv in errs.items()), seconds,
                                                          " ".join("%s=%.3e" % kv for kv in sorted(_worst.items()))))


@pytest.mark.parametrize("row", R.CASES, ids=R.case_id)
def test_convf32_every_form_vs_float64(gpu_ctx, row):
    import torch
    L = _lib()
    t0 = time.time()
    f = R.features(row)
    rc, plan = R.plan_query(L, row)
    assert (rc, plan) == (f["family"], R.expected_plan(f)) and R.eligible_query(L, row) == 1
    keep = {}
    errs, _ = R.run_row(L, row, gpu_ctx.stream, keep=keep)
    _report(row, errs, time.time() - t0)
    assert TOL32 == 3e-6
    for name, e in errs.items():
        assert e < TOL32, "%s against float64: rel err %.3e (tol %.1e)" % (name, e, TOL32)
    if row[0] == "plain":                             # the other route a layer can take: the implicit-GEMM forward on the same data
        _, N, h, w, ci, co, act, has_bias = row
        ws = torch.empty(max(L.query("ladder_igemm_fwd_workspace_bytes", N * h * w, 9 * ci, co), 16), dtype=torch.uint8, device="cuda")
        y1 = torch.full((N, h, w, co), float("nan"), device="cuda")
        L.call("ladder_conv2d_fwd", keep["x"].data_ptr(), keep["w"].data_ptr(), keep["b"].data_ptr() if has_bias else None, y1.data_ptr(),
               N, h, w, ci, h, w, co, 3, 3, 1, 1, 1, act, ws.data_ptr(), ws.numel(), gpu_ctx.stream)
        torch.cuda.synchronize()
        _, ref, _ = R.reference(row)
        got = y1.cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all()
        e = float(np.abs(got - ref).max() / np.abs(ref).max())
        print("ladder_conv2d_fwd (kernel id %d) against float64: %.3e" % (L.query("ladder_conv2d_fwd_kernel_id", N, h, w, ci, h, w, co, 3, 3, 1, 1, 1, 1), e))
        assert e < GATHER_TOL, "ladder_conv2d_fwd against float64: rel err %.3e (tol %.1e)" % (e, GATHER_TOL)


@pytest.mark.parametrize("row", R.REFUSED_ROWS, ids=R.case_id)
def test_convf32_below_256_workgroups_is_refused_and_writes_nothing(gpu_ctx, row):
    R.run_refused(_lib(), row, gpu_ctx.stream)


def test_the_runner_notices_a_poisoned_guard_band_and_an_unwritten_output(gpu_ctx):
    """R._host, through which every output above passes, sees one float outside the interior on either side and one NaN left inside it."""
    g = R._Guarded(64, R._NAN_BITS)
    with pytest.raises(AssertionError, match="NaN left"):
        R._host(g, (64,), "y")
    g.t[:] = 1.0
    assert R._host(g, (8, 8), "y").shape == (8, 8)
    g.t[17] = float("nan")
    with pytest.raises(AssertionError, match="NaN left"):
        R._host(g, (64,), "y")
    g.t[17] = float("inf")
    with pytest.raises(AssertionError, match="not finite"):
        R._host(g, (64,), "y")
    g.t[17] = 1.0
    for at in (g.lo - 1, g.lo + g.n, 0, g.bits.numel() - 1):
        saved = g.bits[at].item()
        g.bits[at] = 0
        with pytest.raises(AssertionError, match="guard band"):
            R._host(g, (64,), "y")
        g.bits[at] = saved
        R._host(g, (64,), "y")


_child_died = []                                      # a child that ended on a signal or at its time limit: no further child is started


@functools.lru_cache(maxsize=None)
def _class_loop_child(setting):
    """One fresh child (started with subprocess: the switch is read once per process) runs the class-launch group under LADDER_CLASS_LOOP=<setting>."""
    assert not _child_died, "not started: the child of LADDER_CLASS_LOOP=%s ended on a signal or at its time limit" % _child_died[0]
    env = dict(os.environ)
    env["LADDER_CLASS_LOOP"] = setting
    proc = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "convf32_cases.py"), "class_loop"],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    if proc.returncode < 0 or proc.returncode in (124, 134, 137, 139):
        _child_died.append(setting)
    return proc.returncode, proc.stdout


@pytest.mark.parametrize("setting", ["1", "0"])
def test_convf32_class_loop_settings_vs_float64(setting):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert 'getenv("LADDER_CLASS_LOOP")' in open(os.path.join(root, "ladder_latent_data_distribution_modelling_amd", "csrc", "convf32.hip")).read()
    rc, out = _class_loop_child(setting)
    print(out[-6000:])
    assert rc == 0, "exit status %d under LADDER_CLASS_LOOP=%s:\n%s" % (rc, setting, out[-6000:])
    assert "group class_loop: %d cases, 0 failed" % len(R.CLASS_LOOP) in out
    assert out.count(" family=1 class_loop=%s " % setting) == len(R.CLASS_LOOP)        # the switch took effect, on the 8x32-pixel kernel
    grids = set(re.findall(r" grid=(\d+) ", out))
    assert grids == ({"128"} if setting == "1" else {"512"})                         # patches alone / patches x four class tiles


def test_convf32_class_loop_settings_agree_bit_for_bit():
    """A class tile accumulates its slabs and taps in the same order whether its workgroup runs one class or all four: the outputs are the same bits."""
    digests = []
    for setting in ("1", "0"):
        rc, out = _class_loop_child(setting)
        assert rc == 0, "exit status %d under LADDER_CLASS_LOOP=%s" % (rc, setting)
        digests.append(re.findall(r"case (\d+) .* digest=([0-9a-f]{64})", out))
    assert len(digests[0]) == len(R.CLASS_LOOP) and digests[0] == digests[1]
