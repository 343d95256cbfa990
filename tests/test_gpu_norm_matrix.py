"""The HBM-bound passes of csrc/norm.hip -- batch-norm and instance-norm statistics and apply passes, both column-statistics stages, the legacy bilinear
resize, depth-to-space, the symmetric pad and the activation backward -- against float64 on EVERY row of tests/norm_cases.py, through the public entry
points: every host-side route (float4 / scalar, fold / finalise + apply, parameter gradients riding or on their own, workspace / no workspace, tensors that
start one float past a 16-byte boundary), one and two sweeps of every grid-stride loop with `fixed` and `!fixed` coefficients, the 8-row batch loop and
its tail of the first statistics stage on both sides of their boundaries and under the 512-block cap, the second stage alone on synthetic partials, the
instance-norm pivot on channels whose mean lies 50 standard deviations off zero (also with the zeroed corner pixel), every in_split outcome, non-square
resizes with fy != fx and more than one workgroup per source row.  tests/test_norm_cases_cpu.py proves that the table reaches all of this.

Every buffer is the interior of a larger allocation whose 8 KiB guard bands are compared bitwise after every launch; outputs start as NaN and workspaces
as 0xFF bytes: an element never written, or one written outside its tensor, fails the row.

THE METRIC for y, dx and `up` is per channel -- the channel's largest error over the channel's largest |reference| -- at the bars the project states for
these kernels: y 1e-5; dx 2e-5 (batch norm), 5e-5 (instance norm); dgamma / dbeta / dstyle 2e-5 of their own vector's scale.  All of them are the STATED
bars: the fp32 numpy restatement of the formulas (mean and 1 / sd rounded to fp32, the expression of csrc/norm_util.h) stays within a quarter of each on
every row (its largest errors: batch norm y 2.6e-7, dx 1.8e-7, dgamma 1.8e-7, dbeta 1.9e-7; instance norm y 1.9e-6, dx 8.7e-7, dstyle 2.4e-6), so no
row's bar is a measured one.  The forward statistics are read as doubles and held to the worst case of an fp64 sum in any order,
|got - ref| <= rows * 2^-52 * sum |term| per channel, extremes bit for bit; the fp32 backward sums to 2e-5 of sum |term| per channel; resize and the pad's
transpose to 1e-6; depth-to-space and the pad exactly; ladder_act_bwd to three fp32 roundings, in place (dx == dy) bit-identical to out of place.

Largest errors measured on the MI355X, 184 cases (instance norm per route: workspace / ws == NULL / x shifted by one float):
  batch norm      y 1.9e-7   dx 1.8e-7   dgamma 3.2e-7   dbeta 4.1e-7                                       (bars 1e-5, 2e-5, 2e-5, 2e-5)
  instance norm   y 2.9e-6 / 7.3e-6 / 7.3e-6   up 2.0e-6   dx 2.5e-6 on every route   dstyle 4.5e-6 / 1.5e-5 / 1.5e-5    (bars 1e-5, 1e-5, 5e-5, 2e-5)
    (the one-workgroup kernels come nearest their bars on (1, 17, 241, 4): 4097 pixels 50 sd off zero summed by 4 row lanes in fp32 -- y 7.3e-6,
    dstyle 1.5e-5 where the split path has 7.1e-7 and 6.6e-7; the zeroed-corner row: y 5.5e-7)
  forward sums 3.1e-2 of the fp64 worst-case bound (525288 rows: 1.3e-5 of it), second stage alone: every sum exact; backward sums 1.1e-7 (bar 2e-5)
  resize y 9.1e-8, dx 1.3e-7; pad transpose 8.7e-8 (bars 1e-6); ladder_act_bwd 0.37 of its three-rounding bound, in place == out of place on every row
Time: the file takes 7 s; the slowest row, bn-33000-96-leaky_relu-plain, 1.4 s (its float64 autograd on the host; the other rows <= 0.3 s)."""
import time

import pytest

import norm_cases as R
from test_gpu_split import _lib

pytestmark = pytest.mark.gpu

_worst = {}
STATED = {"bn": dict(y=1e-5, dx=2e-5, dgamma=2e-5, dbeta=2e-5), "in": dict(y=1e-5, up=1e-5, dx=5e-5, dstyle=2e-5)}


def _report(row, errs, bars, rest, seconds):
    for k, e in errs.items():
        key = "%s.%s" % (row[0], k)
        _worst[key] = max(_worst.get(key, 0.0), e)
    print("%s: %s; restatement %s; %.2f s" % (R.case_id(row), " ".join("%s=%.3e(<%.1e)" % (k, e, bars[k]) for k, e in errs.items()),
                                             " ".join("%s=%.2e" % kv for kv in rest.items()) or "-", seconds))
    print("worst so far: %s" % " ".join("%s=%.3e" % kv for kv in sorted(_worst.items())))


@pytest.mark.parametrize("row", R.CASES, ids=R.case_id)
def test_norm_every_route_vs_float64(gpu_ctx, row):
    t0 = time.time()
    errs, bars, rest = R.run_row(_lib(), row, gpu_ctx.stream)
    _report(row, errs, bars, rest, time.time() - t0)
    assert set(errs) == set(bars)
    for name, e in errs.items():
        if row[0] in STATED:                          # the stated bar, or four times the fp32 restatement's own error where that takes a quarter of it
            q = name.split("/")[0]                    # (instance norm reports quantity/route)
            assert bars[name] == R.row_bar(STATED[row[0]][q], rest["y" if q == "up" else q])
        assert e < bars[name], "%s of %s: %.3e (bar %.1e)" % (name, R.case_id(row), e, bars[name])


def test_the_runner_notices_a_poisoned_guard_band_and_an_unwritten_output(gpu_ctx):
    """R._host and R._Bufs.check, through which every buffer above passes, see one float outside an interior on either side and one NaN left inside it."""
    B = R._Bufs()
    g = B.out(64, "y", 1)
    with pytest.raises(AssertionError, match="NaN left"):
        R._host(g, (64,), "y")
    g.t[:] = 1.0
    assert R._host(g, (8, 8), "y").shape == (8, 8) and not R._untouched(g)
    g.t[17] = float("inf")
    with pytest.raises(AssertionError, match="not finite"):
        R._host(g, (64,), "y")
    g.t[17] = 1.0
    w = B.ws(64, "workspace")
    for buf in (g, w):
        for at in (buf.lo - 1, buf.lo + buf.n, 0, buf.bits.numel() - 1):
            saved = buf.bits[at].item()
            buf.bits[at] = 0
            with pytest.raises(AssertionError, match="guard band"):
                B.check("a poisoned band")
            buf.bits[at] = saved
            B.check("restored")
