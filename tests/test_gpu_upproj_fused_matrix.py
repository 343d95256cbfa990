"""The fused pair forward (csrc/upproj.hip: up2proj_fused_fwd_kernel, up2proj_fused2_fwd_kernel) against the float64 oracle on EVERY case of
tests/upproj_fused_ref.py: every remainder of the unrolled stage rings on both sides of the hand-over, both workgroup mappings, every width, the
resident and the streamed weight slab, the 128-pixel kernel with odd chunk counts, and the projection epilogue in every form the ABI allows (pco
1 .. 4, with and without the map, bias == NULL, proj_b == NULL, act == 0, a proj_out that is only 4-byte aligned: the scalar reduction).
tests/test_upproj_fused_cases_cpu.py proves that the table reaches all of this.

Per case of the 64-pixel kernel: variant masks 3, 2, 1, 0 of ladder_up2proj_fused_fwd_variant and the default entry ladder_up2proj_fused_fwd; mask 3
against float64 at TOL32 = 3e-6 of the reference's scale (the bar tests/test_gpu_upproj.py derives for K = Cin <= 512; every Cin here is <= 256), all
others bit-identical to mask 3.  Per case of the 128-pixel kernel: float64 at TOL32 and a bit-identical second launch.  Every launch writes into
16-byte-aligned interiors of larger buffers whose 8 KiB guard bands are compared bitwise afterwards; outputs start as NaN and the workspace as 0xFF
bytes, so an element or a partial that is never written, or one written outside its tensor, fails the case.

LADDER_UP2FUSE_NO_WRES and LADDER_UP2FUSE_NO_PT2 are read once per process: one fresh child each runs a whole group of the table under the switch.

Largest relative errors measured on the MI355X (of the reference's scale; the bar is 3e-6):
  64-pixel kernel   map 4.7e-7   projection 3.7e-7
  128-pixel kernel  map 3.9e-7   (it has no projection)
  under LADDER_UP2FUSE_NO_WRES=1 (resident group)  map 2.9e-7   projection 2.6e-7
  under LADDER_UP2FUSE_NO_PT2=1  (wide group)      map 3.9e-7"""
import os
import subprocess
import sys

import pytest

import test_gpu_upproj
import upproj_fused_ref as R
from test_gpu_split import _lib

pytestmark = pytest.mark.gpu

PX64 = R.GROUPS["resident"] + R.GROUPS["streamed"]
_seen = {"px64": [], "wide": []}
_child_died = []                                      # a child that ended on a signal or at its time limit: no further child is started


def _report(kind, e):
    _seen[kind].append(e)
    w = R.worst(_seen[kind])
    print("%s: this case map %s projection %s; worst so far map %s projection %s" % (kind, e["map"], e["proj"], w["map"], w["proj"]))


def _hold(e, case):
    assert R.TOL32 == test_gpu_upproj.TOL32 == 3e-6
    assert (e["map"] is not None) == bool(case[6]) and (e["proj"] is not None) == bool(case[5])
    if case[6]:
        assert e["map"] < R.TOL32, "map against float64: rel err %.3e (tol %.1e)" % (e["map"], R.TOL32)
    if case[5]:
        assert e["proj"] < R.TOL32, "projection against float64: rel err %.3e (tol %.1e)" % (e["proj"], R.TOL32)


@pytest.mark.parametrize("case", PX64, ids=R.case_id)
def test_upproj_fused_px64_every_form_vs_float64(gpu_ctx, case):
    L = _lib()
    assert L.query("ladder_up2proj_fused_eligible", *case[:5]) == 1
    assert L.query("ladder_up2proj_fused_wide_tile", *case[:5]) == 0
    e = R.run_case(L, case, gpu_ctx.stream, masks=(3, 2, 1, 0, None))
    _report("px64", e)
    _hold(e, case)


@pytest.mark.parametrize("case", R.GROUPS["wide"], ids=R.case_id)
def test_upproj_fused_wide_tile_vs_float64(gpu_ctx, case):
    L = _lib()
    assert L.query("ladder_up2proj_fused_wide_tile", *case[:5]) == 1
    e = R.run_case(L, case, gpu_ctx.stream, masks=(None, None))
    _report("wide", e)
    _hold(e, case)


def test_guard_bands_and_poison_are_noticed(gpu_ctx):
    """The runner's own checks see one float written one element outside an interior, on either side, aligned or not."""
    import torch
    for shift in (0, 1):
        g = R._Guarded(64, R._NAN_BITS, shift=shift)
        assert g.guards_intact() and bool(torch.isnan(g.t).all().item()) and g.t.numel() == 64
        assert g.t.data_ptr() - g.bits.data_ptr() >= 4096 and (g.bits.numel() - g.lo - g.n) * 4 >= 4096
        g.t[0], g.t[63] = 1.0, 2.0                                         # the interior's own ends: not a guard
        assert g.guards_intact()
        for at in (g.lo - 1, g.lo + g.n, 0, g.bits.numel() - 1):
            saved = g.bits[at].item()
            g.bits[at] = 0
            assert not g.guards_intact(), at
            g.bits[at] = saved
            assert g.guards_intact()


@pytest.mark.parametrize("switch,group", [("LADDER_UP2FUSE_NO_WRES", "resident"), ("LADDER_UP2FUSE_NO_PT2", "wide")])
def test_upproj_fused_process_wide_switches_vs_float64(switch, group):
    """One fresh child runs the group under the switch (tests/upproj_fused_ref.py <group>: every mask and the default entry, float64 at TOL32, guard
    bands, poisoned workspace).  A child that ends on a signal or at its time limit fails the test; nothing is started after it."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert 'getenv("%s")' % switch in open(os.path.join(root, "ladder_latent_data_distribution_modelling_amd", "csrc", "upproj.hip")).read()
    assert not _child_died, "not started: the child of %s ended on a signal or at its time limit" % _child_died[0]
    env = dict(os.environ)
    env[switch] = "1"
    proc = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "upproj_fused_ref.py"), group],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(proc.stdout[-6000:])
    if proc.returncode < 0 or proc.returncode in (124, 134, 137, 139):
        _child_died.append(switch)
    assert proc.returncode == 0, "exit status %d under %s=1:\n%s" % (proc.returncode, switch, proc.stdout[-6000:])
    assert "group %s: %d cases, 0 failed" % (group, len(R.GROUPS[group])) in proc.stdout
    if group == "wide":
        assert " wide_tile=1 " not in proc.stdout and proc.stdout.count(" wide_tile=0 ") == len(R.GROUPS[group])    # the switch took effect
