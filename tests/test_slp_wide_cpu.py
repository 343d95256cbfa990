"""Host side of the wide (8 < R <= 64) batched shortest-likely-path interpolation (no GPU): the new refusals of
SLPInterpolator / optimise_batch and of the trainer's interpolate_paths raise before anything touches the device, and the header, the
ctypes prototypes and the limits the Python layer enforces agree on the two new entry points."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slp(R, K=5, dense=True):
    """An interpolator without a device (as test_slp_batch_cpu._slp): the checks under test run before the engine is used."""
    from ladder_latent_data_distribution_modelling_amd.codes.interpolation import SLPInterpolator
    slp = object.__new__(SLPInterpolator)
    slp.eng, slp.K, slp.R, slp.mixture = None, K, R, types.SimpleNamespace(dense=dense)
    return slp


def test_optimise_batch_rejects_paths_beyond_the_wide_limit():
    from ladder_latent_data_distribution_modelling_amd.codes import interpolation as I
    assert I.MAX_POINTS_WIDE == 2048
    ok = np.zeros((3, 64))
    with pytest.raises(ValueError, match=r"33 \* 64 = 2112 exceeds 2048"):
        _slp(64).optimise_batch(ok, ok, n_step=33)
    with pytest.raises(ValueError, match=r"57 \* 36 = 2052 exceeds 2048"):
        _slp(36).optimise_batch(np.zeros((1, 36)), np.zeros((1, 36)), n_step=57)
    with pytest.raises(ValueError, match=r"n_step must be in 1\.\.64"):
        _slp(16).optimise_batch(np.zeros((1, 16)), np.zeros((1, 16)), n_step=65)
    # at the limit the shape check passes: the next check (n_iter) is the one that raises
    with pytest.raises(ValueError, match="n_iter"):
        _slp(64).optimise_batch(ok, ok, n_step=32, n_iter=0)
    with pytest.raises(ValueError, match="n_iter"):
        _slp(32).optimise_batch(np.zeros((2, 32)), np.zeros((2, 32)), n_step=64, n_iter=0)


def test_interpolator_rejects_wide_r_not_a_multiple_of_4():
    from ladder_latent_data_distribution_modelling_amd.codes.interpolation import SLPInterpolator
    for R in (10, 63, 68):
        with pytest.raises(ValueError, match=r"R % 4 == 0"):
            SLPInterpolator(None, np.ones(3) / 3, np.zeros((3, R)), np.stack([np.eye(R)] * 3))


def test_interpolate_paths_accepts_wide_ours():
    from ladder_latent_data_distribution_modelling_amd.codes.base import BaseTrain_joint as BaseTrain
    tr = types.SimpleNamespace(config=dict(prior="ours", representation_size=16), gm_params=None)
    for bad in ((np.zeros((2, 2)), np.zeros((2, 2))), (np.zeros((2, 16)), np.zeros((3, 16))), (np.zeros(16), np.zeros(16))):
        with pytest.raises(ValueError, match=r"\[P, 16\] points of the mixture on the representation"):
            BaseTrain.interpolate_paths(tr, *bad)
    z = np.zeros((2, 16))
    for mode, which in (("crude-GM", "per-epoch"), ("accurate-GM", "accurate")):
        with pytest.raises(RuntimeError, match="needs the %s mixture, which has not been fitted" % which):
            BaseTrain.interpolate_paths(tr, z, z, mode=mode)
    for R in (10, 68, 0):
        tr = types.SimpleNamespace(config=dict(prior="ours", representation_size=R), gm_params=None)
        with pytest.raises(ValueError, match=r"R % 4 == 0"):
            BaseTrain.interpolate_paths(tr, np.zeros((2, R)), np.zeros((2, R)))


def test_header_prototypes_and_python_limits_agree():
    from ladder_latent_data_distribution_modelling_amd import _lib
    from ladder_latent_data_distribution_modelling_amd.codes import interpolation as I
    header = open(os.path.join(ROOT, "include", "ladder_hip.h")).read()
    for name in ("ladder_slp_wide_state_bytes", "ladder_slp_wide_optimise"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.PROTOTYPES
    decl = re.search(r"int ladder_slp_wide_optimise\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.PROTOTYPES["ladder_slp_wide_optimise"][1]) == 20
    assert _lib.PROTOTYPES["ladder_slp_wide_optimise"] == _lib.PROTOTYPES["ladder_slp_optimise"]
    assert _lib.PROTOTYPES["ladder_slp_wide_state_bytes"] == _lib.PROTOTYPES["ladder_slp_state_bytes"]
    wide = header[header.index("ladder_slp_wide_optimise: "):] if "ladder_slp_wide_optimise: " in header else header[header.index("csrc/slp_wide.hip"):]
    wide = wide[:wide.index("size_t ladder_slp_wide_state_bytes")]
    for limit in ("8 < R <= 64", "R % 4 == 0", "1 <= K <= 1024", "1 <= n_step <= %d" % I.MAX_STEP, "n_step * R <= %d" % I.MAX_POINTS_WIDE,
                  "1 <= n_iter <= %d" % I.MAX_ITER_PER_LAUNCH, "t0 >= 0"):
        assert limit in wide, limit
    assert int(re.search(r"#define LADDER_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 2
