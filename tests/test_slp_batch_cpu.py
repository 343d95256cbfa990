"""Host side of the batched shortest-likely-path interpolation (no GPU): the argument checks of SLPInterpolator.optimise_batch /
decode_paths and of the trainer's interpolate_paths raise before anything touches the device, and the header, the ctypes prototypes and
the limits the Python layer enforces agree on the new entry points."""
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _slp(R=2, K=5):
    """An interpolator without a device: the checks under test run before the engine is used."""
    from ladder_latent_data_distribution_modelling_amd.codes.interpolation import SLPInterpolator
    slp = object.__new__(SLPInterpolator)
    slp.eng, slp.K, slp.R, slp.mixture = None, K, R, None
    return slp


def test_optimise_batch_rejects_bad_shapes():
    slp = _slp(R=2)
    ok = np.zeros((3, 2))
    with pytest.raises(ValueError, match=r"\[P, R\]"):
        slp.optimise_batch(ok, np.zeros((4, 2)))                              # starts / ends mismatch
    with pytest.raises(ValueError, match=r"\[P, R\]"):
        slp.optimise_batch(np.zeros(2), np.zeros(2))                          # one pair, not a batch
    with pytest.raises(ValueError, match="mixture has R = 2"):
        slp.optimise_batch(np.zeros((3, 3)), np.zeros((3, 3)))                # R not the mixture's
    for n_step in (0, 65, -1):
        with pytest.raises(ValueError, match=r"n_step must be in 1\.\.64"):
            slp.optimise_batch(ok, ok, n_step=n_step)
    with pytest.raises(ValueError, match="n_iter"):
        slp.optimise_batch(ok, ok, n_iter=0)
    with pytest.raises(ValueError, match="init must be"):
        slp.optimise_batch(ok, ok, n_step=5, init=np.zeros((3, 4, 2)))


def test_decode_paths_rejects_bad_shapes():
    slp = _slp(R=2)
    s, p = np.zeros((3, 2)), np.zeros((3, 5, 2))
    with pytest.raises(ValueError, match="whole path"):
        slp.decode_paths(s, p, s, chunk=6)                                    # chunk < n_step + 2
    with pytest.raises(ValueError, match="expected"):
        slp.decode_paths(np.zeros((2, 2)), p, s)


def test_interpolate_paths_rejects_priors_without_a_narrow_t_mixture():
    from ladder_latent_data_distribution_modelling_amd.codes.base import BaseTrain_joint as BaseTrain
    z = np.zeros((2, 2))
    for cfg in (dict(prior="GMM", representation_size=2), dict(prior="standard_gaussian", representation_size=2),
                dict(prior="vampPrior", representation_size=2), dict(prior="hierarchical", representation_size=2),
                dict(prior="ours", representation_size=16)):
        tr = types.SimpleNamespace(config=cfg, gm_params=None)
        with pytest.raises(ValueError, match="mixture on the representation"):
            BaseTrain.interpolate_paths(tr, z, z)
    for mode, which in (("crude-GM", "per-epoch"), ("accurate-GM", "accurate")):
        tr = types.SimpleNamespace(config=dict(prior="ours", representation_size=2), gm_params=None)
        with pytest.raises(RuntimeError, match="needs the %s mixture, which has not been fitted" % which):
            BaseTrain.interpolate_paths(tr, z, z, mode=mode)


def test_header_prototypes_and_python_limits_agree():
    from ladder_latent_data_distribution_modelling_amd import _lib
    from ladder_latent_data_distribution_modelling_amd.codes import interpolation as I
    import codes.interpolation as alias
    header = open(os.path.join(ROOT, "include", "ladder_hip.h")).read()
    for name in ("ladder_slp_state_bytes", "ladder_slp_optimise"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in _lib.PROTOTYPES
    decl = re.search(r"int ladder_slp_optimise\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_lib.PROTOTYPES["ladder_slp_optimise"][1]) == 20
    assert "1 <= n_step <= %d" % I.MAX_STEP in header and "1 <= n_iter <= %d" % I.MAX_ITER_PER_LAUNCH in header
    assert int(re.search(r"#define LADDER_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 2
    assert alias.SLPInterpolator is I.SLPInterpolator and hasattr(alias.SLPInterpolator, "optimise_batch") and hasattr(alias.SLPInterpolator, "decode_paths")
