"""Importance-weighted log-likelihood without a GPU: the float64 reference (tests/iw_ref.py) against brute force, the agreement of header, ctypes
prototypes and build list on the new exports, their names against the frozen name families, and the refusals that must come before any device use."""
import json
import math
import os
import re

import numpy as np
import pytest

from oracle import ladder_oracle as O

import iw_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IW_EXPORTS = {"ladder_iw_randn_rows", "ladder_iw_sample_rows", "ladder_iw_laplace_rows_workspace_bytes", "ladder_iw_laplace_rows", "ladder_iw_gauss_rows",
              "ladder_iw_add_term", "ladder_iw_accumulate", "ladder_iw_finish"}
# log p(z) of the VampPrior: declared and defined with the rest of the diagonal mixture (csrc/diag_mixture.hip)
DIAG_ROWS_EXPORTS = {"ladder_diag_mixture_logprob_rows_workspace_bytes", "ladder_diag_mixture_logprob_rows"}
DIAG_TERM_EXPORTS = {"ladder_diag_mixture_workspace_bytes", "ladder_diag_mixture_fwd_bwd", "ladder_diag_mixture_wide_workspace_bytes",
                     "ladder_diag_mixture_wide_fwd_bwd"}


# ------------------------------------------------------------------------------------------------ the reference itself
def test_finish_is_the_direct_estimator():
    rng = np.random.default_rng(0)
    logw = rng.normal(-3.0, 2.0, size=(5, 9))
    got = iw_ref.finish(logw)
    w = np.exp(logw)
    np.testing.assert_allclose(got[:, 0], np.log(w.mean(1)), rtol=0, atol=1e-13)
    np.testing.assert_allclose(got[:, 1], logw.mean(1), rtol=0, atol=1e-13)
    np.testing.assert_allclose(got[:, 2], w.sum(1) ** 2 / (w ** 2).sum(1), rtol=1e-13)
    assert (got[:, 3] == 9).all()
    assert (got[:, 1] <= got[:, 0] + 1e-12).all()                            # Jensen: elbo_1 <= log_px per image
    assert ((1.0 - 1e-12 <= got[:, 2]) & (got[:, 2] <= 9.0 + 1e-12)).all()   # 1 <= ess <= S


def test_finish_identities():
    rng = np.random.default_rng(1)
    logw = rng.normal(0.0, 3.0, size=(4, 7))
    base = iw_ref.finish(logw)
    shifted = iw_ref.finish(logw - 70000.0)                                  # a common shift moves log_px and elbo_1, not ess
    np.testing.assert_allclose(shifted[:, 0] + 70000.0, base[:, 0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(shifted[:, 2], base[:, 2], rtol=1e-9)
    const = iw_ref.finish(np.full((2, 6), -12.5))                            # equal weights: log_px = elbo_1 = the weight, ess = S
    np.testing.assert_allclose(const[:, :3], [[-12.5, -12.5, 6.0]] * 2, rtol=0, atol=1e-13)
    one = iw_ref.finish(logw[:, :1])                                         # S = 1: the estimate is the single log-weight
    np.testing.assert_allclose(one[:, 0], logw[:, 0], rtol=0, atol=1e-13)
    holes = logw.copy()
    holes[0, ::2] = -np.inf                                                  # a -inf weight adds 0 but counts in S
    kept = iw_ref.finish(holes)[0]
    assert abs(kept[0] - (math.log(np.exp(logw[0, 1::2]).sum()) - math.log(7))) < 1e-12 and kept[1] == -np.inf
    dead = iw_ref.finish(np.full((1, 3), -np.inf))[0]
    assert dead[0] == -np.inf and dead[2] == 0.0 and not np.isnan(dead).any()


@pytest.mark.parametrize("prior", ["standard_gaussian", "GMM", "vampPrior", "ours", "hierarchical"])
def test_terms_against_brute_force(golden_dir, prior):
    """Every term of the reference, recomputed sample by sample with plain numpy formulas from the oracle's network outputs."""
    d = np.load(os.path.join(golden_dir, "oracle_mnist_digit.npz"))
    cfg = json.loads(str(d["config"]))
    cfg.update(prior=prior, representation_size=3, n_mixtures=4)
    B, S, Z, R = 2, 3, cfg["code_size"], 3
    rng = np.random.default_rng(5)
    x = rng.random((B, 28, 28, 1))
    P = O.init_params(cfg, seed=4)
    P["encoder/code_std_dev/bias"] = (P["encoder/code_std_dev/bias"] + 0.4).astype(np.float32)
    gm = O.synthetic_gm(dict(n_mixtures=4, representation_size=Z if prior == "GMM" else R), rng)
    eps_z, eps_t = rng.standard_normal((S, B, Z)), rng.standard_normal((S, B, R))
    sigma = 0.37
    got = iw_ref.terms(cfg, P, x, eps_z, eps_t, gm, sigma)
    import torch
    P64 = {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in P.items()}
    mu, sd = (a.numpy() for a in O.encoder(cfg, P64, torch.as_tensor(x)))
    isg = iw_ref.inner_sigma(cfg, P) if prior in ("ours", "hierarchical") else None

    def mvn(v, m, c):
        dv = v - m
        return -0.5 * dv @ np.linalg.solve(c, dv) - 0.5 * np.linalg.slogdet(c)[1] - 0.5 * len(v) * math.log(2 * math.pi)

    def mix(v):
        return math.log(sum(w / gm["weights"].sum() * math.exp(mvn(v, m, c)) for w, m, c in zip(gm["weights"], gm["means"], gm["covs"])))

    for b in range(B):
        for s in range(S):
            z = mu[b] + sd[b] * eps_z[s, b]
            xh = O.decoder(cfg, P64, torch.as_tensor(z[None])).numpy().reshape(-1)
            want = {"log_px_z": -np.abs(x[b].reshape(-1) - xh).sum() / sigma - 784 * math.log(2 * sigma),
                    "log_qz": sum(-0.5 * e * e - math.log(q) - 0.5 * math.log(2 * math.pi) for e, q in zip(eps_z[s, b], sd[b]))}
            if prior == "standard_gaussian":
                want["log_pz"] = mvn(z, np.zeros(Z), np.eye(Z))
            elif prior == "GMM":
                want["log_pz"] = mix(z)
            elif prior == "vampPrior":
                mp, sp = (a.numpy() for a in O.encoder(cfg, P64, P64["prior/Variable"]))
                want["log_pz"] = math.log(np.mean([math.exp(mvn(z, m, np.diag(q ** 2))) for m, q in zip(mp, sp)]))
            else:
                mt, st = (a.numpy()[0] for a in O.inner_encoder(cfg, P64, torch.as_tensor(z[None])))
                t = mt + st * eps_t[s, b]
                zh = O.inner_decoder(cfg, P64, torch.as_tensor(t[None])).numpy()[0]
                want["log_pz"] = mvn(z, zh, isg ** 2 * np.eye(Z))
                want["log_qt"] = mvn(t, mt, np.diag(st ** 2))
                want["log_pt"] = mix(t) if prior == "ours" else mvn(t, np.zeros(R), np.eye(R))
            assert set(want) == set(got) - {"z", "logw"}
            for k, v in want.items():
                assert abs(got[k][b, s] - v) <= 1e-9 * max(1.0, abs(v)), (k, b, s, got[k][b, s], v)
            lw = want["log_px_z"] + want["log_pz"] + want.get("log_pt", 0.0) - want["log_qz"] - want.get("log_qt", 0.0)
            assert abs(got["logw"][b, s] - lw) <= 1e-9 * abs(lw)
            np.testing.assert_allclose(got["z"][b, s], z, rtol=0, atol=1e-12)
    fin = iw_ref.finish(got["logw"])
    assert (fin[:, 1] <= fin[:, 0] + 1e-12).all()


# ------------------------------------------------------------------------------------------------ the surface of the kernels
def test_header_prototypes_and_sources_agree():
    from ladder_latent_data_distribution_modelling_amd import _lib
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    header = open(os.path.join(ROOT, "include", "ladder_hip.h")).read()
    section = header[header.index("N25: importance-weighted marginal log-likelihood"):]
    section = section[:section.index("/* ----", 10)]
    diag = header[header.index("/* ---- diagonal mixture (csrc/diag_mixture.hip)"):]
    diag = diag[:diag.index("/* ----", 10)]
    names = lambda text: set(re.findall(r"^(?:int|size_t) (ladder_[a-z0-9_]+)\(", text, re.M))
    assert names(section) == IW_EXPORTS
    assert names(diag) == DIAG_ROWS_EXPORTS | DIAG_TERM_EXPORTS             # one section for the whole family
    assert len(re.findall(r"ladder_diag_mixture[a-z_]*\(", header)) == 6     # ... and each declared there only
    assert {n for n in _lib.PROTOTYPES if n.startswith("ladder_iw_")} == IW_EXPORTS
    assert {n for n in _lib.PROTOTYPES if n.startswith("ladder_diag_mixture_")} == DIAG_ROWS_EXPORTS | DIAG_TERM_EXPORTS
    for name, text in [(n, section) for n in IW_EXPORTS] + [(n, diag) for n in DIAG_ROWS_EXPORTS]:   # one ctypes argument per declared parameter
        decl = re.search(r"^(?:int|size_t) %s\(([^;]*)\);" % name, text, re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.PROTOTYPES[name][1]), name
        assert _lib.PROTOTYPES[name][0] is (_lib._z if name.endswith("_bytes") else _lib._i)
        assert _lib.PROTOTYPES[name][1][-1] is _lib._p or name.endswith("_bytes")      # every launch takes the stream last
    for cite in ("codes/base.py:383-396", "codes/models.py:97-103", "codes/base.py:216-254", "codes/base.py:286-297"):
        assert cite in section, cite
    assert "codes/base.py:216-254" in diag
    assert re.search(r"#define LADDER_ABI_VERSION (\d+)", header).group(1) == "2" == str(_lib.ABI_VERSION)
    assert "iwll.hip" in build.SOURCES and "diag_mixture.hip" in build.SOURCES
    csrc = os.path.join(ROOT, "ladder_latent_data_distribution_modelling_amd", "csrc")
    source, mixture = open(os.path.join(csrc, "iwll.hip")).read(), open(os.path.join(csrc, "diag_mixture.hip")).read()
    assert names(source[source.index('extern "C"'):]) == IW_EXPORTS
    assert names(mixture[mixture.index('extern "C"'):]) == DIAG_ROWS_EXPORTS | DIAG_TERM_EXPORTS
    assert "atomic" not in source.replace("no atomics", "")                  # every sum has one fixed order
    assert "atomic" not in mixture.replace("No floating-point atomics", "")
    # the component arithmetic of the rows and of the wide term is written ONCE: one scoring loop, called by both kernels, one log s in the prepare kernel
    assert mixture.count("dm_score_chunk(t, m, is, c, ") == 2 and mixture.count("fmaf(-0.5f, wave_sum(") == 1 and mixture.count("logf(s)") == 1
    assert "diag_mixture" not in source and "wave_sum(" not in source and "logf(s)" not in source


def test_new_names_stay_out_of_the_frozen_families():
    from test_mixture_forms_cpu import MIXTURE_PREFIXES
    from ladder_latent_data_distribution_modelling_amd import mixture_forms
    for name in IW_EXPORTS:
        assert not name.startswith(MIXTURE_PREFIXES) and not name.startswith("ladder_pairs_"), name
    table = open(mixture_forms.__file__).read()
    assert not any(name in table for name in IW_EXPORTS | DIAG_ROWS_EXPORTS)  # (the rows export has one form: nothing to select)


# ------------------------------------------------------------------------------------------------ refusals before the device
def test_refusals_come_before_the_device(monkeypatch, tmp_path):
    from ladder_latent_data_distribution_modelling_amd import _lib, evaluate
    from ladder_latent_data_distribution_modelling_amd import log_likelihood as LL
    from ladder_latent_data_distribution_modelling_amd.codes.base import BaseTrain_joint as BaseTrain

    def boom(*_a, **_k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(_lib, "load", boom)
    x = np.zeros((4, 28, 28, 1), np.float32)
    for prior in ("ours", "GMM"):
        tr = BaseTrain.__new__(BaseTrain)
        tr.config, tr.gm_params, tr.cur_epoch, tr.flush = dict(prior=prior, result_dir=str(tmp_path) + "/"), None, 1, boom
        for mode in ("accurate-GM", "crude-GM"):
            with pytest.raises(RuntimeError, match="has not been fitted"):
                tr.estimate_log_likelihood(x, n_samples=4, mode=mode)
        tr.gm_params = object()                                              # the per-epoch fit exists, the accurate one does not
        with pytest.raises(RuntimeError, match="accurate mixture, which has not been fitted"):
            tr.estimate_log_likelihood(x, n_samples=4)
    tr = BaseTrain.__new__(BaseTrain)
    tr.config, tr.gm_params, tr.cur_epoch, tr.flush = dict(prior="standard_gaussian", result_dir=str(tmp_path) + "/"), None, 1, boom
    for kw in (dict(n_samples=0), dict(rows=0), dict(n_samples=-3)):
        with pytest.raises(ValueError, match="n_samples >= 1 and rows >= 1"):
            tr.estimate_log_likelihood(x, **kw)
    with pytest.raises(ValueError, match=r"\[N, H, W, C\]"):
        tr.estimate_log_likelihood(x[0], n_samples=2)

    class It:
        def next(self):
            raise AssertionError("no batch may be drawn")

    with pytest.raises(ValueError, match="max_images"):
        tr.estimate_log_likelihood(It(), n_samples=2)
    assert not os.listdir(str(tmp_path))
    # the command line: defaults, and what it refuses
    a = evaluate.parse_args(["--config", "c.json"])
    assert (a.n_samples, a.rows, a.images, a.max_images, a.sigma, a.seed) == (5000, 128, None, None, None, 0)
    for bad in (["--n-samples", "0"], ["--rows", "0"], ["--max-images", "0"], ["--sigma", "0"], ["--sigma", "-1"]):
        with pytest.raises(SystemExit):
            evaluate.parse_args(["--config", "c.json"] + bad)
    assert LL.TERMS == ("log_px_z", "log_pz", "log_pt", "log_qz", "log_qt") and set(LL.TERMS) == set(iw_ref.SIGNS)
