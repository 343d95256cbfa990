"""The importance-weighted log-likelihood end to end (log_likelihood.ImportanceEstimator, trainer.estimate_log_likelihood, evaluate.py) against the
float64 reference tests/iw_ref.py, on the tiny configurations of tests/golden with oracle-initialised parameters, as tests/test_gpu_model.py builds its engines.

Tolerances are not chosen here.  Every term vector is held, row by row, to the bar at which tests/test_gpu_model.py already holds the matching ELBO scalar
against the float64 oracle, |got - ref| <= rtol |ref| + 1e-4 (its `_ok`), read as an absolute bound on the row value:

    log_px_z  reconstruction_likelihood (+ sigma_regularisor)      log_qz  entropy_z          log_qt  entropy_t
    log_pz    code_reconstruction_likelihood (inner priors), crossEntropy_prior (GMM, vampPrior, standard_gaussian: crossEntropy_prior_sg)
    log_pt    crossEntropy_representation

with rtol the one of the test that covers the configuration (RTOL below).  log_px per image then gets the sum of the term bounds of its worst sample and
nothing more: logsumexp is 1-Lipschitz in the max norm.  The measured deviations are printed (and recorded in DESIGN.md)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ladder_oracle as O

import iw_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-4                        # tests/test_gpu_model.py::_ok
RTOL = {                           # the test of tests/test_gpu_model.py that holds this configuration's scalars to the float64 oracle
    "ours": 2e-5,                  # test_golden_two_iterations, iteration 0
    "standard_gaussian": 2e-5,     # test_golden_two_iterations, iteration 0: reconstruction_likelihood, entropy_z, crossEntropy_prior_sg
    "ours-R16": 5e-5,              # test_two_rung_r8_k50_vs_oracle: another representation size and mixture tier
    "hierarchical": 5e-5,          # test_hierarchical_prior_vs_oracle
    "GMM": 5e-5,                   # test_gmm_prior_on_z_vs_oracle
    "vampPrior": 5e-5,             # test_vamp_prior_vs_oracle
}


def _engine(cfg, values):
    from ladder_latent_data_distribution_modelling_amd.engine import LadderEngine
    return LadderEngine(cfg, "cuda:0", values=values, seed=1)


def _setup(golden_dir, exp, prior, R, seed):
    d = np.load(os.path.join(golden_dir, "oracle_%s.npz" % exp))
    cfg = json.loads(str(d["config"]))
    cfg.update(prior=prior, representation_size=R, n_mixtures=5)
    rng = np.random.default_rng(seed)
    P = O.init_params(cfg, seed=seed)
    # a usable posterior width: the std head of an untrained encoder sits at its 1e-3 floor, where all samples of an image coincide
    P["encoder/code_std_dev/bias"] = (P["encoder/code_std_dev/bias"] + 0.4).astype(np.float32)
    if prior == "vampPrior":
        P["prior/Variable"] = (0.5 + 0.25 * P["prior/Variable"]).astype(np.float32)
    gm = None
    if prior in ("ours", "GMM"):
        gm = {k: v.astype(np.float32) for k, v in O.synthetic_gm(dict(n_mixtures=5, representation_size=R if prior == "ours" else cfg["code_size"]), rng).items()}
    return cfg, P, gm, rng


def _compare(cfg, P, gm, rng, B, S, rows, rtol, what):
    from ladder_latent_data_distribution_modelling_amd.log_likelihood import ImportanceEstimator
    Z, R = cfg["code_size"], cfg["representation_size"]
    x = rng.random((B, cfg["dim_input_x"], cfg["dim_input_y"], cfg["dim_input_channel"])).astype(np.float32)
    noise = dict(eps_z=rng.standard_normal((S, B, Z)).astype(np.float32), eps_t=rng.standard_normal((S, B, R)).astype(np.float32))
    eng = _engine(cfg, P)
    est = ImportanceEstimator(eng, None if gm is None else (gm["weights"], gm["means"], gm["covs"]))
    assert est.sigma == abs(float(np.asarray(P["sigma/Variable"]).reshape(-1)[0]))          # a fixed number: |sigma/Variable|, read once
    out, terms = est.estimate_batch(x, S, rows=rows, noise=noise, return_terms=True)
    assert eng.ctx.keep_activations is True
    ref = iw_ref.terms(cfg, P, x, noise["eps_z"], noise["eps_t"], gm, est.sigma)
    assert set(terms) == set(ref)
    total = np.zeros((B, S))
    for k in iw_ref.SIGNS:
        if k not in ref:
            continue
        bound = rtol * np.abs(ref[k]) + ATOL
        err = np.abs(terms[k] - ref[k])
        total += bound
        print("%s %-8s max |dev| %.3e at |ref| %.3e (bound there %.3e; worst dev / bound %.3f)"
              % (what, k, err.max(), np.abs(ref[k]).reshape(-1)[err.argmax()], bound.reshape(-1)[err.argmax()], (err / bound).max()))
        assert terms[k].shape == (B, S) and (err <= bound).all(), (what, k, err.max())
    assert np.abs(terms["z"].astype(np.float64) - ref["z"]).max() < 1e-4          # the code_sample bar of test_golden_two_iterations
    fin = iw_ref.finish(ref["logw"])
    dev_px = np.abs(out[:, 0] - fin[:, 0])
    print("%s log_px   max |dev| %.3e (bound %.3e), log_px %s, ess %s" % (what, dev_px.max(), total.max(1)[dev_px.argmax()], np.round(out[:, 0], 3), np.round(out[:, 2], 2)))
    assert (dev_px <= total.max(1)).all()
    assert (out[:, 3] == S).all() and (out[:, 1] <= out[:, 0] + 1e-9).all()
    assert np.abs(out[:, 1] - fin[:, 1]).max() <= total.max()
    # the device's own streaming estimate of ITS log-weights is exact to float64 rounding
    own = iw_ref.finish(terms["logw"])
    assert np.abs(out[:, :3] - own[:, :3]).max() <= 1e-12 * np.abs(own[:, :3]).max()
    return out


@pytest.mark.parametrize("prior,R", [("standard_gaussian", 2), ("GMM", 2), ("vampPrior", 2), ("ours", 2), ("hierarchical", 2), ("ours", 16)])
def test_terms_and_estimate_vs_reference_mnist(golden_dir, prior, R):
    """B = 4, S = 8, rows = 12: C = 3 samples of every image per chunk, chunks of 3 + 3 + 2."""
    cfg, P, gm, rng = _setup(golden_dir, "mnist_digit", prior, R, seed=17)
    _compare(cfg, P, gm, rng, B=4, S=8, rows=12, rtol=RTOL["ours-R16" if R == 16 else prior], what="mnist_digit %s R=%d" % (prior, R))


def test_terms_and_estimate_vs_reference_celeba(golden_dir):
    """The 49 152-pixel rows on real decoder output: 4 rows, the (row, slice) route of the pixel likelihood."""
    cfg, P, gm, rng = _setup(golden_dir, "celeba", "ours", 2, seed=23)
    _compare(cfg, P, gm, rng, B=2, S=2, rows=128, rtol=RTOL["ours"], what="celeba ours")


@pytest.mark.parametrize("prior", ["standard_gaussian", "ours"])
def test_device_noise_properties(golden_dir, prior):
    from ladder_latent_data_distribution_modelling_amd.log_likelihood import ImportanceEstimator
    cfg, P, gm, rng = _setup(golden_dir, "mnist_digit", prior, 2, seed=31)
    x = rng.random((8, 28, 28, 1)).astype(np.float32)
    eng = _engine(cfg, P)
    mix = None if gm is None else (gm["weights"], gm["means"], gm["covs"])
    est = ImportanceEstimator(eng, mix, seed=7)
    a, ta = est.estimate_batch(x, 10, rows=16, first=40, return_terms=True)      # C = 2
    b, tb = est.estimate_batch(x, 10, rows=40, first=40, return_terms=True)      # C = 5
    again = est.estimate_batch(x, 10, rows=16, first=40)
    assert np.array_equal(a, again)                                             # the same seed: the same bits
    assert np.array_equal(ta["z"][3, 5], tb["z"][3, 5]) and np.array_equal(ta["z"], tb["z"])       # the draws do not depend on the chunking
    assert np.abs(a[:, 0] - b[:, 0]).max() <= 1e-9 and np.isfinite(a).all()
    assert (a[:, 1] <= a[:, 0] + 1e-9).all() and (a[:, 3] == 10).all() and ((a[:, 2] >= 1 - 1e-9) & (a[:, 2] <= 10 + 1e-9)).all()
    # ... nor on the batch: images 2 .. 7 handed in as their own batch draw the numbers of data-set images 42 .. 47 (the MNIST nets hold no batch
    # statistics; another batch size may round the encoder differently, another draw would move z by the order of sd_z = 0.4)
    _, tc = est.estimate_batch(x[2:], 10, rows=16, first=42, return_terms=True)
    assert np.abs(tc["z"] - ta["z"][2:]).max() < 1e-5
    _, td = est.estimate_batch(x[2:], 10, rows=16, first=41, return_terms=True)
    assert np.abs(td["z"] - ta["z"][2:]).max() > 1e-2
    other = ImportanceEstimator(eng, mix, seed=8).estimate_batch(x, 10, rows=16, first=40)
    assert not np.array_equal(other[:, 0], a[:, 0])
    # the data-set driver: batches of 3 + 3 + 2 images, per-image arrays, means and the standard error
    res = est.estimate(x, n_samples=6, rows=16, batch_size=3)
    assert res["n_images"] == 8 and res["n_samples"] == 6 and res["log_px"].shape == (8,) and np.isfinite(res["log_px"]).all()
    assert abs(res["mean_log_px"] - res["log_px"].mean()) < 1e-12 and abs(res["stderr_log_px"] - res["log_px"].std(ddof=1) / np.sqrt(8)) < 1e-12
    assert res["mean_elbo_1"] <= res["mean_log_px"] + 1e-9 and res["sigma"] == est.sigma


@pytest.mark.parametrize("prior", ["standard_gaussian", "ours"])
def test_trainer_method_writes_the_archive(tmp_path, golden_dir, prior):
    from ladder_latent_data_distribution_modelling_amd.codes.data_loader import DataGenerator
    from ladder_latent_data_distribution_modelling_amd.codes.models import MNISTModel_digit
    from ladder_latent_data_distribution_modelling_amd.codes.trainers import MNISTTrainer_joint_training
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import tiny_config
    cfg = tiny_config("mnist_digit")
    cfg.update(prior=prior, batch_size=64, num_epochs=1, accurate_fit=2, GM_fit_restart=1, synthetic_n_train=128, synthetic_n_val=640, result_dir=str(tmp_path) + "/",
               checkpoint_dir=str(tmp_path) + "/", data_path=str(tmp_path) + "/no-data-here/")
    data = DataGenerator(cfg, None)
    tr = MNISTTrainer_joint_training(None, MNISTModel_digit(cfg), data, cfg)
    x = data.val_set["image"][:8]
    if prior == "ours":
        with pytest.raises(RuntimeError, match="has not been fitted"):
            tr.estimate_log_likelihood(x, n_samples=6)
        gm = O.synthetic_gm(cfg, np.random.default_rng(2))
        tr.gm_final_params = tuple(gm[k].astype(np.float32) for k in ("weights", "means", "covs"))
    res = tr.estimate_log_likelihood(x, n_samples=6, rows=16, seed=3)
    saved = np.load(os.path.join(str(tmp_path), "log_likelihood_accurate-GM.npz"))
    for k in ("log_px", "elbo_1", "ess", "mean_log_px", "stderr_log_px", "mean_elbo_1", "mean_ess", "n_samples", "n_images", "sigma"):
        assert k in saved.files and np.array_equal(saved[k], res[k]) and np.isfinite(saved[k]).all(), k
    assert res["n_images"] == 8 and res["n_samples"] == 6 and res["log_px"].shape == (8,)
    again = tr.estimate_log_likelihood(x, n_samples=6, rows=16, seed=3, sigma=2 * res["sigma"])
    assert again["sigma"] == 2 * res["sigma"] and not np.array_equal(again["log_px"], res["log_px"])


def test_evaluate_cli(tmp_path, golden_dir):
    """evaluate.py as a fresh child process on 8 synthetic images, the way tests/test_gpu_generate.py drives generate.py (no checkpoint in the scratch
    directory: the freshly initialised model)."""
    cfg = json.load(open(os.path.join(ROOT, "codes", "mnist_digit_config.json")))
    cfg.update(num_hidden_units=64, num_hidden_units_inner_VAE=32, n_layers_inner_VAE=2, batch_size=64)
    cpath = str(tmp_path / "mnist_digit_config.json")
    json.dump(cfg, open(cpath, "w"))
    imgs = str(tmp_path / "images.npz")
    np.savez(imgs, images=np.random.default_rng(0).integers(0, 256, (8, 28, 28, 1), dtype=np.uint8))
    env = dict(os.environ, PYTHONPATH=ROOT)
    outp = str(tmp_path / "ll.npz")
    cmd = [sys.executable, os.path.join(ROOT, "evaluate.py"), "--config", cpath, "--n-samples", "6", "--rows", "16", "--images", imgs, "--batch-size", "8",
           "--seed", "4", "--out", outp, "--gm", os.path.join(golden_dir, "GM_prior_info.npz")]
    out = subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"')]            # (process_config prints the config as a Python dict first)
    assert len(lines) == 1, out.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_images"] == 8 and j["n_samples"] == 6 and j["prior"] == cfg["prior"] and j["sigma"] > 0
    assert all(np.isfinite(j[k]) for k in ("mean_log_px", "stderr_log_px", "mean_elbo_1", "mean_ess")) and j["mean_elbo_1"] <= j["mean_log_px"] + 1e-9
    r = np.load(outp)
    assert r["log_px"].shape == (8,) and abs(float(r["log_px"].mean()) - j["mean_log_px"]) < 1e-9
    miss = subprocess.run(cmd[:-2], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert miss.returncode != 0 and "no fitted mixture" in miss.stderr
