"""VampPrior models whose code is wider than 64 (the reference's shipped codes/celeba_config.json has code_size 256): the engine's RUN#1 / RUN#3 /
evaluate with the wide term (csrc/diag_mixture.hip) against the float64 oracle, the captured runs against the eager ones, and the trainer,
generation, `model.psedeu_prior` and the demo's prior on an 80-dimensional code.  Before there was a wide term every test here met the library's
shape error in the first run that evaluates the prior."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ladder_oracle as O

pytestmark = pytest.mark.gpu


def _engine(cfg, values=None):
    from ladder_latent_data_distribution_modelling_amd.engine import LadderEngine
    return LadderEngine(cfg, "cuda:0", values=values, seed=1)


def _ok(a, b, rtol, atol=1e-4):
    """|a-b| <= rtol*|b| + atol (tests/test_gpu_model.py: several fetches are small differences of O(10..1e3) terms)"""
    return abs(a - b) <= rtol * abs(b) + atol


@pytest.mark.parametrize("exp,Z", [("mnist_fashion", 80), ("celeba", 256)])
def test_vamp_prior_wide_code_vs_oracle(golden_dir, exp, Z):
    """tests/test_gpu_model.py::test_vamp_prior_vs_oracle on a code wider than 64, same preparation (std-head bias +0.7, pseudo-inputs rescaled):
    RUN#1 and RUN#3 fetches, every gradient (`prior/Variable` through the encoder's input included) at that test's max(bar * scale, 5 * cond), the
    exactly zero pseudo-input gradient under the standard-Gaussian switch, and evaluate."""
    d = np.load(os.path.join(golden_dir, "oracle_%s.npz" % exp))
    cfg = json.loads(str(d["config"]))
    cfg.update(prior="vampPrior", code_size=Z, n_mixtures=5, n_MC_samples=6)
    B = cfg["batch_size"]
    rng = np.random.default_rng(63)
    x = rng.random(d["x"].shape).astype(np.float32)
    P = O.init_params(cfg, seed=12)
    P["encoder/code_std_dev/bias"] = (P["encoder/code_std_dev/bias"] + 0.7).astype(np.float32)
    P["prior/Variable"] = (0.5 + 0.25 * P["prior/Variable"]).astype(np.float32)
    noise = O.make_noise(cfg, B, rng, np.float32)
    assert noise["eps_mc"].shape == (6, B, Z)
    st = O.OracleState(cfg, P, np.float64)
    st32 = O.OracleState(cfg, P, np.float32)
    eng = _engine(cfg, values=P)
    assert eng.vamp and not eng.has_inner and eng.vamp_mixture.form.query_takes_L
    for group, runner in (("ae", eng.run_ae), ("prior", eng.run_prior)):
        ref = O.run(st, x, noise, None, False, False, train=group, lr=0.0)
        ref32 = O.run(st32, x, noise, None, False, False, train=group, lr=0.0)
        runner(x, 0.0, noise, False, False)
        f = eng.fetch()
        for k in ("loss_ae", "elbo", "l1_reconstruction_error", "entropy_z", "crossEntropy_prior", "crossEntropy_prior_sg", "sigma"):
            print(group, k, f[k], float(ref[k]))
            assert _ok(f[k], float(ref[k]), 5e-5), (group, k, f[k], float(ref[k]))
        assert "prior/Variable" in ref["_grads"] or group == "ae"
        for name, g in ref["_grads"].items():
            got = eng.ps.g[name].cpu().numpy().reshape(g.shape).astype(np.float64)
            scale = np.abs(g).max()
            if scale < 1e-9:
                continue
            cond = np.abs(ref32["_grads"][name].astype(np.float64) - g).max()
            tol = max((1.5e-3 if exp == "celeba" else 5e-4) * scale, 5 * cond)
            print("%s %s: err %.3e scale %.3e cond %.3e" % (group, name, np.abs(got - g).max(), scale, cond))
            assert np.abs(got - g).max() < tol, (group, name, np.abs(got - g).max(), scale, cond)
    ref = O.run(st, x, noise, None, False, False, train="ae", lr=0.0)
    eng.evaluate(x, noise, False, False)                        # val_step
    assert _ok(eng.fetch()["elbo"], float(ref["elbo"]), 5e-5)
    # standard-Gaussian switch: crossEntropy_prior = sg, the pseudo-inputs get an exactly zero gradient
    ref = O.run(st, x, noise, None, True, False, train="ae", lr=0.0)
    eng.run_ae(x, 0.0, noise, True, False)
    assert _ok(eng.fetch()["elbo"], float(ref["elbo"]), 5e-5)
    eng.run_prior(x, 0.0, noise, True, False)
    assert float(eng.ps.g["prior/Variable"].abs().max()) == 0.0


def test_hip_graph_replay_equals_eager_vamp_wide(golden_dir):
    """The scheme of tests/test_gpu_model.py::test_hip_graph_replay_equals_eager on the tiny CelebA net with prior "vampPrior", code_size 256: the wide
    term's six launches are captured with the run after its two eager warm-ups; scalars equal in every iteration, final parameters equal."""
    d = np.load(os.path.join(golden_dir, "oracle_celeba.npz"))
    cfg = json.loads(str(d["config"]))
    cfg.update(prior="vampPrior", code_size=256, n_mixtures=5, n_MC_samples=6)
    x = d["x"]
    lr_ae, lr_s, lr_p = cfg["learning_rate_ae"], cfg["learning_rate_sigma"] * 0.99, cfg["learning_rate_prior"] * 1.01
    engs = []
    for graphs in (False, True):
        eng = _engine(cfg)
        eng.use_graphs = graphs
        engs.append(eng)
    xd = torch.as_tensor(x).cuda()
    for it in range(5):
        outs = []
        for eng in engs:
            o = []
            eng.run_ae(xd, lr_ae * (0.9 if it == 4 else 1.0), None, False, False); o.append(eng.scalars.clone())
            eng.run_sigma(xd, lr_s, None, False, False); o.append(eng.scalars.clone())
            eng.run_prior(xd, lr_p, None, False, False, reuse_encoder=True); o.append(eng.scalars.clone())
            outs.append(o)
        for a, b in zip(*outs):
            assert torch.equal(a, b), it
        assert torch.isfinite(outs[0][0]).all()
    assert len(engs[1]._graphs) >= 3 and not engs[0]._graphs
    pa, pb = engs[0].ps.to_dict(), engs[1].ps.to_dict()
    for k in pa:
        assert np.array_equal(pa[k], pb[k]), k
    assert engs[0].ps.step == engs[1].ps.step


def test_trainer_and_generation_vamp_wide(tmp_path):
    """tests/test_gpu_model.py::test_trainer_vamp_prior_epochs at code_size 80, then everything else that reads the pseudo-input mixture at that
    width: generation from it, `model.psedeu_prior.sample` through Session, and the demo's MixturePrior."""
    from ladder_latent_data_distribution_modelling_amd.codes.data_loader import DataGenerator
    from ladder_latent_data_distribution_modelling_amd.codes.models import MNISTModel_digit
    from ladder_latent_data_distribution_modelling_amd.codes.trainers import MNISTTrainer_joint_training
    from ladder_latent_data_distribution_modelling_amd.codes.session import Session
    from ladder_latent_data_distribution_modelling_amd.codes import tf_bundle
    from ladder_latent_data_distribution_modelling_amd.demo.demo_tools import MixturePrior, define_prior_distribution
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import tiny_config
    cfg = tiny_config("mnist_digit")
    cfg.update(prior="vampPrior", code_size=80, n_mixtures=6, batch_size=64, num_epochs=2, sg_pretraining=1, synthetic_n_train=256,
               synthetic_n_val=640, result_dir=str(tmp_path) + "/", checkpoint_dir=str(tmp_path) + "/", n_MC_samples=5)
    data = DataGenerator(cfg, None)
    model = MNISTModel_digit(cfg)
    p0 = model.engine.ps.to_dict()["prior/Variable"].copy()
    tr = MNISTTrainer_joint_training(None, model, data, cfg)
    tr.train()
    sess = Session()
    n_it = tr.n_train_iter
    assert len(tr.vampPrior_crossEntropy_prior_train) == 2 * n_it and len(tr.train_loss_prior) == 2 * n_it
    assert np.isfinite(tr.elbo_train).all() and np.isfinite(tr.vampPrior_crossEntropy_prior_val).all()
    assert np.isfinite(tr.vampPrior_crossEntropy_prior_train).all() and np.isfinite(tr.train_loss_prior).all()
    p1 = model.engine.ps.to_dict()["prior/Variable"]
    assert p1.shape == (6, 28, 28, 1) and not np.array_equal(p0, p1)                  # the pseudo-inputs moved (epoch 2)
    ck = tf_bundle.load_checkpoint(os.path.join(str(tmp_path), "prior-model"))
    assert list(ck) == ["prior/Variable"] and np.array_equal(ck["prior/Variable"], p1)
    code, _ = tr.generate_samples_from_prior_by_method(method="vampPrior", n_sample=3)
    assert code.shape == (9, 80) and code.dtype == np.float32 and np.isfinite(code).all()
    s = sess.run(model.psedeu_prior.sample(4))
    assert s.shape == (4, 80) and np.isfinite(s).all()
    pr = define_prior_distribution(cfg, sess, model)
    assert isinstance(pr, MixturePrior) and (pr.K, pr.R) == (6, 80)
    lp = sess.run(pr.log_prob(pr.m.astype(np.float32)))
    assert lp.shape == (6,) and np.isfinite(lp).all()
