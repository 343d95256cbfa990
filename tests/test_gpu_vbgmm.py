"""Device VB-GMM fit (csrc/vbgmm.hip) against sklearn.mixture.BayesianGaussianMixture itself -- the reference's own producer
of the hyper-prior feed (codes/base.py:93-99) -- through sklearn's public API: same data, same `random_state` (hence the same
k-means labels), cold fit, warm-started refit on new samples, both weight-prior types, R = 2 and R = 8."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _samples(rng, n, R, centres=6):
    c = rng.normal(0, 2.0, size=(centres, R))
    A = rng.normal(0, 0.35, size=(centres, R, R))
    idx = rng.integers(0, centres, n)
    return (c[idx] + np.einsum("nij,nj->ni", A[idx], rng.normal(size=(n, R)))).astype(np.float32)


@pytest.mark.parametrize("R,K,ptype,max_iter", [(2, 10, "dirichlet_distribution", 1000), (2, 30, "dirichlet_distribution", 1000),
                                                (8, 50, "dirichlet_distribution", 300), (2, 30, "dirichlet_process", 2000),
                                                (3, 7, "dirichlet_process", 5)])
def test_vbgmm_matches_sklearn(R, K, ptype, max_iter):
    import warnings
    from sklearn.mixture import BayesianGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.codes.vbgmm import DeviceBayesianGaussianMixture
    rng = np.random.default_rng(R * 100 + K)
    X1, X2 = _samples(rng, 2048, R), _samples(rng, 2048, R)
    kw = dict(n_components=K, covariance_type="full", max_iter=max_iter, n_init=1, weight_concentration_prior_type=ptype,
              weight_concentration_prior=0.1, warm_start=True, random_state=7)
    ref, dev = BayesianGaussianMixture(**kw), DeviceBayesianGaussianMixture(**kw)
    for X in (X1, X2):                                     # cold fit, then warm start on fresh samples (one per epoch in training)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref.fit(X.astype(np.float64))                  # the reference feeds float64 copies of its float32 samples
            dev.fit(torch.as_tensor(X).cuda())
        assert dev.n_iter_ == ref.n_iter_ and dev.converged_ == ref.converged_
        assert abs(dev.lower_bound_ - ref.lower_bound_) <= 1e-9 * abs(ref.lower_bound_)
        np.testing.assert_allclose(dev.weights_, ref.weights_, rtol=1e-8, atol=1e-12)
        np.testing.assert_allclose(dev.means_, ref.means_, rtol=1e-8, atol=1e-10)
        np.testing.assert_allclose(dev.covariances_, ref.covariances_, rtol=1e-7, atol=1e-10)
        # the float32 feed copies are the rounded float64 parameters
        np.testing.assert_array_equal(dev.weights_dev.cpu().numpy(), dev.weights_.astype(np.float32))
        np.testing.assert_array_equal(dev.covariances_dev.cpu().numpy(), dev.covariances_.astype(np.float32))


def test_vbgmm_restarts_determinism_and_errors():
    from ladder_latent_data_distribution_modelling_amd.codes.vbgmm import DeviceBayesianGaussianMixture
    from sklearn.mixture import BayesianGaussianMixture
    rng = np.random.default_rng(5)
    X = _samples(rng, 3000, 2)
    kw = dict(n_components=12, covariance_type="full", max_iter=2000, n_init=3, weight_concentration_prior_type="dirichlet_process",
              weight_concentration_prior=0.1, warm_start=False, random_state=3)
    a = DeviceBayesianGaussianMixture(**kw).fit(torch.as_tensor(X).cuda())
    b = DeviceBayesianGaussianMixture(**kw).fit(X)                              # host array input, second object: bit-identical
    assert a.lower_bound_ == b.lower_bound_ and np.array_equal(a.covariances_, b.covariances_)
    ref = BayesianGaussianMixture(**kw).fit(X.astype(np.float64))                # best of the same three k-means initialisations
    assert a.n_iter_ == ref.n_iter_ and abs(a.lower_bound_ - ref.lower_bound_) <= 1e-9 * abs(ref.lower_bound_)
    np.testing.assert_allclose(a.weights_, ref.weights_, rtol=1e-8, atol=1e-12)
    with pytest.raises(ValueError, match="n_samples >= n_components"):
        DeviceBayesianGaussianMixture(n_components=12).fit(X[:5])
    with pytest.raises(NotImplementedError):
        DeviceBayesianGaussianMixture(n_components=3, covariance_type="diag")


@pytest.mark.parametrize("R,K,ptype,max_iter", [(2, 30, "dirichlet_distribution", 1000), (8, 50, "dirichlet_distribution", 300),
                                                (2, 30, "dirichlet_process", 2000), (3, 7, "dirichlet_process", 5)])
def test_vbgmm_sharded_statistics_fit_matches_sklearn_one_rank(R, K, ptype, max_iter):
    """The sharded fit (E-step + local sufficient statistics / all-reduce / M-step per iteration: csrc/vbgmm.hip, exchange step C5) on ONE
    rank, where the all-reduce is the identity: cold fit and warm-started refit against sklearn -- same iteration count, lower bound
    to 1e-8, parameters to 1e-7 (second moments are accumulated raw and centred in the M-step; sklearn centres first) -- and the
    result must not depend on how often the host looks at the `done` flag (iterations enqueued past the end are no-ops)."""
    import warnings
    from sklearn.mixture import BayesianGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.codes.vbgmm import DeviceBayesianGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.engine import Comm
    rng = np.random.default_rng(R * 100 + K)
    X1, X2 = _samples(rng, 2048, R), _samples(rng, 2048, R)
    kw = dict(n_components=K, covariance_type="full", max_iter=max_iter, n_init=1, weight_concentration_prior_type=ptype,
              weight_concentration_prior=0.1, warm_start=True, random_state=7)
    ref, dev, dev1 = BayesianGaussianMixture(**kw), DeviceBayesianGaussianMixture(**kw), DeviceBayesianGaussianMixture(**kw)
    comm = Comm()
    assert not comm.on
    for X in (X1, X2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref.fit(X.astype(np.float64))
            dev.fit_sharded(torch.as_tensor(X).cuda(), comm)
            dev1.fit_sharded(torch.as_tensor(X).cuda(), comm, check_every=1)
        assert dev.n_iter_ == ref.n_iter_ and dev.converged_ == ref.converged_
        assert abs(dev.lower_bound_ - ref.lower_bound_) <= 1e-8 * abs(ref.lower_bound_)
        np.testing.assert_allclose(dev.weights_, ref.weights_, rtol=1e-7, atol=1e-11)
        np.testing.assert_allclose(dev.means_, ref.means_, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(dev.covariances_, ref.covariances_, rtol=1e-6, atol=1e-9)
        assert dev1.n_iter_ == dev.n_iter_ and dev1.lower_bound_ == dev.lower_bound_ and np.array_equal(dev1.covariances_, dev.covariances_)
        np.testing.assert_array_equal(dev.weights_dev.cpu().numpy(), dev.weights_.astype(np.float32))


SHARD_WORKER = r'''
import os, sys, warnings
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
rank, world = int(sys.argv[1]), int(sys.argv[2])
if world > 1:
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=world)
from ladder_latent_data_distribution_modelling_amd.codes.vbgmm import DeviceBayesianGaussianMixture
from ladder_latent_data_distribution_modelling_amd.engine import Comm
d = np.load(sys.argv[3])
comm = Comm()
assert comm.world == world
kw = dict(n_components=int(d["K"]), covariance_type="full", max_iter=1000, n_init=1, weight_concentration_prior_type="dirichlet_distribution",
          weight_concentration_prior=0.1, warm_start=True, random_state=7)
gm = DeviceBayesianGaussianMixture(device="cuda:0", **kw)
out = {}
for i, key in enumerate(("X1", "X2")):
    X = d[key]
    n = X.shape[0] // world
    Xl = X[rank * n:(rank + 1) * n] if rank < world - 1 else X[rank * n:]          # contiguous shards in rank order (ragged tail on the last)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        gm.fit_sharded(torch.as_tensor(Xl).cuda(), comm)
    out["n_iter%%d" %% i], out["lb%%d" %% i] = gm.n_iter_, gm.lower_bound_
    out["w%%d" %% i], out["m%%d" %% i], out["c%%d" %% i] = gm.weights_, gm.means_, gm.covariances_
if rank == 0:
    np.savez(sys.argv[4], **out)
if world > 1:
    dist.barrier()
    dist.destroy_process_group()
'''


def test_vbgmm_sharded_fit_two_ranks_equals_sklearn(tmp_path):
    """C5 with a real exchange: two processes (sharing cuda:0 over gloo; RCCL refuses two ranks on one device) hold 1024 + 1027 samples each
    and all-reduce the sufficient statistics every variational iteration; cold fit + warm-started refit must reproduce sklearn's fit of
    the 2051 samples (same iteration count, lower bound 1e-8, parameters 1e-7)."""
    import os
    import subprocess
    import sys
    import warnings
    from sklearn.mixture import BayesianGaussianMixture
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rng = np.random.default_rng(77)
    R, K = 2, 20
    X1, X2 = _samples(rng, 2051, R), _samples(rng, 2051, R)
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, X1=X1, X2=X2, K=K)
    script = tmp_path / "shard_worker.py"
    script.write_text(SHARD_WORKER % dict(root=root, port=32500 + os.getpid() % 2000))
    procs = [subprocess.Popen([sys.executable, str(script), str(r), "2", inp, outp], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(2)]
    outs = [p.communicate(timeout=900)[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[-2500:] for o in outs]
    got = np.load(outp)
    ref = BayesianGaussianMixture(n_components=K, covariance_type="full", max_iter=1000, n_init=1,
                                  weight_concentration_prior_type="dirichlet_distribution", weight_concentration_prior=0.1, warm_start=True,
                                  random_state=7)
    for i, X in enumerate((X1, X2)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref.fit(X.astype(np.float64))
        assert int(got["n_iter%d" % i]) == ref.n_iter_, (i, int(got["n_iter%d" % i]), ref.n_iter_)
        assert abs(float(got["lb%d" % i]) - ref.lower_bound_) <= 1e-8 * abs(ref.lower_bound_)
        np.testing.assert_allclose(got["w%d" % i], ref.weights_, rtol=1e-7, atol=1e-11)
        np.testing.assert_allclose(got["m%d" % i], ref.means_, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(got["c%d" % i], ref.covariances_, rtol=1e-6, atol=1e-9)


DP_TRAINER_WORKER = r'''
import json, os, sys
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests", "golden"))
rank, mode, outp = int(sys.argv[1]), sys.argv[2], sys.argv[3]
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=2)
from make_golden import tiny_config
from ladder_latent_data_distribution_modelling_amd.codes.data_loader import DataGenerator
from ladder_latent_data_distribution_modelling_amd.codes.models import MNISTModel_digit
from ladder_latent_data_distribution_modelling_amd.codes.trainers import MNISTTrainer_joint_training
cfg = tiny_config("mnist_digit")
cfg.update(batch_size=64, num_epochs=1, sg_pretraining=1, accurate_fit=2, GM_fit_restart=1, synthetic_n_train=512, synthetic_n_val=256,
           result_dir=sys.argv[4] + "/", checkpoint_dir=sys.argv[4] + "/", n_MC_samples=10, gm_fit_backend="hip", gm_fit_mode=mode, gm_random_state=7)
data = DataGenerator(cfg, None)
model = MNISTModel_digit(cfg, device="cuda:0")
tr = MNISTTrainer_joint_training(None, model, data, cfg)
assert tr.engine.ctx.comm.world == 2
tr.train()
w, m, c = (np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, np.float64) for a in tr.gm_params)
gm = tr.model.GM_prior_training
allw = [torch.zeros(w.size, dtype=torch.float64) for _ in range(2)]
dist.all_gather(allw, torch.as_tensor(w))
assert torch.equal(allw[0], allw[1]), "the ranks hold different mixtures"
if rank == 0:
    gf = tr.GM_prior_final
    np.savez(outp, w=w, m=m, c=c, n_iter=gm.n_iter_, lb=gm.lower_bound_, elbo=np.asarray(tr.elbo_train), n_iter_final=gf.n_iter_, lb_final=gf.lower_bound_,
             w_final=np.asarray(gf.weights_))
dist.barrier()
dist.destroy_process_group()
'''


def test_trainer_fit_gm_two_ranks_statistics_allreduce_vs_replicated(tmp_path):
    """The reference's per-epoch fit_GM hand-off (codes/base.py:681-789, 988-999) under data parallelism, through the trainer: 2 ranks on
    cuda:0 over gloo, one epoch ending in the "fast" and the "accurate" fit.  `gm_fit_mode: "allreduce_stats"` (the default: every rank
    keeps its own t-samples and the sufficient statistics are all-reduced per variational iteration) must give the same mixture as
    `"replicated"` (all-gather + the same persistent-kernel fit on every rank) and identical mixtures on both ranks."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for i, mode in enumerate(("allreduce_stats", "replicated")):
        script = tmp_path / ("dp_trainer_%s.py" % mode)
        script.write_text(DP_TRAINER_WORKER % dict(root=root, port=33500 + os.getpid() % 2000 + i))
        outp = str(tmp_path / (mode + ".npz"))
        wd = tmp_path / mode
        wd.mkdir()
        procs = [subprocess.Popen([sys.executable, str(script), str(r), mode, outp, str(wd)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                                  text=True, cwd=str(wd)) for r in range(2)]
        outs = [p.communicate(timeout=900)[0] for p in procs]
        assert all(p.returncode == 0 for p in procs), [o[-2500:] for o in outs]
        res[mode] = np.load(outp)
    a, b = res["allreduce_stats"], res["replicated"]
    # one epoch: the training steps before the fits are identical in both modes, so both fit the SAME t-samples (the fits of a second
    # epoch would see samples that differ at fp32 level -- the mixture feeds differ in the last float64 bits -- and a 290-iteration
    # variational loop stops a few iterations earlier or later on such inputs; warm starts are covered at kernel level above)
    assert np.array_equal(a["elbo"], b["elbo"])
    for suffix in ("", "_final"):                                   # the per-epoch "fast" fit and the "accurate" Dirichlet-process fit
        assert int(a["n_iter" + suffix]) == int(b["n_iter" + suffix]), (suffix, int(a["n_iter" + suffix]), int(b["n_iter" + suffix]))
        assert abs(float(a["lb" + suffix]) - float(b["lb" + suffix])) <= 1e-8 * abs(float(b["lb" + suffix]))
    np.testing.assert_allclose(a["w"], b["w"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(a["m"], b["m"], rtol=1e-6, atol=1e-8)
    np.testing.assert_allclose(a["c"], b["c"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(a["w_final"], b["w_final"], rtol=1e-6, atol=1e-9)


def test_sliced_fit_at_accurate_fit_size_vs_sklearn_and_persistent(monkeypatch):
    """From 1 024 samples on fit() runs one multi-workgroup E-step (256-sample slices, fixed-order reduction of their statistics) + one
    M-step launch per variational iteration -- the reference's accurate fit (codes/base.py:723-789) takes 20 096 samples, which the
    one-workgroup persistent kernel walks in 3.8 ms per iteration.  Same iteration count and lower bound as sklearn and as the
    persistent kernel, parameters to float64 round-off; N is not a multiple of the slice (ragged last workgroup)."""
    import warnings
    from sklearn.mixture import BayesianGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.codes import vbgmm
    rng = np.random.default_rng(5)
    N, R, K = 5003, 2, 12
    X = _samples(rng, N, R, centres=5)
    kw = dict(n_components=K, covariance_type="full", max_iter=2000, n_init=1, weight_concentration_prior_type="dirichlet_process",
              weight_concentration_prior=0.1, warm_start=False, random_state=0)

    def fit(obj, data):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return obj.fit(data)

    sk = fit(BayesianGaussianMixture(**kw), X.astype(np.float64))
    assert N >= vbgmm.SLICED_FIT_MIN_SAMPLES
    dv = fit(vbgmm.DeviceBayesianGaussianMixture(**kw), torch.as_tensor(X).cuda())
    assert (dv.n_iter_, dv.converged_) == (sk.n_iter_, sk.converged_), (dv.n_iter_, sk.n_iter_)
    assert abs(dv.lower_bound_ - sk.lower_bound_) <= 1e-8 * abs(sk.lower_bound_)
    np.testing.assert_allclose(dv.weights_, sk.weights_, rtol=1e-7, atol=1e-10)
    np.testing.assert_allclose(dv.means_, sk.means_, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(dv.covariances_, sk.covariances_, rtol=1e-6, atol=1e-9)
    monkeypatch.setattr(vbgmm, "SLICED_FIT_MIN_SAMPLES", 1 << 30)                       # the persistent one-workgroup kernel
    pv = fit(vbgmm.DeviceBayesianGaussianMixture(**kw), torch.as_tensor(X).cuda())
    assert (pv.n_iter_, pv.converged_) == (dv.n_iter_, dv.converged_)
    assert abs(pv.lower_bound_ - dv.lower_bound_) <= 1e-9 * abs(dv.lower_bound_)
    np.testing.assert_allclose(pv.means_, dv.means_, rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(pv.covariances_, dv.covariances_, rtol=1e-7, atol=1e-10)


@pytest.mark.parametrize("R,K,ptype,max_iter", [(2, 30, "dirichlet_distribution", 1000), (8, 50, "dirichlet_distribution", 300)])
def test_persistent_kernel_still_matches_sklearn(R, K, ptype, max_iter, monkeypatch):
    """The single-launch persistent fit (now the path of fits below 1 024 samples) at the sizes it was written for."""
    from ladder_latent_data_distribution_modelling_amd.codes import vbgmm
    monkeypatch.setattr(vbgmm, "SLICED_FIT_MIN_SAMPLES", 1 << 30)
    test_vbgmm_matches_sklearn(R, K, ptype, max_iter)


# the two paths of fit(): threshold 0 -> the sliced E-step / M-step launches, 1 << 30 -> the persistent one-workgroup kernel
PATHS = [pytest.param(0, id="sliced"), pytest.param(1 << 30, id="persistent")]


@pytest.mark.parametrize("threshold", PATHS)
@pytest.mark.parametrize("ptype", ["dirichlet_distribution", "dirichlet_process"])
@pytest.mark.parametrize("N,R,K", [(70, 1, 1), (70, 1, 2), (257, 1, 3), (257, 2, 1)])
def test_vbgmm_smallest_shapes_match_sklearn(N, R, K, ptype, threshold, monkeypatch):
    """The shapes at which the device functions both paths share (csrc/vbgmm.hip: vb_*) would go wrong with a wrong stride or loop bound:
    K = 1 (empty stick-breaking prefix and suffix), R = 1 (1 x 1 factors), N = 70 (no multiple of the wavefront), N = 257 (one 256-sample
    slice plus a one-sample slice).  Cold fit, then a warm-started refit, five iterations each by construction (tol = 0), against sklearn at
    the tolerances test_vbgmm_matches_sklearn (persistent) and test_vbgmm_sharded_statistics_fit_matches_sklearn_one_rank (sliced) hold."""
    import warnings
    from sklearn.mixture import BayesianGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.codes import vbgmm
    monkeypatch.setattr(vbgmm, "SLICED_FIT_MIN_SAMPLES", threshold)
    sliced = threshold == 0
    rng = np.random.default_rng(N * 100 + R * 10 + K)
    X1, X2 = _samples(rng, N, R, centres=3), _samples(rng, N, R, centres=3)
    kw = dict(n_components=K, covariance_type="full", max_iter=5, tol=0.0, n_init=1, weight_concentration_prior_type=ptype,
              weight_concentration_prior=0.1, warm_start=True, random_state=7)
    ref, dev = BayesianGaussianMixture(**kw), vbgmm.DeviceBayesianGaussianMixture(**kw)
    for X in (X1, X2):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref.fit(X.astype(np.float64))
            dev.fit(torch.as_tensor(X).cuda())
        assert dev.n_iter_ == ref.n_iter_ == 5 and dev.converged_ == ref.converged_
        assert abs(dev.lower_bound_ - ref.lower_bound_) <= (1e-8 if sliced else 1e-9) * abs(ref.lower_bound_)
        np.testing.assert_allclose(dev.weights_, ref.weights_, rtol=1e-7 if sliced else 1e-8, atol=1e-11 if sliced else 1e-12)
        np.testing.assert_allclose(dev.means_, ref.means_, rtol=1e-7 if sliced else 1e-8, atol=1e-9 if sliced else 1e-10)
        np.testing.assert_allclose(dev.covariances_, ref.covariances_, rtol=1e-6 if sliced else 1e-7, atol=1e-9 if sliced else 1e-10)
        np.testing.assert_array_equal(dev.weights_dev.cpu().numpy(), dev.weights_.astype(np.float32))
        if not sliced:
            np.testing.assert_array_equal(dev.covariances_dev.cpu().numpy(), dev.covariances_.astype(np.float32))


@pytest.mark.parametrize("threshold", PATHS)
@pytest.mark.parametrize("ptype", ["dirichlet_distribution", "dirichlet_process"])
def test_vbgmm_ill_defined_covariance_raises(ptype, threshold, monkeypatch):
    """64 identical samples without reg_covar: the empirical covariance has no positive pivot, the M-step of either path leaves status -1 in
    the state tail and fit() raises what sklearn raises.  An error return, not a device fault."""
    from ladder_latent_data_distribution_modelling_amd.codes import vbgmm
    monkeypatch.setattr(vbgmm, "SLICED_FIT_MIN_SAMPLES", threshold)
    X = np.full((64, 2), 0.5, dtype=np.float32)
    gm = vbgmm.DeviceBayesianGaussianMixture(n_components=2, covariance_type="full", reg_covar=0.0, weight_concentration_prior_type=ptype,
                                             random_state=7)
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        gm.fit(torch.as_tensor(X).cuda())
