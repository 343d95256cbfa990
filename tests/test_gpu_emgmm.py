"""Device EM fit of the "GMM" prior (csrc/emgmm.hip, codes/emgmm.py) against sklearn.mixture.GaussianMixture itself -- the reference's own
producer of the mixture on z (codes/base.py:101-106, 699-710, 749-767) -- through sklearn's public API: same data, same `random_state` (hence the
same k-means labels), cold fit, warm-started refit on new samples of the same mixture; one GPU, sharded over two ranks, and through the trainer."""
import functools
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emgmm_ref as E  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATTRS = ("weights_", "means_", "covariances_", "precisions_cholesky_")


@functools.lru_cache(maxsize=None)
def _reference(i):
    """sklearn's cold fit (+ warm refit) of case i, computed once: per fit a dict of n_iter_, converged_, lower_bound_, the parameters and the number
    of ConvergenceWarnings.  Each fit first passes the precondition that round-off cannot decide its iteration count."""
    from sklearn.mixture import GaussianMixture
    N, R, K, max_iter, centres, spread, seed, n_iters = E.CASES[i]
    ref = GaussianMixture(n_components=K, max_iter=max_iter, **E.KW)
    out = []
    for X, n_iter in zip(E.data(N, R, centres, spread, seed), n_iters):
        if n_iter is None:
            break
        warned = E.sklearn_fit(ref, X)
        E.assert_iteration_count_is_decidable(ref, E.KW["tol"], max_iter)
        assert ref.n_iter_ == n_iter
        snap = dict(n_iter_=ref.n_iter_, converged_=ref.converged_, lower_bound_=ref.lower_bound_, warned=len(warned))
        snap.update({a: getattr(ref, a).copy() for a in ATTRS})
        out.append(snap)
    return out


class _Snap:
    def __init__(self, d):
        self.__dict__.update(d)


def _device_fit(dev, X, comm=None, **kw):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        if comm is None:
            dev.fit(X)
        else:
            dev.fit_sharded(X, comm, **kw)
    return len([x for x in w if x.category.__name__ == "ConvergenceWarning"])


def _check(dev, warned, snap):
    assert (dev.n_iter_, dev.converged_, warned) == (snap["n_iter_"], snap["converged_"], snap["warned"])
    E.assert_close(dev, _Snap(snap))
    # the float32 feed copies are the rounded float64 parameters
    np.testing.assert_array_equal(dev.weights_dev.cpu().numpy(), dev.weights_.astype(np.float32))
    np.testing.assert_array_equal(dev.means_dev.cpu().numpy(), dev.means_.astype(np.float32))
    np.testing.assert_array_equal(dev.covariances_dev.cpu().numpy(), dev.covariances_.astype(np.float32))


@pytest.mark.parametrize("i", range(len(E.CASES)), ids=["%dx%dx%d" % c[:3] for c in E.CASES])
def test_emgmm_matches_sklearn(i):
    """Cold fit on X1, warm refit on X2: n_iter_, converged_ and the ConvergenceWarning equal sklearn's; lower bound to 1e-8, weights / means to 1e-7,
    covariances / precisions_cholesky_ to 1e-6 (the bars of the sharded VB fit, tests/emgmm_ref.py)."""
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    N, R, K, max_iter, centres, spread, seed, _ = E.CASES[i]
    dev = DeviceGaussianMixture(n_components=K, max_iter=max_iter, **E.KW)
    for X, snap in zip(E.data(N, R, centres, spread, seed), _reference(i)):
        warned = _device_fit(dev, torch.as_tensor(X).cuda())
        _check(dev, warned, snap)


def test_emgmm_one_rank_sharded_fit_does_not_depend_on_check_every():
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.engine import Comm
    i = 3
    N, R, K, max_iter, centres, spread, seed, _ = E.CASES[i]
    comm = Comm()
    assert not comm.on
    a, b = (DeviceGaussianMixture(n_components=K, max_iter=max_iter, **E.KW) for _ in range(2))
    for X, snap in zip(E.data(N, R, centres, spread, seed), _reference(i)):
        Xd = torch.as_tensor(X).cuda()
        wa = _device_fit(a, Xd, comm=comm, check_every=1)
        _device_fit(b, Xd, comm=comm, check_every=16)
        _check(a, wa, snap)
        assert a.n_iter_ == b.n_iter_ and a.lower_bound_ == b.lower_bound_ and a.converged_ == b.converged_
        for name in ATTRS:
            assert np.array_equal(getattr(a, name), getattr(b, name)), name


SHARD_WORKER = r'''
import os, sys, warnings
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, %(root)r)
rank, world = int(sys.argv[1]), int(sys.argv[2])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%(port)d", rank=rank, world_size=world)
from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
from ladder_latent_data_distribution_modelling_amd.engine import Comm
d = np.load(sys.argv[3])
comm = Comm()
assert comm.world == world and comm.on
gm = DeviceGaussianMixture(n_components=int(d["K"]), covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=int(d["max_iter"]), n_init=1,
                           warm_start=True, random_state=7, device="cuda:0")
out = {}
for i, key in enumerate(("X1", "X2")):
    X = d[key]
    Xl = X[:1024] if rank == 0 else X[1024:]                                        # 1024 + 1027 samples, rank order
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        gm.fit_sharded(torch.as_tensor(Xl).cuda(), comm)
    out["warned%%d" %% i] = len([x for x in w if x.category.__name__ == "ConvergenceWarning"])
    out["n_iter%%d" %% i], out["lb%%d" %% i], out["conv%%d" %% i] = gm.n_iter_, gm.lower_bound_, gm.converged_
    out["w%%d" %% i], out["m%%d" %% i], out["c%%d" %% i], out["p%%d" %% i] = gm.weights_, gm.means_, gm.covariances_, gm.precisions_cholesky_
np.savez(sys.argv[4] + ".%%d.npz" %% rank, **out)
dist.barrier()
dist.destroy_process_group()
'''


def test_emgmm_sharded_fit_two_ranks_equals_sklearn(tmp_path):
    """Two processes (sharing cuda:0 over gloo) hold 1024 + 1027 samples and all-reduce the statistics -- the sum of log_prob_norm among them -- every
    EM iteration; cold fit + warm refit reproduce sklearn's fit of the 2051 samples at the bars of the one-GPU fit, and both ranks end with
    bit-identical float64 parameters."""
    i = 3
    N, R, K, max_iter, centres, spread, seed, _ = E.CASES[i]
    assert (N, R, K) == (2051, 16, 5)
    X1, X2 = E.data(N, R, centres, spread, seed)
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out")
    np.savez(inp, X1=X1, X2=X2, K=K, max_iter=max_iter)
    script = tmp_path / "emgmm_shard_worker.py"
    script.write_text(SHARD_WORKER % dict(root=ROOT, port=34500 + os.getpid() % 2000))
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, str(script), str(r), "2", inp, outp], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate()[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[-2500:] for o in outs]
    got = [np.load(outp + ".%d.npz" % r) for r in range(2)]
    for f, snap in enumerate(_reference(i)):
        g = got[0]
        assert (int(g["n_iter%d" % f]), bool(g["conv%d" % f]), int(g["warned%d" % f])) == (snap["n_iter_"], snap["converged_"], snap["warned"])
        E.assert_close(_Snap(dict(lower_bound_=float(g["lb%d" % f]), weights_=g["w%d" % f], means_=g["m%d" % f], covariances_=g["c%d" % f],
                                  precisions_cholesky_=g["p%d" % f])), _Snap(snap))
        for key in ("n_iter", "lb", "w", "m", "c", "p"):
            assert np.array_equal(got[0]["%s%d" % (key, f)], got[1]["%s%d" % (key, f)]), (key, f)


def test_emgmm_determinism_restarts_and_errors():
    from sklearn.mixture import GaussianMixture
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    N, R, K, max_iter, centres, spread, seed, _ = E.CASES[0]
    X = E.data(N, R, centres, spread, seed)[0]
    kw = dict(n_components=K, covariance_type="full", tol=1e-3, reg_covar=1e-6, max_iter=max_iter, n_init=3, warm_start=False, random_state=3)
    a = DeviceGaussianMixture(**kw).fit(torch.as_tensor(X).cuda())
    b = DeviceGaussianMixture(**kw).fit(X)                                        # host array input, second object: bit-identical
    assert a.lower_bound_ == b.lower_bound_ and a.n_iter_ == b.n_iter_
    for name in ATTRS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    ref = GaussianMixture(**kw).fit(X.astype(np.float64))                          # best of the same three k-means initialisations
    assert a.n_iter_ == ref.n_iter_ and a.converged_ == ref.converged_
    E.assert_close(a, ref)
    with pytest.raises(ValueError, match="n_samples >= n_components"):
        DeviceGaussianMixture(n_components=12).fit(X[:5])
    with pytest.raises(NotImplementedError):
        DeviceGaussianMixture(n_components=3, covariance_type="diag")

    # the C ABI refuses before any launch: the buffers below are far too small for a kernel that ran
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
    x, buf, f32 = torch.zeros(64, 64, device="cuda"), f64(64), torch.zeros(64, device="cuda")
    ws = torch.empty(1 << 16, dtype=torch.uint8, device="cuda")
    for Kb, Rb in ((3, 65), (65, 3)):
        assert lib.ladder_emgmm_state_doubles(Kb, Rb) > 0
        assert lib.ladder_emgmm_estep(x.data_ptr(), 8, Kb, Rb, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), ws.data_ptr(), ws.numel(), st) == -1
        assert lib.ladder_emgmm_mstep(buf.data_ptr(), buf.data_ptr(), Kb, Rb, buf.data_ptr(), 1e-6, 1e-3, 10, 1, f32.data_ptr(), f32.data_ptr(),
                                      f32.data_ptr(), st) == -1
        assert lib.ladder_emgmm_prepare(buf.data_ptr(), Kb, Rb, st) == -1
    assert lib.ladder_emgmm_shift(x.data_ptr(), 8, 65, buf.data_ptr(), st) == -1
    assert lib.ladder_emgmm_shift(x.data_ptr(), 0, 3, buf.data_ptr(), st) == -1
    state, stats = f64(lib.ladder_emgmm_state_doubles(2, 3)), f64(lib.ladder_emgmm_stats_doubles(2, 3))
    need = lib.ladder_emgmm_workspace_bytes(64, 2, 3)
    assert 0 < need <= ws.numel()
    args = (x.data_ptr(), 64, 2, 3, None, state.data_ptr(), buf.data_ptr(), stats.data_ptr(), ws.data_ptr())
    assert lib.ladder_emgmm_estep(*args, need - 1, st) == -3
    assert lib.ladder_emgmm_estep(x.data_ptr(), 0, 2, 3, None, state.data_ptr(), buf.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws.numel(), st) == -1
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0 and float(state.abs().sum()) == 0.0 and float(stats.abs().sum()) == 0.0

    # a covariance with a non-positive pivot is a STATUS: -1 in the state, sklearn's ValueError in Python
    gm = DeviceGaussianMixture(n_components=2)
    host = np.zeros(state.numel())
    host[0:2] = 0.5
    host[2 + 6:2 + 6 + 18] = np.stack([np.eye(3), np.diag([1.0, -1.0, 1.0])]).ravel()
    state.copy_(torch.as_tensor(host))
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        gm._prepare_state(state, 3)
    tail = state[-4:].cpu().numpy()
    assert tail[2] == -1.0 and tail[3] == 1.0
    pchol = state[2 + 6 + 18:2 + 6 + 36].cpu().numpy().reshape(2, 3, 3)
    np.testing.assert_array_equal(pchol[0], np.eye(3))
    host[2 + 6 + 9:2 + 6 + 18] = np.array([[4.0, 2.0, 0.0], [2.0, 5.0, 0.0], [0.0, 0.0, 1.0]]).ravel()
    state.copy_(torch.as_tensor(host))
    gm._prepare_state(state, 3)                                                   # well-defined now: no error, precisions_cholesky_ = L^-T
    pchol = state[2 + 6 + 18:2 + 6 + 36].cpu().numpy().reshape(2, 3, 3)
    np.testing.assert_allclose(pchol[1], np.linalg.inv(np.linalg.cholesky(host[2 + 6 + 9:2 + 6 + 18].reshape(3, 3))).T, rtol=1e-14, atol=1e-15)


def _train_gmm_prior(tmp_path, **extra):
    from ladder_latent_data_distribution_modelling_amd.codes.data_loader import DataGenerator
    from ladder_latent_data_distribution_modelling_amd.codes.models import MNISTModel_fashion
    from ladder_latent_data_distribution_modelling_amd.codes.trainers import MNISTTrainer_joint_training
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import tiny_config
    cfg = tiny_config("mnist_fashion")
    cfg.update(prior="GMM", code_size=16, n_mixtures=3, batch_size=64, num_epochs=2, sg_pretraining=1, synthetic_n_train=256,
               synthetic_n_val=640, result_dir=str(tmp_path) + "/", checkpoint_dir=str(tmp_path) + "/", n_MC_samples=5, **extra)
    model = MNISTModel_fashion(cfg)
    return model, MNISTTrainer_joint_training(None, model, DataGenerator(cfg, None), cfg)


def test_trainer_gmm_prior_on_the_device(tmp_path):
    """prior "GMM" with gm_fit_backend = "hip" set explicitly: both fits run on the device, the feed stays there, GM_prior_info.npz keeps the
    reference's keys in float64."""
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    model, tr = _train_gmm_prior(tmp_path, gm_fit_backend="hip", gm_random_state=7)
    assert isinstance(model.GM_prior_training, DeviceGaussianMixture)
    tr.train()
    assert tr.cur_epoch == 2 and np.isfinite(tr.elbo_train).all()
    assert isinstance(tr.GM_prior_final, DeviceGaussianMixture) and tr.GM_prior_final.max_iter == 2000
    for params in (tr.gm_params, tr.gm_final_params):
        assert all(isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32 for p in params)
        assert [tuple(p.shape) for p in params] == [(3,), (3, 16), (3, 16, 16)]
    gmi = np.load(os.path.join(str(tmp_path), "GM_prior_info.npz"))
    assert sorted(gmi.files) == sorted(["w_active", "m_active", "K_active", "w_full", "m_full", "K_full"])
    assert gmi["w_full"].dtype == gmi["K_full"].dtype == np.float64
    assert gmi["K_full"].shape == (3, 16, 16) and gmi["m_full"].shape == (3, 16) and abs(gmi["w_full"].sum() - 1) < 1e-9
    np.testing.assert_array_equal(gmi["K_full"], tr.GM_prior_final.covariances_)


def test_model_gmm_prior_keeps_sklearn_without_the_key(tmp_path):
    from sklearn.mixture import GaussianMixture
    model, _ = _train_gmm_prior(tmp_path)
    assert type(model.GM_prior_training) is GaussianMixture
