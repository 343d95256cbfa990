"""Device EM fit of the "GMM" prior on 80 .. 256 dimensions (csrc/emgmm_wide.hip through codes/emgmm.py) against sklearn.mixture.GaussianMixture
itself, as tests/test_gpu_emgmm.py does for the narrow fit: same data, same `random_state` (hence the same k-means labels), cold fit, warm-started
refit on new samples of the same mixture; one GPU, sharded over two ranks, the C ABI's refusals, the status of a bad covariance, and the trainer."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emgmm_wide_ref as W  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_fit(dev, X, comm=None, **kw):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        if comm is None:
            dev.fit(X)
        else:
            dev.fit_sharded(X, comm, **kw)
    return len([x for x in w if x.category.__name__ == "ConvergenceWarning"])


def _check(i, f, dev, warned, snap):
    assert (dev.n_iter_, dev.converged_, warned) == (snap["n_iter_"], snap["converged_"], snap["warned"])
    W.assert_close_case(i, f, dev, W.Snap(snap))
    # the float32 feed copies are the rounded float64 parameters
    np.testing.assert_array_equal(dev.weights_dev.cpu().numpy(), dev.weights_.astype(np.float32))
    np.testing.assert_array_equal(dev.means_dev.cpu().numpy(), dev.means_.astype(np.float32))
    np.testing.assert_array_equal(dev.covariances_dev.cpu().numpy(), dev.covariances_.astype(np.float32))


@pytest.mark.parametrize("i", range(len(W.CASES)), ids=W.IDS)
def test_emgmm_wide_matches_sklearn(i):
    """Cold fit on X1, warm refit on X2: n_iter_, converged_ and the ConvergenceWarning equal sklearn's; lower bound to 1e-8, weights / means to 1e-7,
    covariances / precisions_cholesky_ to 1e-6 (tests/emgmm_ref.py: BARS).  One exception, derived in tests/emgmm_wide_ref.py: precisions_cholesky_ of
    the rank-deficient case's warm refit, where the float64 restatement NumpyEM is itself 14.33 times over that bar (condition number 1e6); its bar
    there is ten times NumpyEM's error, and the kernels measured 0.16 of it (0.48 of the unchanged bar on the cold fit)."""
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    N, R, K, max_iter, centres, spread, seed, _ = W.CASES[i]
    dev = DeviceGaussianMixture(n_components=K, max_iter=max_iter, **W.KW)
    for f, (X, snap) in enumerate(zip(W.data(N, R, centres, spread, seed), W.reference(i))):
        warned = _device_fit(dev, torch.as_tensor(X).cuda())
        _check(i, f, dev, warned, snap)


def test_emgmm_wide_does_not_depend_on_check_every():
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.engine import Comm
    i = 0
    N, R, K, max_iter, centres, spread, seed, _ = W.CASES[i]
    assert R == 80
    comm = Comm()
    assert not comm.on
    a, b = (DeviceGaussianMixture(n_components=K, max_iter=max_iter, **W.KW) for _ in range(2))
    for f, (X, snap) in enumerate(zip(W.data(N, R, centres, spread, seed), W.reference(i))):
        Xd = torch.as_tensor(X).cuda()
        wa = _device_fit(a, Xd, comm=comm, check_every=1)
        _device_fit(b, Xd, comm=comm, check_every=16)
        _check(i, f, a, wa, snap)
        assert a.n_iter_ == b.n_iter_ and a.lower_bound_ == b.lower_bound_ and a.converged_ == b.converged_
        for name in W.ATTRS:
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
    Xl = X[:550] if rank == 0 else X[550:]                                          # 550 + 550 samples, rank order
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


def test_emgmm_wide_sharded_fit_two_ranks_equals_sklearn(tmp_path):
    """Two processes (sharing cuda:0 over gloo) hold 550 + 550 samples of the R = 80 case and all-reduce the statistics every EM iteration; cold fit
    + warm refit reproduce sklearn's fit of the 1100 samples at the bars of the one-GPU fit, and both ranks end with bit-identical float64
    parameters."""
    i = 0
    N, R, K, max_iter, centres, spread, seed, _ = W.CASES[i]
    assert (N, R, K) == (1100, 80, 3)
    X1, X2 = W.data(N, R, centres, spread, seed)
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out")
    np.savez(inp, X1=X1, X2=X2, K=K, max_iter=max_iter)
    script = tmp_path / "emgmm_wide_shard_worker.py"
    script.write_text(SHARD_WORKER % dict(root=ROOT, port=36500 + os.getpid() % 2000))
    procs = [subprocess.Popen(["timeout", "-k", "10", "240", sys.executable, str(script), str(r), "2", inp, outp], stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True) for r in range(2)]
    outs = [p.communicate()[0] for p in procs]
    assert all(p.returncode == 0 for p in procs), [o[-2500:] for o in outs]
    got = [np.load(outp + ".%d.npz" % r) for r in range(2)]
    for f, snap in enumerate(W.reference(i)):
        g = got[0]
        assert (int(g["n_iter%d" % f]), bool(g["conv%d" % f]), int(g["warned%d" % f])) == (snap["n_iter_"], snap["converged_"], snap["warned"])
        W.assert_close_case(i, f, W.Snap(dict(lower_bound_=float(g["lb%d" % f]), weights_=g["w%d" % f], means_=g["m%d" % f],
                                              covariances_=g["c%d" % f], precisions_cholesky_=g["p%d" % f])), W.Snap(snap))
        for key in ("n_iter", "lb", "w", "m", "c", "p"):
            assert np.array_equal(got[0]["%s%d" % (key, f)], got[1]["%s%d" % (key, f)]), (key, f)


def test_emgmm_wide_abi_refuses_before_any_launch():
    """Device buffers far too small for a kernel that ran: a launch would have written past them or into them; they stay all zero."""
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
    x, buf, f32 = torch.zeros(64, 256, device="cuda"), f64(64), torch.zeros(64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    for Kb, Rb in ((3, 64), (3, 72), (3, 272), (65, 80)):
        assert lib.ladder_emgmm_wide_estep(x.data_ptr(), 8, Kb, Rb, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), ws.data_ptr(), ws.numel(),
                                           st) == -1
        assert lib.ladder_emgmm_wide_mstep(buf.data_ptr(), buf.data_ptr(), Kb, Rb, buf.data_ptr(), ws.data_ptr(), ws.numel(), 1e-6, 1e-3, 10, 1,
                                           f32.data_ptr(), f32.data_ptr(), f32.data_ptr(), st) == -1
        assert lib.ladder_emgmm_wide_prepare(buf.data_ptr(), Kb, Rb, ws.data_ptr(), ws.numel(), st) == -1
    for Rb in (64, 72, 272):
        assert lib.ladder_emgmm_wide_shift(x.data_ptr(), 8, Rb, buf.data_ptr(), st) == -1
    assert lib.ladder_emgmm_wide_shift(x.data_ptr(), 0, 80, buf.data_ptr(), st) == -1
    # the narrow exports keep refusing the wide widths
    assert lib.ladder_emgmm_estep(x.data_ptr(), 8, 3, 80, None, buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), ws.data_ptr(), ws.numel(), st) == -1
    assert lib.ladder_emgmm_prepare(buf.data_ptr(), 3, 80, st) == -1
    # a workspace one byte short
    K, R, N = 2, 80, 64
    state, stats = f64(lib.ladder_emgmm_wide_state_doubles(K, R)), f64(lib.ladder_emgmm_wide_stats_doubles(K, R))
    big = torch.zeros(max(lib.ladder_emgmm_wide_workspace_bytes(N, K, R), lib.ladder_emgmm_wide_mstep_workspace_bytes(K, R)), dtype=torch.uint8,
                      device="cuda")
    need_e, need_m = lib.ladder_emgmm_wide_workspace_bytes(N, K, R), lib.ladder_emgmm_wide_mstep_workspace_bytes(K, R)
    assert 0 < need_e <= big.numel() and 0 < need_m <= big.numel()
    assert lib.ladder_emgmm_wide_estep(x.data_ptr(), N, K, R, None, state.data_ptr(), buf.data_ptr(), stats.data_ptr(), big.data_ptr(), need_e - 1,
                                       st) == -3
    fw = torch.zeros(K * R * R, device="cuda")
    assert lib.ladder_emgmm_wide_mstep(stats.data_ptr(), buf.data_ptr(), K, R, state.data_ptr(), big.data_ptr(), need_m - 1, 1e-6, 1e-3, 10, 1,
                                       fw.data_ptr(), fw.data_ptr(), fw.data_ptr(), st) == -3
    assert lib.ladder_emgmm_wide_prepare(state.data_ptr(), K, R, big.data_ptr(), need_m - 1, st) == -3
    assert lib.ladder_emgmm_wide_estep(x.data_ptr(), 0, K, R, None, state.data_ptr(), buf.data_ptr(), stats.data_ptr(), big.data_ptr(), big.numel(),
                                       st) == -1
    torch.cuda.synchronize()
    for t in (buf, state, stats, f32, fw, ws, big):
        assert float(t.double().abs().sum()) == 0.0


def test_emgmm_wide_bad_covariance_is_a_status():
    """A covariance with a negative diagonal entry in a hand-made R = 80 state: -1 in the state, sklearn's ValueError in Python -- and the good
    component's precisions_cholesky_ is inv(cholesky(C)).T."""
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    K, R = 2, 80
    n = L.load().ladder_emgmm_wide_state_doubles(K, R)
    rng = np.random.default_rng(11)
    A = rng.normal(size=(R, R)) / np.sqrt(R)
    good = A @ A.T + 0.5 * np.eye(R)
    bad = good.copy()
    bad[37, 37] = -1.0
    host = np.zeros(n)
    host[0:K] = 0.5
    c0 = K + K * R
    host[c0:c0 + K * R * R] = np.stack([good, bad]).ravel()
    state = torch.as_tensor(host).cuda()
    gm = DeviceGaussianMixture(n_components=K)
    with pytest.raises(ValueError, match="ill-defined empirical covariance"):
        gm._prepare_state(state, R)
    tail = state[-4:].cpu().numpy()
    assert tail[2] == -1.0 and tail[3] == 1.0
    got = state.cpu().numpy()
    cstat = got[n - 4 - K:n - 4]
    assert list(cstat) == [0.0, -1.0]
    p0 = got[c0 + K * R * R:c0 + 2 * K * R * R].reshape(K, R, R)[0]
    want = np.linalg.inv(np.linalg.cholesky(good)).T
    err = np.abs(p0 - want).max() / np.abs(want).max()
    print("precisions_cholesky_ of the good component: max err / max |ref| = %.3e" % err)
    assert err <= 1e-13
    assert np.array_equal(np.tril(p0, -1), np.zeros((R, R)))
    logdet = got[c0 + 2 * K * R * R:c0 + 2 * K * R * R + K]
    assert abs(logdet[0] - np.log(np.diag(want)).sum()) <= 1e-12 * R
    host[c0 + R * R:c0 + 2 * R * R] = good.T.ravel() * 2.0                       # well-defined now: no error
    state = torch.as_tensor(host).cuda()
    gm._prepare_state(state, R)
    p1 = state.cpu().numpy()[c0 + K * R * R:c0 + 2 * K * R * R].reshape(K, R, R)[1]
    want1 = np.linalg.inv(np.linalg.cholesky(2.0 * good)).T
    assert np.abs(p1 - want1).max() <= 1e-13 * np.abs(want1).max()
    with pytest.raises(ValueError, match=r"80 \.\. 256 in steps of 16"):        # a width neither family takes
        DeviceGaussianMixture(n_components=2).fit(torch.zeros(100, 72, device="cuda"))


def test_trainer_gmm_prior_wide_on_the_device(tmp_path):
    """tests/test_gpu_model_wide_code.py::test_trainer_gmm_prior_wide_epochs with gm_fit_backend = "hip_wide": both fits run on the device, the feed
    stays there, the engine's mixture is the wide one, GM_prior_info.npz keeps the reference's keys in float64."""
    from ladder_latent_data_distribution_modelling_amd.codes.data_loader import DataGenerator
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.codes.models import MNISTModel_fashion
    from ladder_latent_data_distribution_modelling_amd.codes.trainers import MNISTTrainer_joint_training
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import tiny_config
    cfg = tiny_config("mnist_fashion")
    cfg.update(prior="GMM", code_size=80, n_mixtures=2, batch_size=64, num_epochs=2, sg_pretraining=1, synthetic_n_train=256,
               synthetic_n_val=640, result_dir=str(tmp_path) + "/", checkpoint_dir=str(tmp_path) + "/", n_MC_samples=5,
               gm_fit_backend="hip_wide", gm_random_state=7)
    with pytest.raises(ValueError, match="gm_fit_backend.*hip_wide"):
        MNISTModel_fashion(dict(cfg, code_size=72))
    model = MNISTModel_fashion(cfg)
    assert isinstance(model.GM_prior_training, DeviceGaussianMixture)
    tr = MNISTTrainer_joint_training(None, model, DataGenerator(cfg, None), cfg)
    tr.train()
    assert tr.cur_epoch == 2 and np.isfinite(tr.elbo_train).all()
    assert isinstance(tr.GM_prior_final, DeviceGaussianMixture) and tr.GM_prior_final.max_iter == 2000
    for params in (tr.gm_params, tr.gm_final_params):
        assert all(isinstance(p, torch.Tensor) and p.is_cuda and p.dtype == torch.float32 for p in params)
        assert [tuple(p.shape) for p in params] == [(2,), (2, 80), (2, 80, 80)]
    assert model.engine.mixture.wide
    gmi = np.load(os.path.join(str(tmp_path), "GM_prior_info.npz"))
    assert sorted(gmi.files) == sorted(["w_active", "m_active", "K_active", "w_full", "m_full", "K_full"])
    assert gmi["w_full"].dtype == gmi["m_full"].dtype == gmi["K_full"].dtype == np.float64
    assert gmi["K_full"].shape == (2, 80, 80) and gmi["m_full"].shape == (2, 80) and abs(gmi["w_full"].sum() - 1) < 1e-9
    np.testing.assert_array_equal(gmi["K_full"], tr.GM_prior_final.covariances_)
