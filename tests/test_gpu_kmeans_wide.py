"""Device k-means on 80 .. 256 dimensions (csrc/kmeans_wide.hip through codes/kmeans.py) against sklearn.cluster.KMeans itself on the cases of
tests/kmeans_wide_ref.py, as tests/test_gpu_kmeans.py does for the narrow kernels: labels_ and n_iter_ EXACTLY sklearn's (the preconditions asserted by
tests/test_kmeans_wide_cpu.py keep round-off from deciding them), cluster_centers_ and inertia_ to 1e-10 relative.  Then determinism, the C ABI's
refusals, the wide EM fit labelled on the device against the one labelled by sklearn, and the trainer with the host k-means forbidden."""
import functools
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emgmm_wide_ref as W  # noqa: E402
import kmeans_wide_ref as KW  # noqa: E402

pytestmark = pytest.mark.gpu

REL = 1e-10          # cluster_centers_ (per centre: max |difference| over max |coordinate|) and inertia_: the narrow test's bar


@functools.lru_cache(maxsize=None)
def _sklearn(i):
    sk, _ = KW.sklearn_fit(KW.CASES[i])
    return dict(labels=sk.labels_.astype(np.int32), n_iter=sk.n_iter_, centres=sk.cluster_centers_.copy(), inertia=float(sk.inertia_))


def _device(i, **kw):
    from ladder_latent_data_distribution_modelling_amd.codes.kmeans import DeviceKMeans
    case = KW.CASES[i]
    X, C = KW.data(case)
    km = DeviceKMeans(n_clusters=case[2], random_state=np.random.RandomState(case[5]), init="k-means++" if C is None else C)
    return km.fit(torch.as_tensor(X).cuda(), **kw)


@pytest.mark.parametrize("i", range(len(KW.CASES)), ids=KW.IDS)
def test_kmeans_wide_matches_sklearn(i):
    """k-means++ cases and the explicit-init cases with one relocation: zero mismatching labels, the same n_iter_."""
    ref, km = _sklearn(i), _device(i)
    mism = int((km.labels_ != ref["labels"]).sum())
    cerr = float((np.abs(km.cluster_centers_ - ref["centres"]).max(1) / np.abs(ref["centres"]).max(1)).max())
    ierr = abs(km.inertia_ - ref["inertia"]) / ref["inertia"]
    print("%s: mismatches %d, n_iter %d / %d, centres rel %.3g, inertia rel %.3g" % (KW.IDS[i], mism, km.n_iter_, ref["n_iter"], cerr, ierr))
    assert km.labels_dev.dtype == torch.int32 and km.labels_dev.is_cuda
    assert mism == 0
    assert km.n_iter_ == ref["n_iter"] == KW.N_ITER[i]
    assert cerr <= REL and ierr <= REL


def test_kmeans_wide_is_deterministic_and_independent_of_check_every():
    for i in (1, 5):                                                              # a k-means++ case and a relocation case
        assert (KW.CASES[i][6] is None) == (i == 1)
        a, b, c = _device(i, check_every=1), _device(i, check_every=16), _device(i, check_every=16)
        for other in (b, c):
            assert torch.equal(a._state, other._state) and torch.equal(a.labels_dev, other.labels_dev)
            assert (a.n_iter_, a.inertia_) == (other.n_iter_, other.inertia_)


def test_kmeans_picks_the_family_by_width_and_names_both_ranges():
    from ladder_latent_data_distribution_modelling_amd.codes.kmeans import DeviceKMeans
    for K, R in ((3, 72), (3, 272), (65, 80)):                                    # (which entries a taken width gets: tests/test_mixture_forms_cpu.py)
        with pytest.raises(NotImplementedError, match=r"n_features <= 64 or 80 <= n_features <= 256"):
            DeviceKMeans(n_clusters=K).fit(np.zeros((100, R), np.float32))


def test_kmeans_wide_abi_refuses_before_any_launch():
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    lib = L.load()
    st = torch.cuda.current_stream().cuda_stream
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device="cuda")
    x, draws, state = torch.zeros(80, 272, device="cuda"), f64(512), f64(65 * 272 + 4)
    labels = torch.zeros(80, dtype=torch.int32, device="cuda")
    ws = torch.zeros(4 << 20, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    need = lib.ladder_kmeans_wide_workspace_bytes(80, 2, 80)
    assert 0 < need <= ws.numel()
    # R = 64, 72, 272; K = 65; K > N; a workspace one byte short
    for N, K, R, nbytes in ((80, 3, 64, ws.numel()), (80, 3, 72, ws.numel()), (80, 3, 272, ws.numel()), (80, 65, 80, ws.numel()), (8, 9, 80, ws.numel()),
                            (80, 2, 80, need - 1)):
        assert lib.ladder_kmeans_wide_seed(p(x), N, K, R, p(draws), p(state), p(ws), nbytes, st) == -1
        assert lib.ladder_kmeans_wide_set_centres(p(x), N, K, R, p(draws), p(state), p(ws), nbytes, st) == -1
        assert lib.ladder_kmeans_wide_assign(p(x), N, K, R, 1, p(state), p(labels), p(ws), nbytes, st) == -1
        assert lib.ladder_kmeans_wide_update(p(x), N, K, R, p(labels), p(state), 1e-4, 300, 1, p(ws), nbytes, st) == -1
    # the narrow entries keep refusing what the wide ones take
    assert lib.ladder_kmeans_assign(p(x), 80, 2, 80, 1, p(state), p(labels), p(ws), ws.numel(), st) == -1
    torch.cuda.synchronize()
    assert float(state.abs().sum()) == 0.0 and int(ws.sum()) == 0 and int(labels.abs().sum()) == 0


def _fit(X, backend, **kw):
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return DeviceGaussianMixture(kmeans_backend=backend, **kw).fit(torch.as_tensor(X).cuda())


def _initial_labels(gm, X, random_state):
    from ladder_latent_data_distribution_modelling_amd.codes.mixture_fit import OneRank
    return gm._initial_labels(torch.as_tensor(X).cuda(), OneRank(), np.random.RandomState(random_state)).cpu().numpy()


@pytest.mark.parametrize("i", KW.MIX_CASES, ids=[W.IDS[i] for i in KW.MIX_CASES])
def test_wide_em_mixture_labelled_on_the_device_equals_the_sklearn_labelled_fit(i):
    N, R, K, max_iter, centres, spread, seed, n_iters = W.CASES[i]
    X = W.data(N, R, centres, spread, seed)[0]
    want = KW.assert_labels_are_decidable(X, K, W.KW["random_state"])
    kw = dict(n_components=K, max_iter=max_iter, **W.KW)
    hip, sk = _fit(X, "hip_wide", **kw), _fit(X, "sklearn", **kw)
    for gm in (hip, sk):
        assert np.array_equal(_initial_labels(gm, X, W.KW["random_state"]), want)
    assert hip.n_iter_ == sk.n_iter_ == n_iters[0] and hip.converged_ == sk.converged_
    W.assert_close_case(i, 0, hip, sk)
    W.assert_close_case(i, 0, sk, hip)


def test_trainer_gmm_prior_wide_never_runs_the_host_kmeans(tmp_path, monkeypatch):
    """The tiny config of tests/test_gpu_emgmm_wide.py::test_trainer_gmm_prior_wide_on_the_device with kmeans_backend = "hip_wide": two epochs with the
    host k-means made to raise."""
    from ladder_latent_data_distribution_modelling_amd.codes import mixture_fit
    from ladder_latent_data_distribution_modelling_amd.codes.data_loader import DataGenerator
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    from ladder_latent_data_distribution_modelling_amd.codes.models import MNISTModel_fashion
    from ladder_latent_data_distribution_modelling_amd.codes.trainers import MNISTTrainer_joint_training
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_golden import tiny_config

    def no_host_kmeans(*a, **k):
        raise AssertionError("the host k-means ran")

    monkeypatch.setattr(mixture_fit, "kmeans_labels", no_host_kmeans)
    cfg = tiny_config("mnist_fashion")
    cfg.update(prior="GMM", code_size=80, n_mixtures=2, batch_size=64, num_epochs=2, sg_pretraining=1, synthetic_n_train=256,
               synthetic_n_val=640, result_dir=str(tmp_path) + "/", checkpoint_dir=str(tmp_path) + "/", n_MC_samples=5,
               gm_fit_backend="hip_wide", kmeans_backend="hip_wide", gm_random_state=7)
    with pytest.raises(ValueError, match="kmeans_backend|gm_fit_backend"):
        MNISTModel_fashion(dict(cfg, code_size=72))
    model = MNISTModel_fashion(cfg)
    assert isinstance(model.GM_prior_training, DeviceGaussianMixture) and model.GM_prior_training.kmeans_backend == "hip_wide"
    tr = MNISTTrainer_joint_training(None, model, DataGenerator(cfg, None), cfg)
    tr.train()
    assert tr.cur_epoch == 2 and np.isfinite(tr.elbo_train).all()
    assert isinstance(tr.GM_prior_final, DeviceGaussianMixture) and tr.GM_prior_final.kmeans_backend == "hip_wide"
