"""The EM mixture fit of the "GMM" prior without a GPU: the module imports, the constructor's refusals, the C ABI is declared / exported /
bound, and the ALGORITHM the kernels implement (tests/emgmm_ref.py: shifted raw moments centred in the M-step, Cholesky, triangular inverse)
reproduces sklearn.mixture.GaussianMixture's cold and warm fits."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emgmm_ref as E  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_module_imports_and_constructor_refuses_what_it_does_not_cover():
    from ladder_latent_data_distribution_modelling_amd.codes.emgmm import DeviceGaussianMixture
    import codes.emgmm as alias
    assert alias.DeviceGaussianMixture is DeviceGaussianMixture
    gm = DeviceGaussianMixture(n_components=3, max_iter=7, warm_start=True, random_state=1)
    assert (gm.n_components, gm.max_iter, gm.tol, gm.reg_covar, gm.n_init) == (3, 7, 1e-3, 1e-6, 1)
    with pytest.raises(NotImplementedError):
        DeviceGaussianMixture(n_components=3, covariance_type="diag")
    with pytest.raises(NotImplementedError):
        DeviceGaussianMixture(n_components=3, init_params="random")
    for arg in ("weights_init", "means_init", "precisions_init"):
        with pytest.raises(NotImplementedError):
            DeviceGaussianMixture(n_components=3, **{arg: np.ones(3)})


def test_abi_is_declared_exported_and_bound():
    from ladder_latent_data_distribution_modelling_amd import _lib
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    header = open(os.path.join(ROOT, "include", "ladder_hip.h")).read()
    declared = set(re.findall(r"\b(ladder_emgmm_[a-z0-9_]+)\s*\(", header))
    assert {"ladder_emgmm_state_doubles", "ladder_emgmm_stats_doubles", "ladder_emgmm_workspace_bytes", "ladder_emgmm_estep",
            "ladder_emgmm_mstep"} <= declared
    assert "codes/base.py:101-106" in header and "699-710" in header and "749-767" in header
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in declared:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    # the size queries do no device work
    for name in ("ladder_emgmm_state_doubles", "ladder_emgmm_stats_doubles", "ladder_emgmm_workspace_bytes"):
        getattr(lib, name).restype = ctypes.c_size_t
    K, R = 30, 64
    assert lib.ladder_emgmm_stats_doubles(K, R) == 1 + K * (1 + R + R * R)
    assert lib.ladder_emgmm_state_doubles(K, R) >= K * (1 + R + 2 * R * R) + 4
    assert lib.ladder_emgmm_workspace_bytes(2048, K, R) >= 2048 * K * 8 and lib.ladder_emgmm_workspace_bytes(0, K, R) == 0
    assert int(re.search(r"#define LADDER_ABI_VERSION (\d+)", header).group(1)) == 2


@pytest.mark.parametrize("case", [E.CASES[0], E.CASES[2], E.CASES[7], E.CASES[8]], ids=["600x3x7", "1100x33x6", "129x5x1", "257x17x2"])
def test_numpy_restatement_reproduces_sklearn(case):
    """Cold fit + warm refit: same iteration count and convergence, lower bound and parameters to 1e-10 (measured: lower bound 3e-15, weights 2e-14,
    means 1e-14, covariances 2e-14, precisions_cholesky_ 3e-12, relative to each array's largest magnitude)."""
    from sklearn.cluster import KMeans
    from sklearn.mixture import GaussianMixture
    from sklearn.utils import check_random_state
    N, R, K, max_iter, centres, spread, seed, n_iters = case
    X1, X2 = E.data(N, R, centres, spread, seed)
    ref = GaussianMixture(n_components=K, max_iter=max_iter, **E.KW)
    mine = E.NumpyEM(K, tol=E.KW["tol"], reg_covar=E.KW["reg_covar"], max_iter=max_iter)
    labels = KMeans(n_clusters=K, n_init=1, random_state=check_random_state(E.KW["random_state"])).fit(X1.astype(np.float64)).labels_
    for X, lab, n_iter in ((X1, labels, n_iters[0]), (X2, None, n_iters[1])):
        E.sklearn_fit(ref, X)
        E.assert_iteration_count_is_decidable(ref, E.KW["tol"], max_iter)
        mine.fit(X, lab)
        assert ref.n_iter_ == n_iter and mine.n_iter_ == n_iter and mine.converged_ == ref.converged_
        assert abs(mine.lower_bound_ - ref.lower_bound_) <= 1e-10 * abs(ref.lower_bound_)
        for name in ("weights_", "means_", "covariances_", "precisions_cholesky_"):
            a, b = getattr(mine, name), getattr(ref, name)
            err = np.abs(a - b).max() / np.abs(b).max()
            print(name, err)
            assert err <= 1e-10, (name, err)
