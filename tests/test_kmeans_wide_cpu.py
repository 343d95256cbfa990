"""The wide k-means (csrc/kmeans_wide.hip) without a GPU: the unchanged numpy restatement of tests/kmeans_ref.py passes its preconditions on every wide
case and gives sklearn's labels_ and n_iter_ exactly; the C ABI is declared, bound and refuses unsupported shapes; the config check knows
kmeans_backend "hip_wide"; the samples of the mixture-level GPU comparisons are admitted like a case."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_wide_ref as KW  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ladder_kmeans_wide_state_doubles", "ladder_kmeans_wide_workspace_bytes", "ladder_kmeans_wide_seed", "ladder_kmeans_wide_set_centres",
         "ladder_kmeans_wide_assign", "ladder_kmeans_wide_update")


@pytest.fixture(scope="module")
def lib_path():
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    return build.build(verbose=False)


@functools.lru_cache(maxsize=None)
def _sk(i):
    return KW.sklearn_fit(KW.CASES[i])[0]


def test_required_cases_are_present():
    shapes = {(c[0], c[1], c[2], c[6]) for c in KW.CASES}
    assert {(1300, 80, 33, None), (1000, 144, 17, None), (2049, 256, 50, None), (600, 256, 64, None), (333, 96, 1, None), (1500, 128, 6, "far"),
            (700, 256, 12, "far"), (4100, 256, 50, None)} <= shapes
    assert len(KW.N_ITER) == len(KW.CASES)
    assert all(64 < c[1] <= 256 and c[1] % 16 == 0 and 1 <= c[2] <= 64 for c in KW.CASES)


@pytest.mark.parametrize("i", range(len(KW.CASES)), ids=KW.IDS)
def test_restatement_equals_sklearn(i):
    """Labels and n_iter_ exactly; centres and inertia to round-off.  The preconditions are asserted inside the restatement."""
    case = KW.CASES[i]
    X, C = KW.data(case)
    ref = KW.NumpyKMeans(case[2]).fit(X, rs=np.random.RandomState(case[5]), init=C)
    sk = _sk(i)
    cerr = float(np.abs(ref.cluster_centers_ - sk.cluster_centers_).max())
    ierr = abs(ref.inertia_ - sk.inertia_) / sk.inertia_
    print("%s: n_iter %d / %d, centres abs %.3g, inertia rel %.3g" % (KW.IDS[i], ref.n_iter_, sk.n_iter_, cerr, ierr))
    assert ref.n_iter_ == sk.n_iter_ == KW.N_ITER[i]
    assert int((ref.labels_ != sk.labels_).sum()) == 0
    np.testing.assert_allclose(ref.cluster_centers_, sk.cluster_centers_, rtol=1e-10, atol=1e-12)
    assert ierr <= 1e-10
    if C is not None:
        assert ref.relocations_ == 1


def test_mixture_level_samples_pass_the_preconditions():
    """The data of the mixture-level GPU comparisons (tests/test_gpu_kmeans_wide.py) is admitted like a case."""
    import emgmm_wide_ref as W
    for i in KW.MIX_CASES:
        N, R, K, _mi, centres, spread, seed, _ = W.CASES[i]
        assert (N, R, K) in ((1500, 144, 3), (2051, 256, 2))
        lab = KW.assert_labels_are_decidable(W.data(N, R, centres, spread, seed)[0], K, W.KW["random_state"])
        assert tuple(np.bincount(lab, minlength=K)) == KW.MIX_COUNTS[i]


def test_kmeans_wide_abi_is_declared_and_bound():
    from ladder_latent_data_distribution_modelling_amd import _lib
    header = open(os.path.join(ROOT, "include", "ladder_hip.h")).read()
    for name in NAMES:
        assert name in _lib.PROTOTYPES, name
        assert name + "(" in header, name
        assert _lib.PROTOTYPES[name] == _lib.PROTOTYPES[name.replace("_wide", "")], name          # the signatures of the narrow entries
    assert _lib.ABI_VERSION == 2


def test_kmeans_wide_size_queries_refuse_unsupported_shapes(lib_path):
    import ctypes as C
    lib = C.CDLL(lib_path)
    for name in ("ladder_kmeans_wide_state_doubles", "ladder_kmeans_wide_workspace_bytes", "ladder_kmeans_state_doubles"):
        getattr(lib, name).restype = C.c_size_t
    assert lib.ladder_kmeans_wide_state_doubles(50, 256) == 50 * 256 + 4
    assert lib.ladder_kmeans_wide_workspace_bytes(20032, 50, 256) > 0
    for K, R in ((3, 64), (3, 72), (3, 272), (65, 80), (0, 80)):
        assert lib.ladder_kmeans_wide_state_doubles(K, R) == 0
        assert lib.ladder_kmeans_wide_workspace_bytes(1000, K, R) == 0
    assert lib.ladder_kmeans_wide_workspace_bytes(5, 6, 80) == 0                       # N < K
    for R in range(1, 300):                                                           # every width has at most one k-means
        narrow, wide = lib.ladder_kmeans_state_doubles(3, R) != 0, lib.ladder_kmeans_wide_state_doubles(3, R) != 0
        assert narrow == (R <= 64) and wide == (80 <= R <= 256 and R % 16 == 0)


def test_config_check_knows_the_wide_kmeans():
    from ladder_latent_data_distribution_modelling_amd.codes.mixture_fit import KMEANS_BACKENDS, check_device_fit_width, check_kmeans_backend
    assert KMEANS_BACKENDS == ("sklearn", "hip", "hip_wide")
    assert check_kmeans_backend("hip_wide") == "hip_wide"
    cfg = dict(prior="GMM", kmeans_backend="hip_wide")
    for fit in ("hip_wide", "sklearn"):
        for R in (8, 64, 80, 256):
            check_device_fit_width(dict(cfg, code_size=R, gm_fit_backend=fit))
        with pytest.raises(ValueError, match="kmeans_backend"):
            check_device_fit_width(dict(cfg, code_size=72, gm_fit_backend=fit))
    with pytest.raises(ValueError, match="kmeans_backend"):
        check_device_fit_width(dict(cfg, code_size=272))
    with pytest.raises(ValueError, match="kmeans_backend.*64.*hip_wide"):              # "hip" stays refused beyond 64 and now says where to go
        check_device_fit_width(dict(cfg, code_size=256, kmeans_backend="hip"))
    for prior in ("ours", "VampPrior"):                                               # the other priors: accepted, means "hip"
        check_device_fit_width(dict(prior=prior, code_size=256, representation_size=8, kmeans_backend="hip_wide"))
