"""The algorithm of csrc/kmeans.hip pinned against sklearn.cluster.KMeans without a GPU: the numpy restatement of tests/kmeans_ref.py passes its
preconditions on every case and gives sklearn's labels_ and n_iter_ exactly; codes/mixture_fit.py: kmeans_draws leaves the generator in the state a
sklearn fit leaves it in; the C ABI of the device k-means is declared, bound and refuses unsupported shapes."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_ref as KR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ladder_kmeans_state_doubles", "ladder_kmeans_draws_doubles", "ladder_kmeans_workspace_bytes", "ladder_kmeans_seed",
         "ladder_kmeans_set_centres", "ladder_kmeans_assign", "ladder_kmeans_update")


@pytest.fixture(scope="module")
def lib_path():
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    return build.build(verbose=False)


@functools.lru_cache(maxsize=None)
def _sk(i):
    return KR.sklearn_fit(KR.CASES[i])


def test_required_cases_are_present():
    shapes = {(c[0], c[1], c[2], c[6]) for c in KR.CASES}
    assert {(2000, 2, 10, None), (4097, 3, 7, None), (5000, 64, 50, None), (777, 5, 1, None), (1500, 3, 6, "far"), (4000, 16, 12, "far")} <= shapes


@pytest.mark.parametrize("i", range(len(KR.CASES)), ids=KR.IDS)
def test_restatement_equals_sklearn(i):
    """Labels and n_iter_ exactly; centres and inertia to round-off.  The preconditions are asserted inside the restatement."""
    case = KR.CASES[i]
    X, C = KR.data(case)
    ref = KR.NumpyKMeans(case[2]).fit(X, rs=np.random.RandomState(case[5]), init=C)
    sk, _ = _sk(i)
    assert ref.n_iter_ == sk.n_iter_
    assert int((ref.labels_ != sk.labels_).sum()) == 0
    np.testing.assert_allclose(ref.cluster_centers_, sk.cluster_centers_, rtol=1e-10, atol=1e-12)
    assert abs(ref.inertia_ - sk.inertia_) <= 1e-10 * sk.inertia_
    if C is not None:
        assert ref.relocations_ == 1
    else:
        np.testing.assert_array_equal(X[ref.seed_indices_].astype(np.float64)[0], X[ref.seed_indices_[0]])


@pytest.mark.parametrize("i", [i for i, c in enumerate(KR.CASES) if c[6] is None], ids=[s for s, c in zip(KR.IDS, KR.CASES) if c[6] is None])
def test_kmeans_draws_consumes_the_generator_as_sklearn_does(i):
    """After kmeans_draws the RandomState equals the one sklearn's fit leaves behind: a second restart stays aligned."""
    from ladder_latent_data_distribution_modelling_amd.codes.mixture_fit import kmeans_draws
    N, _R, K = KR.CASES[i][:3]
    _, rs_sk = _sk(i)
    rs = np.random.RandomState(KR.CASES[i][5])
    first, u = kmeans_draws(rs, N, K)
    assert 0 <= first < N and u.shape == (K - 1, 2 + int(np.log(K))) and ((u >= 0) & (u < 1)).all()
    a, b = rs.get_state(), rs_sk.get_state()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_mixture_level_samples_pass_the_preconditions():
    """The data of the mixture-level GPU comparisons (tests/test_gpu_kmeans.py) is admitted like a case."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import emgmm_ref as E
    N, R, K, _mi, centres, spread, seed, _ = E.CASES[0]
    KR.assert_labels_are_decidable(E.data(N, R, centres, spread, seed)[0], K, E.KW["random_state"])
    for N, R, K, seed in KR.MIX_VB:
        KR.assert_labels_are_decidable(KR.mixture_samples(N, R, K, seed), K, KR.MIX_RS)


def test_kmeans_abi_is_declared_and_bound():
    from ladder_latent_data_distribution_modelling_amd import _lib
    header = open(os.path.join(ROOT, "include", "ladder_hip.h")).read()
    for name in NAMES:
        assert name in _lib.PROTOTYPES, name
        assert name + "(" in header, name
    assert _lib.ABI_VERSION == 2


def test_kmeans_size_queries_refuse_unsupported_shapes(lib_path):
    import ctypes as C
    lib = C.CDLL(lib_path)
    for name in ("ladder_kmeans_state_doubles", "ladder_kmeans_workspace_bytes", "ladder_kmeans_draws_doubles"):
        getattr(lib, name).restype = C.c_size_t
    assert lib.ladder_kmeans_state_doubles(50, 64) == 50 * 64 + 4
    assert lib.ladder_kmeans_draws_doubles(50) == 1 + 49 * 5 and lib.ladder_kmeans_draws_doubles(1) == 1
    assert lib.ladder_kmeans_workspace_bytes(20096, 50, 64) > 0
    for K, R in ((3, 65), (65, 3), (0, 3)):
        assert lib.ladder_kmeans_state_doubles(K, R) == 0
        assert lib.ladder_kmeans_workspace_bytes(1000, K, R) == 0
    assert lib.ladder_kmeans_workspace_bytes(5, 6, 3) == 0                          # N < K
    assert lib.ladder_kmeans_draws_doubles(65) == 0 and lib.ladder_kmeans_draws_doubles(0) == 0
