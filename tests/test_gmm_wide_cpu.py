"""Host-side checks of the wide mixture and the wide sampler (include/ladder_hip.h section N21; 64 < R <= 256, R % 16 == 0) that need no GPU:
the size queries, the workspace bound that replaces the [S, K*R] product, argument validation that returns before any launch, and the
refusal of device fits on more than 64 dimensions."""
import ctypes

import pytest

E_SHAPE = -1


@pytest.fixture(scope="module")
def lib():
    from ladder_latent_data_distribution_modelling_amd import _lib
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    return _lib.load(build.build(verbose=False))


def test_size_queries(lib):
    a16 = lambda b: (b + 15) // 16 * 16
    n15 = lambda K, R: 16 + a16(8 * K) + a16(4 * K * (R + R * (R + 1) // 2))           # the sampler's layout: head of csrc/sample.hip
    for K, R in [(1, 80), (50, 256), (1024, 128)]:
        assert lib.ladder_gmm_wide_param_bytes(K, R) > 0, (K, R)
        assert lib.ladder_gmm_wide_prepare_workspace_bytes(K, R) > 0, (K, R)
        assert lib.ladder_mixture_sample_wide_param_bytes(K, R) == n15(K, R), (K, R)
        assert lib.ladder_mixture_sample_wide_prepare_workspace_bytes(K, R) > 0, (K, R)
    for R in (64, 72, 250, 272):
        assert lib.ladder_gmm_wide_param_bytes(5, R) == 0 and lib.ladder_mixture_sample_wide_param_bytes(5, R) == 0, R
        assert lib.ladder_gmm_wide_workspace_bytes(3, 4, R, 5) == 0, R
    for K in (0, 1025):
        assert lib.ladder_gmm_wide_param_bytes(K, 128) == 0, K
    for K in (0, -1):
        assert lib.ladder_mixture_sample_wide_param_bytes(K, 128) == 0, K
    # the limits of the narrow sampler stay where they were: every width has one form
    assert lib.ladder_mixture_sample_param_bytes(3, 80) == 0 and lib.ladder_mixture_sample_param_bytes(3, 64) > 0


def test_workspace_is_not_the_whitened_product(lib):
    """Y [S, K*R] of the GEMM form would be 4 S K R bytes; the wide term's whole workspace is at least eight times smaller at the shipped shape."""
    ws = lib.ladder_gmm_wide_workspace_bytes(100, 128, 256, 50)
    assert ws > 0 and 8 * ws <= 4 * 12800 * 50 * 256


@pytest.mark.parametrize("L,B,R", [(100, 128, 256), (7, 19, 128), (1, 1, 80), (100, 4, 96)])
def test_workspace_growth_in_K(lib, L, B, R):
    """Doubling K adds the new columns of q [S, K] and alignment only: nothing in the workspace is S * K * R."""
    S = L * B
    for K in (1, 3, 25, 50, 512):
        a, b = lib.ladder_gmm_wide_workspace_bytes(L, B, R, K), lib.ladder_gmm_wide_workspace_bytes(L, B, R, 2 * K)
        assert 0 < a <= b <= a + 4 * S * K + 4096, (K, a, b)


def test_shape_rejections_before_launch(lib):
    """R = 64 (the other forms' width), R = 264, n < 0, `first` outside [0, 2^56 - n] and u without eps are LADDER_E_SHAPE; the checks come before
    any pointer is touched or kernel launched (host buffers here)."""
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    big = 1 << 40
    samp = lambda K, R, n, first=0: lib.ladder_mixture_sample_wide(p, K, R, n, first, None, None, 1, 0, p, None, None)
    term = lambda K, R, L=3, B=4: lib.ladder_gmm_wide_logprob_fwd_bwd(p, p, p, p, L, B, R, K, p, p, p, p, big, None)
    rows = lambda K, R, n=5: lib.ladder_gmm_wide_logprob_rows(p, p, n, R, K, p, p, big, None)
    for R in (64, 264, 72, 0):
        assert samp(3, R, 8) == E_SHAPE and term(3, R) == E_SHAPE and rows(3, R) == E_SHAPE, R
        assert lib.ladder_gmm_wide_prepare(p, p, p, 3, R, p, p, big, None) == E_SHAPE
        assert lib.ladder_mixture_sample_wide_prepare(p, p, p, 3, R, p, p, big, None) == E_SHAPE
        assert lib.ladder_mixture_sample_wide_prepare_diag(p, p, 3, R, p, None) == E_SHAPE
    assert samp(3, 128, -1) == E_SHAPE and rows(3, 128, n=-1) == E_SHAPE
    assert term(3, 128, L=-1) == E_SHAPE and term(3, 128, B=0) == E_SHAPE and term(0, 128) == E_SHAPE and term(1025, 128) == E_SHAPE
    assert samp(0, 128, 8) == E_SHAPE
    assert samp(3, 128, 8, first=-1) == E_SHAPE and samp(3, 128, 8, first=2 ** 56 - 7) == E_SHAPE and samp(3, 128, 8, first=2 ** 56) == E_SHAPE
    assert lib.ladder_mixture_sample_wide(p, 3, 128, 8, 0, p, None, 1, 0, p, None, None) == E_SHAPE          # u without eps
    assert lib.ladder_mixture_sample_wide(p, 3, 128, 8, 0, None, p, 1, 0, p, None, None) == E_SHAPE          # eps without u
    assert lib.ladder_gmm_wide_logprob_fwd_bwd(p, p, p, p, 3, 4, 128, 3, p, p, None, p, big, None) == E_SHAPE  # dmu without dsd
    assert lib.ladder_gmm_wide_prepare(p, p, p, 0, 128, p, p, big, None) == E_SHAPE
    assert lib.ladder_mixture_sample_wide_prepare(p, p, p, 0, 128, p, p, big, None) == E_SHAPE


def test_empty_draw(lib):
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    assert lib.ladder_mixture_sample_wide(p, 3, 128, 0, 0, None, None, 1, 0, p, None, None) == 0           # nothing to draw: no launch
    assert lib.ladder_mixture_sample_wide(p, 3, 256, 0, 2 ** 56, None, None, 1, 0, p, None, None) == 0


def test_device_fit_refused_beyond_64_dimensions():
    """prior "GMM" fits on z: with code_size > 64 a device fit (csrc/emgmm.hip, csrc/kmeans.hip: R <= 64) cannot work, and the config says so."""
    from ladder_latent_data_distribution_modelling_amd.codes.mixture_fit import check_device_fit_width
    cfg = dict(prior="GMM", code_size=128, n_mixtures=6)
    check_device_fit_width(cfg)                                      # the defaults are the host fits
    check_device_fit_width(dict(cfg, gm_fit_backend="sklearn", kmeans_backend="sklearn"))
    with pytest.raises(ValueError, match="gm_fit_backend.*64"):
        check_device_fit_width(dict(cfg, gm_fit_backend="hip"))
    with pytest.raises(ValueError, match="kmeans_backend.*64"):
        check_device_fit_width(dict(cfg, kmeans_backend="hip"))
    check_device_fit_width(dict(cfg, code_size=64, gm_fit_backend="hip", kmeans_backend="hip"))
    check_device_fit_width(dict(cfg, prior="ours", gm_fit_backend="hip"))      # on t: codes/vbgmm.py checks the representation size itself
