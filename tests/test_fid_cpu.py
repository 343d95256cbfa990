"""The host side of the FID evaluation (ladder_latent_data_distribution_modelling_amd/fid.py), no GPU: the float64 Frechet distance against the closed
form and against the svd restatement of tf.contrib.gan's rule, the weight loader, the refusals, the CLI's uint8 rule and the preprocess reference."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_ref as R  # noqa: E402

from ladder_latent_data_distribution_modelling_amd import fid as F  # noqa: E402


def test_frechet_closed_form_diagonal():
    """Commuting (diagonal) covariances: FID = sum (sqrt a - sqrt b)^2 + |dm|^2."""
    rng = np.random.default_rng(0)
    for D in (1, 7, 64):
        a, b = rng.uniform(0.1, 5.0, D), rng.uniform(0.1, 5.0, D)
        m1, m2 = rng.standard_normal(D), rng.standard_normal(D)
        want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((m1 - m2) ** 2).sum()
        got = F.frechet_distance(m1, np.diag(a), m2, np.diag(b))
        assert abs(got - want) <= 1e-12 * abs(want), (D, got, want)


@pytest.mark.parametrize("n,D", [(24, 64), (200, 48), (64, 512)])
def test_frechet_matches_svd_restatement(n, D):
    """eigh form == svd form (the contrib code as written), rank-deficient sets (n < D) included."""
    rng = np.random.default_rng(n + D)
    fa = rng.standard_normal((n, D)) * rng.uniform(0.2, 3.0, D) + rng.standard_normal(D)
    fb = rng.standard_normal((n + 3, D)) * rng.uniform(0.2, 3.0, D) + rng.standard_normal(D)
    (m1, c1), (m2, c2) = R.stats64(fa), R.stats64(fb)
    got, want = F.frechet_distance(m1, c1, m2, c2), R.frechet_svd(m1, c1, m2, c2)
    print("n %d D %d eigh %.17g svd %.17g rel %.3g" % (n, D, got, want, abs(got - want) / abs(want)))
    assert abs(got - want) <= 1e-12 * abs(want)


@pytest.mark.parametrize("n,D", [(24, 64), (200, 48), (64, 512)])
def test_frechet_of_a_set_with_itself(n, D):
    rng = np.random.default_rng(3 * n + D)
    f = rng.standard_normal((n, D)) * rng.uniform(0.2, 3.0, D) + 5.0
    m, c = R.stats64(f)
    got = F.frechet_distance(m, c, m, c)
    print("n %d D %d self-FID %.3g at trace %.4g" % (n, D, got, 2 * np.trace(c)))
    assert abs(got) <= 1e-12 * 2 * np.trace(c)


def test_sqrt_rule_threshold():
    """An eigenvalue at 1e-11 is left as it is, one at 1e-9 is replaced by its root (threshold 1e-10 on |lambda|); signs are kept."""
    root, tr = F.sqrtm_sym(np.diag([1e-11, 1e-9, 4.0, -1e-11, -9.0]))
    want = np.array([1e-11, np.sqrt(1e-9), 2.0, -1e-11, -3.0])
    assert np.allclose(np.diag(root), want, rtol=1e-14, atol=0) and np.allclose(root - np.diag(np.diag(root)), 0, atol=1e-300)
    assert abs(tr - want.sum()) <= 1e-15 * np.abs(want).sum()
    # rotated: the same eigenvalues behind an orthogonal basis (eigh resolves 1e-11 beside 4 to ~1e-16 absolute)
    q, _ = np.linalg.qr(np.random.default_rng(1).standard_normal((3, 3)))
    root, _ = F.sqrtm_sym(q @ np.diag([1e-11, 1e-9, 4.0]) @ q.T)
    ev = np.sort(np.linalg.eigvalsh(root))
    assert abs(ev[0] - 1e-11) < 1e-14 and abs(ev[1] - np.sqrt(1e-9)) < 1e-10 and abs(ev[2] - 2.0) < 1e-12
    assert np.allclose(R.sqrt_svd(q @ np.diag([1e-11, 1e-9, 4.0]) @ q.T), root, atol=1e-14)


def test_weight_loader(tmp_path):
    w = R.random_weights(0)
    assert len(w) == 26 and [n for n, _, _ in F.vgg16_layers()][:3] == ["block1_conv1", "block1_conv2", "block2_conv1"]
    got = F.load_vgg16_weights(w)
    assert set(got) == set(w) and all(got[k].dtype == np.float32 and np.array_equal(got[k], w[k]) for k in w)
    path = str(tmp_path / "vgg16.npz")
    np.savez(path, **w)
    got = F.load_vgg16_weights(path)
    assert all(np.array_equal(got[k], w[k]) for k in w)
    missing = dict(w)
    del missing["block3_conv2/bias"]
    with pytest.raises(KeyError, match="block3_conv2/bias"):
        F.load_vgg16_weights(missing)
    transposed = dict(w)
    transposed["block2_conv1/kernel"] = np.ascontiguousarray(w["block2_conv1/kernel"].transpose(3, 2, 0, 1))      # OIHW instead of HWIO
    with pytest.raises(ValueError, match="block2_conv1/kernel"):
        F.load_vgg16_weights(transposed)


def test_refusals():
    from ladder_latent_data_distribution_modelling_amd.codes import utils
    import codes.utils as alias
    assert alias.compute_FID_score is utils.compute_FID_score
    with pytest.raises(NotImplementedError, match='only "VGG"'):
        utils.compute_FID_score("a.npz", "b.npz", "inception", "avg", weights=R.random_weights(0))
    with pytest.raises(ValueError, match="block\\{b\\}_conv\\{i\\}/kernel"):
        utils.compute_FID_score("a.npz", "b.npz", "VGG", "avg")                 # weights=None: says where they are expected
    with pytest.raises(ValueError, match="at least 32"):
        utils.compute_FID_score("a.npz", "b.npz", "VGG", "avg", weights=R.random_weights(0), input_size=31)
    with pytest.raises(ValueError, match="pooling"):
        utils.compute_FID_score("a.npz", "b.npz", "VGG", "mean", weights=R.random_weights(0))


def test_cli_reads_uint8_as_original(tmp_path):
    u8, f32 = np.zeros((2, 4, 4, 3), np.uint8), np.zeros((2, 4, 4, 3), np.float32)
    assert F.second_set_for(u8)[0] == "original" and "uint8" in F.second_set_for(u8)[1]
    assert F.second_set_for(f32) == ("generated", None)
    assert F.second_set_for(u8, "generated") == ("generated", None) and F.second_set_for(f32, "original") == ("original", None)
    a = F.parse_args(["--real", "a.npz", "--generated", "b.npz", "--weights", "w.npz"])
    assert (a.pooling, a.chunk, a.second_set, a.input_size) == ("avg", 256, None, 64)
    path = str(tmp_path / "b.npz")
    np.savez(path, sampled_images=u8)
    assert F.load_images(path).dtype == np.uint8 and F.load_images(f32) is f32


def test_preprocess_reference_is_the_reference_arithmetic():
    """fid_ref.preprocess_ref against preprocess_input_original / _generated + the legacy bilinear resize written out in numpy (float64);
    values outside [0, 1] are clipped in "generated" and NOT in "original"."""
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.4, 1.5, (2, 7, 9, 3)).astype(np.float32)
    x[0, 0, 0] = [-0.25, 1.25, 0.5]

    def resize(t, oh, ow):
        N, H, W, C = t.shape
        out = np.empty((N, oh, ow, C))
        for i in range(oh):
            sy = i * (H / oh)
            y0 = int(np.floor(sy))
            y1, fy = min(y0 + 1, H - 1), sy - y0
            for j in range(ow):
                sx = j * (W / ow)
                x0 = int(np.floor(sx))
                x1, fx = min(x0 + 1, W - 1), sx - x0
                top = t[:, y0, x0] + (t[:, y0, x1] - t[:, y0, x0]) * fx
                bot = t[:, y1, x0] + (t[:, y1, x1] - t[:, y1, x0]) * fx
                out[:, i, j] = top + (bot - top) * fy
        return out

    for oh, ow in ((5, 4), (7, 9), (14, 18)):
        gen = resize((np.clip(x.astype(np.float64), 0.0, 1.0) - 0.5) * 2.0, oh, ow)
        org = resize((x.astype(np.float64) / 255.0 - 0.5) * 2.0, oh, ow)
        assert np.abs(R.preprocess_ref(x, "generated", oh, ow).numpy() - gen).max() < 1e-14
        assert np.abs(R.preprocess_ref(x, "original", oh, ow).numpy() - org).max() < 1e-14
    same = R.preprocess_ref(x, "generated", 7, 9).numpy()
    assert same[0, 0, 0, 0] == -1.0 and same[0, 0, 0, 1] == 1.0 and same.min() >= -1.0 and same.max() <= 1.0
    org = R.preprocess_ref(x, "original", 7, 9).numpy()
    assert org[0, 0, 0, 0] < -1.0                                 # -0.25 / 255 is below 0 and stays there: "original" does not clip
    u8 = rng.integers(0, 256, (1, 4, 4, 3), dtype=np.uint8)
    assert np.abs(R.preprocess_ref(u8, "original", 4, 4).numpy() - (u8 / 255.0 - 0.5) * 2.0).max() < 1e-15
