"""FID evaluation on the device (csrc/fid.hip, ladder_latent_data_distribution_modelling_amd/fid.py) against float64 references: the streaming moments,
the two pools, the preprocess + resize kernel, the VGG16 stack, compute_FID_score end to end, generate(sink=...) and the trainer's compute_FID."""
import functools
import json
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -53        # unit round-offs
SENT = -7.0e33


def _L():
    from ladder_latent_data_distribution_modelling_amd import _lib
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def _guarded(n, dtype=torch.float32, pad=64):
    """A device buffer of n elements followed by `pad` sentinels: (whole buffer, view of the n elements)."""
    buf = torch.full((n + pad,), SENT, dtype=dtype, device="cuda")
    return buf, buf[:n]


def _intact(buf, n):
    return bool((buf[n:] == SENT).all().item())


@functools.lru_cache(maxsize=None)
def weights():
    return R.random_weights(0)


# ------------------------------------------------------------------------------------------------ moments
CHUNKINGS = {1: [1], 3: [2, 1], 4: [1, 3], 5: [2, 3], 67: [5, 1, 61]}


def run_moments(x, chunks):
    """Streams x [n, D] (fp32 numpy) through ladder_moments_accumulate in `chunks`; state and workspace sit in front of sentinels.  -> host state."""
    L, D = _L(), x.shape[1]
    nd = L.query("ladder_moments_state_doubles", D)
    assert nd == 2 + 2 * D + D * D
    sbuf, state = _guarded(nd, torch.float64)
    state.zero_()
    lo = 0
    for b in chunks:
        nb = L.query("ladder_moments_workspace_bytes", b, D)
        assert nb > 0 and nb % 8 == 0
        wbuf, ws = _guarded(nb // 8, torch.float64)
        xd = torch.as_tensor(np.ascontiguousarray(x[lo:lo + b])).cuda()                 # exactly b * D floats
        L.call("ladder_moments_accumulate", xd.data_ptr(), b, D, state.data_ptr(), ws.data_ptr(), nb, _st())
        torch.cuda.synchronize()
        assert _intact(wbuf, nb // 8)
        lo += b
    assert lo == x.shape[0] and _intact(sbuf, nd)
    return state.cpu().numpy()


def dyadic(n, D, first, seed):
    """Small integers / 8 whose column sums over the first `first` rows and over all n rows are multiples of first / of n (in eighths).  Then the shift
    c (the first chunk's column mean, whether that chunk is the first `first` rows or all n) and the mean are themselves multiples of 1/8, x - c is a
    small multiple of 1/8, and every product, every partial sum, s s^T / n and S - s s^T / n are exactly representable: nothing rounds before the one
    multiplication by 1 / (n - 1) that np.cov performs too.  (With an arbitrary column mean, c carries 24 significant bits and the squares of x - c
    need more than 53: the sums would no longer be exact and no summation order could be compared bit for bit.)"""
    k = np.random.default_rng(seed).integers(-16, 17, (n, D))
    k[first - 1] -= k[:first].sum(0) % first
    k[n - 1] -= k.sum(0) % n
    assert not (k[:first].sum(0) % first).any() and not (k.sum(0) % n).any()
    return (k / 8.0).astype(np.float32)


def cov64(x):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.asarray(np.cov(x.astype(np.float64), rowvar=False)).reshape(x.shape[1], x.shape[1])


@pytest.mark.parametrize("n", [1, 3, 4, 5, 67])
@pytest.mark.parametrize("D", [1, 15, 16, 17, 80])
def test_moments_exact_on_dyadic_data(gpu_ctx, D, n):
    from ladder_latent_data_distribution_modelling_amd.fid import moments_from_state
    chunks = CHUNKINGS[n]
    x = dyadic(n, D, chunks[0], 100 * D + n)
    x64 = x.astype(np.float64)
    results = []
    for ch in ([n], chunks):
        state = run_moments(x, ch)
        c = (x64[:ch[0]].sum(0) / ch[0]).astype(np.float32).astype(np.float64)
        a = x64 - c
        assert state[0] == n and state[1] == D
        assert np.array_equal(state[2:2 + D], c) and np.array_equal(state[2 + D:2 + 2 * D], a.sum(0))
        assert np.array_equal(np.triu(state[2 + 2 * D:].reshape(D, D)), np.triu(a.T @ a))
        cnt, mean, cov = moments_from_state(state, D)
        assert cnt == n and np.array_equal(mean, x64.mean(0))
        assert np.array_equal(cov, cov64(x), equal_nan=True) and (n == 1 or np.isfinite(cov).all())
        results.append((mean, cov))
    assert np.array_equal(results[0][0], results[1][0]) and np.array_equal(results[0][1], results[1][1], equal_nan=True)


def moments_bounds(x, c, nchunks):
    """Entry-wise bounds on |mean - np.mean| and |cov - np.cov| for fp32 data x [n, D] shifted by c, u = 2^-53.

    a = x - c is exact (x and c are fp32 numbers of like magnitude: their difference has well under 53 bits), and so is every product a_i a_j
    (2 x 24 bits).  S_ij is a sum of n such products taken in some fixed order over MFMA steps, <= 16 partial tiles and the chunks: at most n + 16 +
    nchunks additions touch a term, so |dS_ij| <= (n + 16 + nchunks) u A_ij with A_ij = sum_r |a_ri| |a_rj|.  Likewise |ds_i| <= (n + nchunks) u B_i,
    B_i = sum_r |a_ri|.  cov_ij = (S_ij - s_i s_j / n) * (1 / (n - 1)) adds four roundings on terms no larger than |S_ij| + |s_i s_j| / n and carries
    (|s_i| ds_j + |s_j| ds_i) / n.  np.cov, the float64 reference, centres on its own mean and sums the same n products: its own error is bounded by
    (n + 4) u A'_ij with A' taken about the mean.  mean_i = c_i + s_i / n: ds_i / n + 2 u |mean_i|, and np.mean's own sum of n numbers of size |x|:
    n u max|x_i|."""
    n = x.shape[0]
    x64 = x.astype(np.float64)
    a, am = np.abs(x64 - c), np.abs(x64 - x64.mean(0))
    A, Am, B = a.T @ a, am.T @ am, a.sum(0)
    s = (x64 - c).sum(0)
    S = (x64 - c).T @ (x64 - c)
    ds = (n + nchunks) * U64 * B
    cov_tol = ((n + 16 + nchunks) * U64 * A + (n + 4) * U64 * Am + 4 * U64 * (np.abs(S) + np.abs(np.outer(s, s)) / n)
               + (np.outer(np.abs(s), ds) + np.outer(ds, np.abs(s))) / n) / max(n - 1, 1)
    mean_tol = ds / n + 2 * U64 * np.abs(x64.mean(0)) + n * U64 * np.abs(x64).max(0)
    return mean_tol, cov_tol


@pytest.mark.parametrize("n", [1, 3, 4, 5, 67])
@pytest.mark.parametrize("D", [1, 15, 16, 17, 80])
def test_moments_normal_data_with_offset(gpu_ctx, D, n):
    from ladder_latent_data_distribution_modelling_amd.fid import moments_from_state
    x = (50.0 + np.random.default_rng(7 * D + n).standard_normal((n, D))).astype(np.float32)
    for ch in ([n], CHUNKINGS[n]):
        state = run_moments(x, ch)
        again = run_moments(x, ch)
        assert np.array_equal(state.view(np.uint64), again.view(np.uint64))                  # same chunking, same bits
        cnt, mean, cov = moments_from_state(state, D)
        mean_tol, cov_tol = moments_bounds(x, state[2:2 + D], len(ch))
        assert cnt == n and (np.abs(mean - x.astype(np.float64).mean(0)) <= mean_tol).all()
        if n > 1:
            err = np.abs(cov - cov64(x))
            print("D %d n %d chunks %s: max cov err / bound %.3g, max rel err %.3g" % (D, n, ch, (err / cov_tol).max(), (err / np.abs(cov64(x)).max()).max()))
            assert (err <= cov_tol).all()


def test_moments_symmetric_mirror_many_tiles(gpu_ctx):
    """D = 512: 36 upper tiles; a chunk of 200 rows (4 row splits), then one of 100 (2 row splits)."""
    from ladder_latent_data_distribution_modelling_amd.fid import moments_from_state
    D, n = 512, 300
    x = (50.0 + np.random.default_rng(1).standard_normal((n, D)) * np.linspace(0.5, 2.0, D)).astype(np.float32)
    state = run_moments(x, [200, 100])
    S = state[2 + 2 * D:].reshape(D, D)
    assert not S[64:, :64].any() and S[:64, 64:].all()            # tiles below the diagonal are never written, those above are
    _, mean, cov = moments_from_state(state, D)
    assert np.array_equal(cov, cov.T)
    mean_tol, cov_tol = moments_bounds(x, state[2:2 + D], 2)
    assert (np.abs(cov - cov64(x)) <= cov_tol).all() and (np.abs(mean - x.astype(np.float64).mean(0)) <= mean_tol).all()


def test_moments_refusals(gpu_ctx):
    L = _L()
    x, st = torch.zeros(8, device="cuda"), torch.zeros(64, dtype=torch.float64, device="cuda")
    ws = torch.zeros(L.query("ladder_moments_workspace_bytes", 2, 4), dtype=torch.uint8, device="cuda")
    with pytest.raises(L.LadderHipError, match="LADDER_E_SHAPE"):
        L.call("ladder_moments_accumulate", x.data_ptr(), 2, 0, st.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    with pytest.raises(L.LadderHipError, match="LADDER_E_WORKSPACE"):
        L.call("ladder_moments_accumulate", x.data_ptr(), 2, 4, st.data_ptr(), ws.data_ptr(), ws.numel() - 8, _st())
    assert L.query("ladder_moments_state_doubles", 0) == 0 and L.query("ladder_moments_workspace_bytes", 0, 4) == 0


def test_moments_refuse_another_width_on_the_device(gpu_ctx):
    """The D of a state is fixed by its first chunk; the host cannot see it without synchronising, so a later chunk of another width is refused on the
    device: nothing but the row count changes, and that becomes NaN, which the reader turns into an error."""
    from ladder_latent_data_distribution_modelling_amd.fid import moments_from_state
    L = _L()
    nd = L.query("ladder_moments_state_doubles", 4)
    sbuf, state = _guarded(nd, torch.float64)
    state.zero_()
    ws = torch.zeros(L.query("ladder_moments_workspace_bytes", 3, 5), dtype=torch.uint8, device="cuda")
    x4, x5 = torch.rand(3, 4, device="cuda"), torch.rand(3, 5, device="cuda")
    L.call("ladder_moments_accumulate", x4.data_ptr(), 3, 4, state.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    before = state.cpu().numpy()
    L.call("ladder_moments_accumulate", x5.data_ptr(), 3, 5, state.data_ptr(), ws.data_ptr(), ws.numel(), _st())
    after = state.cpu().numpy()
    assert before[0] == 3 and before[1] == 4 and np.isnan(after[0]) and np.array_equal(after[1:], before[1:]) and _intact(sbuf, nd)
    with pytest.raises(ValueError, match="another feature width"):
        moments_from_state(after, 4)


# ------------------------------------------------------------------------------------------------ pools
@pytest.mark.parametrize("C", [1, 3, 4, 64])
@pytest.mark.parametrize("H,W", [(2, 2), (3, 5), (7, 4)])
def test_maxpool2x2(gpu_ctx, H, W, C):
    L, N = _L(), 2
    x = (-1.0 - np.random.default_rng(H * 100 + W * 10 + C).random((N, H, W, C))).astype(np.float32)          # all negative: a zero-initialised maximum fails
    ref = torch.nn.functional.max_pool2d(torch.as_tensor(x).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1).numpy()
    n_out = ref.size
    buf, y = _guarded(n_out)
    L.call("ladder_maxpool2x2_fwd", torch.as_tensor(x).cuda().data_ptr(), y.data_ptr(), N, H, W, C, _st())
    torch.cuda.synchronize()
    assert ref.shape == (N, H // 2, W // 2, C) and np.array_equal(y.cpu().numpy().reshape(ref.shape), ref) and _intact(buf, n_out)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 4), (5, 1)])
def test_maxpool2x2_refuses_an_empty_output(gpu_ctx, H, W):
    L = _L()
    x, y = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    with pytest.raises(L.LadderHipError, match="LADDER_E_SHAPE"):
        L.call("ladder_maxpool2x2_fwd", x.data_ptr(), y.data_ptr(), 1, H, W, 4, _st())


@pytest.mark.parametrize("kind", ["avg", "max"])
@pytest.mark.parametrize("C", [1, 4, 512])
@pytest.mark.parametrize("HW", [1, 4, 9])
def test_global_pool(gpu_ctx, HW, C, kind):
    L, N = _L(), 3
    x = (np.random.default_rng(HW * 1000 + C).standard_normal((N, HW, C)) - 2.0).astype(np.float32)
    buf, y = _guarded(N * C)
    L.call("ladder_global_pool", torch.as_tensor(x).cuda().data_ptr(), y.data_ptr(), N, HW, C, 0 if kind == "avg" else 1, _st())
    torch.cuda.synchronize()
    got = y.cpu().numpy().reshape(N, C)
    assert _intact(buf, N * C)
    if kind == "max":
        assert np.array_equal(got, x.max(1))
    else:
        # fp32 sum of HW terms in index order (HW - 1 roundings, each <= u * sum |x|) and one division: HW * u * sum |x| / HW
        tol = HW * U32 * np.abs(x.astype(np.float64)).sum(1) / HW
        assert (np.abs(got - x.astype(np.float64).mean(1)) <= tol).all()


# ------------------------------------------------------------------------------------------------ preprocess + resize
@pytest.mark.parametrize("mode", ["original", "generated"])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("geo", [(2, 128, 128, 64, 64), (3, 7, 9, 5, 4), (2, 16, 16, 64, 64)])
def test_fid_preprocess(gpu_ctx, geo, u8, mode):
    L = _L()
    N, H, W, OH, OW = geo
    rng = np.random.default_rng(H + 3 * OW + u8)
    if u8:
        x = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    else:
        x = (rng.uniform(-0.2, 1.3, (N, H, W, 3)) * (255.0 if mode == "original" else 1.0)).astype(np.float32)      # below 0 and above 1 (x 255: the byte scale)
        assert x.min() < 0 and x.max() > (255.0 if mode == "original" else 1.0)
    ref = R.preprocess_ref(x, mode, OH, OW).numpy()
    taps = R.preprocess_ref(x, mode, H, W).numpy()                      # the preprocessed source pixels (no resize at equal size)
    buf, y = _guarded(ref.size)
    L.call("ladder_fid_preprocess", torch.as_tensor(x).cuda().data_ptr(), int(u8), y.data_ptr(), N, H, W, 3, OH, OW, 0 if mode == "original" else 1, _st())
    torch.cuda.synchronize()
    got = y.cpu().numpy().reshape(ref.shape)
    assert _intact(buf, ref.size)
    # Bound, u = 2^-24, P = max |preprocessed tap|.  A tap: v / 255 (one rounding), - 0.5 (one rounding on a number <= P / 2 + 1), * 2 (exact); the clip is
    # exact: |dp| <= 4 u (P + 1).  One interpolation t0 + (t1 - t0) * f in fp32: the difference (<= 2 P) rounds once, the fp32 weight f carries a relative
    # u, the product and the sum round once each (or once together when fused): <= 7 u P, and a convex combination does not amplify what its inputs carry.
    # Two levels (along x, then along y): 14 u P + 4 u (P + 1) <= 18 u (P + 1).  An exact pick (128 -> 64) interpolates nothing: 4 u (P + 1).
    P = np.abs(taps).max()
    exact_pick = H % OH == 0 and W % OW == 0 and H >= OH
    tol = (4 if exact_pick else 18) * U32 * (P + 1.0)
    err = np.abs(got - ref).max()
    print("geo %s u8 %s %s: err %.3g, bound %.3g" % (geo, u8, mode, err, tol))
    assert err <= tol
    if mode == "generated":
        assert got.min() >= -1.0 and got.max() <= 1.0
    elif not u8:
        assert got.min() < -1.0 and got.max() > 1.0                     # "original" does not clip


def test_fid_preprocess_refuses(gpu_ctx):
    L = _L()
    x, y = torch.zeros(256, device="cuda"), torch.zeros(256, device="cuda")
    for args in ((1, 4, 4, 4, 2, 2, 0), (1, 4, 4, 3, 0, 2, 0), (1, 4, 4, 3, 2, 2, 2)):          # C != 3, empty output, unknown mode
        with pytest.raises(L.LadderHipError, match="LADDER_E_SHAPE"):
            L.call("ladder_fid_preprocess", x.data_ptr(), 0, y.data_ptr(), *args, _st())


# ------------------------------------------------------------------------------------------------ the VGG16 stack
STACK_CASES = {"32": (3, (32, 32)), "40x48": (2, (40, 48))}


@functools.lru_cache(maxsize=None)
def stack_case(key):
    """Input, float64 features and fp32-CPU features of a case for all three poolings (computed once, never modified)."""
    N, hw = STACK_CASES[key]
    x = np.random.default_rng(len(key)).uniform(-1.0, 1.0, (N,) + hw + (3,)).astype(np.float32)
    t = torch.as_tensor(x)
    return x, {p: (R.vgg_ref(t, weights(), p, torch.float64), R.vgg_ref(t, weights(), p, torch.float32)) for p in (None, "avg", "max")}


@pytest.mark.parametrize("pooling", [None, "avg", "max"])
@pytest.mark.parametrize("key", ["32", "40x48"])
def test_vgg16_stack(gpu_ctx, key, pooling):
    """Device features against the float64 stack (conv2d_tf / relu of the oracle).  Yardstick: the same stack in fp32 on the CPU deviates from float64 by
    `cpu` = max |f32 - f64| / max |f64|; the device gets 4 x that (MFMA chains and split-K sum in another order than a CPU loop).
    Measured (cpu deviation, device deviation), relative to the largest feature:
        32x32,  N = 3 (all three poolings: the final map is 1x1)   3.78e-07, 4.21e-07
        40x48,  N = 2 (all three poolings agree to the digits shown) 5.31e-07, 4.15e-07
    """
    from ladder_latent_data_distribution_modelling_amd.fid import VGG16Features
    N, hw = STACK_CASES[key]
    x, refs = stack_case(key)
    f64, f32 = refs[pooling]
    feats = VGG16Features(gpu_ctx, weights(), pooling, input_size=hw)
    got = feats.stack(torch.as_tensor(x).cuda()).cpu().numpy()
    D = 512 if pooling else 512 * (hw[0] // 32) * (hw[1] // 32)
    assert got.shape == f64.shape == (N, D) and feats.D == D
    scale = np.abs(f64).max()
    cpu, dev = np.abs(f32 - f64).max() / scale, np.abs(got - f64).max() / scale
    print("stack %s pooling %s: fp32 CPU deviation %.3g, device deviation %.3g (largest feature %.4g, %d of %d features non-zero)"
          % (key, pooling, cpu, dev, scale, np.count_nonzero(f64), f64.size))
    print("routes:", feats.routes(N))
    assert np.count_nonzero(f64) > f64.size // 4                         # the random weights leave the network alive
    assert dev <= 4 * cpu


def test_vgg16_stack_on_the_halo_routes(gpu_ctx):
    """A chunk of 128 images at 64x64 puts nine of the layers on the strict-fp32 halo kernels (the small chunks above run on the general kernel
    throughout).  An image's features do not depend on its chunk, so the first and the last image are compared with the float64 stack of those two
    alone; same yardstick and factor.
    Measured: fp32 CPU deviation 4.78e-07, device deviation 1.52e-06 (3.2 of the factor 4).
    """
    from ladder_latent_data_distribution_modelling_amd.fid import VGG16Features
    N = 128
    x = np.random.default_rng(64).uniform(-1.0, 1.0, (N, 64, 64, 3)).astype(np.float32)
    feats = VGG16Features(gpu_ctx, weights(), None, input_size=64)
    routes = feats.routes(N)
    assert [fn for _, fn, _ in routes].count("ladder_conv3x3_split") == 9 and routes[0][1] == "ladder_conv2d_fwd" and routes[-1][1] == "ladder_conv2d_fwd"
    got = feats.stack(torch.as_tensor(x).cuda()).cpu().numpy()[[0, N - 1]]
    t = torch.as_tensor(x[[0, N - 1]])
    f64, f32 = R.vgg_ref(t, weights(), None, torch.float64), R.vgg_ref(t, weights(), None, torch.float32)
    scale = np.abs(f64).max()
    cpu, dev = np.abs(f32 - f64).max() / scale, np.abs(got - f64).max() / scale
    print("stack on the halo routes: fp32 CPU deviation %.3g, device deviation %.3g" % (cpu, dev))
    assert got.shape == f64.shape == (2, 2048) and dev <= 4 * cpu


def test_vgg16_routes_and_private_store(gpu_ctx):
    """The 13 layers go through Conv2D.route: the general kernel for Cin = 3, the strict-fp32 halo kernels on the wide maps; the frozen weights stay out
    of the model's parameter layout."""
    from ladder_latent_data_distribution_modelling_amd import arch
    from ladder_latent_data_distribution_modelling_amd.fid import VGG16Features
    feats = VGG16Features(gpu_ctx, weights(), "avg", input_size=64)
    routes = feats.routes(256)
    assert len(routes) == 13 and routes[0][1] == "ladder_conv2d_fwd"
    assert sum(fn == "ladder_conv3x3_split" for _, fn, _ in routes) >= 8
    assert feats.ctx is not gpu_ctx and gpu_ctx.pack_banks is not feats.ctx.pack_banks and gpu_ctx.keep_activations is True
    with pytest.raises(ValueError):
        arch.group_of("block1_conv1/kernel")


# ------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def e2e_sets():
    rng = np.random.default_rng(11)
    real = rng.integers(0, 256, (24, 16, 16, 3), dtype=np.uint8)
    gen = rng.uniform(-0.2, 1.3, (31, 16, 16, 3)).astype(np.float32)
    ref = {s: (R.fid_pipeline_ref(real, gen, weights(), "avg", (32, 32), s, torch.float64),
               R.fid_pipeline_ref(real, gen, weights(), "avg", (32, 32), s, torch.float32)) for s in ("generated", "original")}
    return real, gen, ref


def test_compute_fid_score_end_to_end(gpu_ctx, tmp_path, capsys):
    """compute_FID_score on two archives against the float64 pipeline; the bar is 4 x the deviation of the fp32 CPU pipeline from float64.
    Measured (float64 score, fp32 CPU deviation, device deviation at chunk 256 and 7):
        "generated": 8.9186343873, 1.30e-06 (bar 5.18e-06), 1.97e-06, 5.29e-07
    """
    from ladder_latent_data_distribution_modelling_amd.codes import utils
    real, gen, ref = e2e_sets()
    a, b = str(tmp_path / "real.npz"), str(tmp_path / "gen.npz")
    np.savez(a, sampled_images=real)
    np.savez(b, sampled_images=gen)
    f64, f32 = ref["generated"]
    bar = 4 * abs(f32 - f64)
    s256 = utils.compute_FID_score(a, b, "VGG", "avg", weights=weights(), input_size=32)
    out = capsys.readouterr().out
    assert "FID score between {} and {} is:\n{}".format(a, b, s256) in out and isinstance(s256, float)
    s7 = utils.compute_FID_score(a, b, "VGG", "avg", weights=weights(), input_size=32, chunk=7)
    with capsys.disabled():
        print("\ne2e: float64 %.12g, fp32 CPU deviation %.3g (bar %.3g), device deviation chunk 256 %.3g, chunk 7 %.3g"
              % (f64, abs(f32 - f64), bar, abs(s256 - f64), abs(s7 - f64)))
    assert abs(s256 - f64) <= bar and abs(s7 - f64) <= bar and abs(s7 - s256) <= bar
    o64, o32 = ref["original"]
    so = utils.compute_FID_score(a, b, "VGG", "avg", second_set="original", weights=weights(), input_size=32)
    assert abs(so - o64) <= 4 * abs(o32 - o64) and abs(so - s256) > 1e-3 * abs(s256)


# ------------------------------------------------------------------------------------------------ generate(sink=...) and the trainer
@pytest.mark.parametrize("as_uint8", [False, True])
def test_generate_sink_hands_over_the_same_chunks(golden_dir, as_uint8):
    from ladder_latent_data_distribution_modelling_amd.engine import LadderEngine
    d = np.load(os.path.join(golden_dir, "oracle_mnist_digit.npz"))
    cfg = json.loads(str(d["config"]))
    eng = LadderEngine(cfg, "cuda:0", seed=3)
    sampler = eng.prior_sampler("standard_gaussian", seed=9)
    want = eng.generate(70, sampler, chunk=32, as_uint8=as_uint8)
    got, firsts = [], []

    def sink(chunk, first):
        assert chunk.is_cuda and tuple(chunk.shape[1:]) == want.shape[1:]
        got.append(chunk.cpu().numpy())
        firsts.append(first)

    assert eng.generate(70, sampler, chunk=32, as_uint8=as_uint8, sink=sink) is None
    got = np.concatenate(got)
    assert firsts == [0, 32, 64] and got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)) and eng.ctx.keep_activations is True


def test_trainer_compute_fid_keeps_the_images_on_the_device(golden_dir):
    """trainer.compute_FID == fid_from_arrays on the images generate_images returns for the same seed and chunk, within the bar of the end-to-end test
    (4 x the fp32 CPU pipeline's deviation from float64 on these images)."""
    from oracle import ladder_oracle as O
    from ladder_latent_data_distribution_modelling_amd import fid as F
    from ladder_latent_data_distribution_modelling_amd.codes import models as M
    from ladder_latent_data_distribution_modelling_amd.codes.base import BaseTrain_joint
    from ladder_latent_data_distribution_modelling_amd.codes.session import Session
    d = np.load(os.path.join(golden_dir, "oracle_celeba.npz"))
    cfg = json.loads(str(d["config"]))
    cfg.update(checkpoint_dir="/tmp/", result_dir="/tmp/res/", prior="standard_gaussian")
    model = M.CelebAModel_densenet(cfg, device="cuda:0", values=O.init_params(cfg, seed=5))
    tr = BaseTrain_joint(Session(), model, None, cfg)
    tr.cur_epoch = 3
    real = np.random.default_rng(2).integers(0, 256, (12, 128, 128, 3), dtype=np.uint8)
    n = 10
    imgs = tr.generate_images(n, chunk=4, seed=42)
    score = tr.compute_FID(real, n, weights(), pooling="avg", chunk=4, seed=42, input_size=32)
    feats = F.VGG16Features(model.engine.ctx, weights(), "avg", input_size=32)
    want = F.fid_from_arrays(real, imgs, feats, chunk=4)
    f64 = R.fid_pipeline_ref(real, imgs, weights(), "avg", (32, 32), "generated", torch.float64)
    f32 = R.fid_pipeline_ref(real, imgs, weights(), "avg", (32, 32), "generated", torch.float32)
    print("trainer: compute_FID %.12g, fid_from_arrays %.12g, float64 %.12g, fp32 CPU deviation %.3g" % (score, want, f64, abs(f32 - f64)))
    assert abs(score - want) <= 4 * abs(f32 - f64)
    assert model.engine.ctx.keep_activations is True
