"""The kernels of the importance-weighted log-likelihood (csrc/iwll.hip) through the C ABI, each against numpy float64 on the same fp32 inputs.

Row kernels (sample_rows' log q, laplace_rows, gauss_rows) form every difference, square and sum in float64, so the bar is DERIVED, not measured: a sum
of n_terms float64 terms in any order is within n_terms * 2^-52 * sum |terms| of the exact sum, plus 1e-12 relative on the terms a `log` produces (the
device's float64 log is good to a few ulp; numpy's likewise).  `sample` is fp32 fmaf(sd, eps, mu): it must equal the z of ladder_latent_fwd bit for bit.
It was meant to equal torch.addcmul's bits too; measured on an MI355X it does not (addcmul rounds the product before the sum), so that comparison is held
at 1 ulp, as DESIGN.md says.  The diagonal-mixture rows run the fp32 arithmetic of the responsibilities pass of csrc/diag_mixture.hip and
are held to the bar tests/test_gpu_diag_mixture_wide.py::check holds that kernel's sum of log-probs to, per row: |got - ref| < 3e-5 |ref| + 1e-3.
accumulate + finish are compared with the one-shot float64 estimator at 1e-12 RELATIVE (log-weights near -7e4: one float64 ulp there is 1.5e-11, so an
absolute 1e-12 could not be met by any float64 code; relative 1e-12 is 7e-8 absolute there, and four orders above the rounding of an 8-term sum)."""
import math

import numpy as np
import pytest
import torch

import iw_ref

pytestmark = pytest.mark.gpu
E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3
EPS64 = 2.0 ** -52
LOG_REL = 1e-12
DIAG_ROW_RTOL, DIAG_ROW_ATOL = 3e-5, 1e-3          # tests/test_gpu_diag_mixture_wide.py::check, the sum of log-probs
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
SENTINEL = -123.25


def _lib():
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    return L


def dev(a, dtype=np.float32):
    return torch.as_tensor(np.ascontiguousarray(a, dtype)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def f64(n, fill=SENTINEL):
    return torch.full((n,), fill, dtype=torch.float64, device="cuda")


# ------------------------------------------------------------------------------------------------ sample_rows
@pytest.mark.parametrize("per", [1, 3])
@pytest.mark.parametrize("parents", [1, 65, 130])
@pytest.mark.parametrize("W", [2, 40, 256])
def test_sample_rows(gpu_ctx, W, parents, per):
    L, n = _lib(), parents * per
    rng = np.random.default_rng(W + parents + per)
    mu, sd = rng.standard_normal((parents, W)).astype(np.float32), (1e-3 + rng.random((parents, W))).astype(np.float32)
    eps = rng.standard_normal((n, W)).astype(np.float32)
    mud, sdd, epd = dev(mu), dev(sd), dev(eps)
    sample, logq = torch.full((n * W + 8,), SENTINEL, device="cuda"), f64(n + 8)
    L.call("ladder_iw_sample_rows", p(mud), p(sdd), p(epd), n, per, W, p(sample), p(logq), gpu_ctx.stream)
    torch.cuda.synchronize()
    assert (sample[n * W:] == SENTINEL).all() and (logq[n:] == SENTINEL).all()
    # the code sample: bit for bit the z of the training path (ladder_latent_fwd with a zero floor on the std-dev head: sd_raw + 0 = sd) ...
    got = sample[:n * W].reshape(n, W)
    mur, sdr = mud.repeat_interleave(per, 0).contiguous(), sdd.repeat_interleave(per, 0).contiguous()
    z_train, sd_out, scratch = torch.empty(n, W, device="cuda"), torch.empty(n, W, device="cuda"), torch.empty(2, device="cuda")
    L.call("ladder_latent_fwd", p(mur), p(sdr), p(epd), 0.0, p(z_train), p(sd_out), p(scratch), p(scratch[1:]), None, n, W, gpu_ctx.stream)
    assert torch.equal(got, z_train)
    # ... which is ONE rounding of sd * eps + mu.  torch.addcmul rounds the product first (measured on an MI355X: its bits differ), so the two are
    # within 1 ulp of the largest of |mu|, |sd * eps|, |z|: (1/2 ulp(product) + 1/2 ulp(z')) + 1/2 ulp(z), and both results sit on that grid.
    want = torch.addcmul(mur, sdr, epd)
    big = torch.maximum(torch.maximum(mur.abs(), (sdr * epd).abs()), torch.maximum(got.abs(), want.abs())).cpu().numpy()
    ulps = np.abs(got.cpu().numpy().astype(np.float64) - want.cpu().numpy().astype(np.float64)) / np.spacing(big).astype(np.float64)
    print("sample_rows W=%d n=%d per=%d: %d of %d elements differ from torch.addcmul, at most %.2f ulp" % (W, n, per, (ulps > 0).sum(), ulps.size, ulps.max()))
    assert ulps.max() <= 1.0
    e, s = eps.astype(np.float64), np.repeat(sd.astype(np.float64), per, 0)
    ref = -0.5 * (e * e).sum(1) - np.log(s).sum(1) - W * HALF_LOG_2PI
    mag = 0.5 * (e * e).sum(1) + np.abs(np.log(s)).sum(1) + W * HALF_LOG_2PI
    bound = (2 * W + 1) * EPS64 * mag + LOG_REL * np.abs(np.log(s)).sum(1)
    err = np.abs(logq[:n].cpu().numpy() - ref)
    print("sample_rows W=%d n=%d per=%d: max err %.3e, bound there %.3e" % (W, n, per, err.max(), bound[err.argmax()]))
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ laplace_rows
def _laplace(L, st, x, xh, per, sigma, x_off=0):
    """one call on host arrays -> out [n] float64; x may sit `x_off` floats into its allocation (off 16 bytes)"""
    n, D = xh.shape
    xd = torch.zeros(x.size + x_off, device="cuda")
    xd[x_off:] = dev(x).reshape(-1)
    hd = dev(xh)
    out = f64(n + 8)
    nws = L.query("ladder_iw_laplace_rows_workspace_bytes", n, D)
    ws = torch.empty(max(nws, 16), dtype=torch.uint8, device="cuda")
    L.call("ladder_iw_laplace_rows", p(xd) + 4 * x_off, p(hd), n, per, D, float(sigma), p(out), p(ws) if nws else None, nws, st)
    torch.cuda.synchronize()
    assert (out[n:] == SENTINEL).all()
    return out[:n].cpu().numpy(), nws


def _laplace_check(got, x, xh, per, sigma, what):
    D = xh.shape[1]
    a = np.abs(np.repeat(x.astype(np.float64), per, 0) - xh.astype(np.float64)).sum(1)
    ref = -a / sigma - D * math.log(2 * sigma)
    bound = (D + 2) * EPS64 * (a / sigma + D * abs(math.log(2 * sigma))) + LOG_REL * D * abs(math.log(2 * sigma))
    err = np.abs(got - ref)
    print("laplace_rows %s: max err %.3e, bound there %.3e (|ref| %.3e)" % (what, err.max(), bound[err.argmax()], np.abs(ref).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize("per", [1, 3])
@pytest.mark.parametrize("parents", [1, 65, 130])
@pytest.mark.parametrize("D", [7, 784, 49152])
def test_laplace_rows(gpu_ctx, D, parents, per):
    """rows = parents * per: 1 .. 195 take the (row, slice) route where D has more than one slice, 390 the workgroup-per-row route"""
    L, n = _lib(), parents * per
    rng = np.random.default_rng(D + parents + per)
    x, xh = rng.random((parents, D)).astype(np.float32), (rng.random((n, D)) * 1.1 - 0.05).astype(np.float32)
    sigma = 0.0371
    got, nws = _laplace(L, gpu_ctx.stream, x, xh, per, sigma)
    assert (nws > 0) == (n < 256 and D > 1024)
    _laplace_check(got, x, xh, per, sigma, "D=%d n=%d per=%d ws=%d" % (D, n, per, nws))
    again, _ = _laplace(L, gpu_ctx.stream, x, xh, per, sigma)
    assert np.array_equal(got, again)                                       # one fixed order: the same bits


def test_laplace_rows_sliced_route_and_scalar_loads(gpu_ctx):
    L = _lib()
    rng = np.random.default_rng(3)
    x, xh = rng.random((2, 49152)).astype(np.float32), rng.random((2, 49152)).astype(np.float32)
    got, nws = _laplace(L, gpu_ctx.stream, x, xh, 1, 0.5)
    assert nws >= 2 * 48 * 8                                                # 48 slices of 1024 floats per row
    _laplace_check(got, x, xh, 1, 0.5, "sliced n=2 D=49152")
    off, _ = _laplace(L, gpu_ctx.stream, x, xh, 1, 0.5, x_off=1)            # x off 16 bytes: scalar loads, the same bound
    _laplace_check(off, x, xh, 1, 0.5, "sliced, x off 16 bytes")
    x3, xh3 = rng.random((1, 4099)).astype(np.float32), rng.random((2, 4099)).astype(np.float32)     # D % 4 != 0 across slices
    got3, nws3 = _laplace(L, gpu_ctx.stream, x3, xh3, 2, 2.0)
    assert nws3 > 0
    _laplace_check(got3, x3, xh3, 2, 2.0, "sliced n=2 D=4099")


# ------------------------------------------------------------------------------------------------ gauss_rows
@pytest.mark.parametrize("n", [1, 65, 130])
@pytest.mark.parametrize("W", [2, 40, 256])
@pytest.mark.parametrize("with_b,s", [(True, 0.07), (False, 1.0)])
def test_gauss_rows(gpu_ctx, W, n, with_b, s):
    L = _lib()
    rng = np.random.default_rng(W + n)
    a = rng.standard_normal((n, W)).astype(np.float32)
    b = (a + 0.1 * rng.standard_normal((n, W))).astype(np.float32) if with_b else None
    out = f64(n + 8)
    ad, bd = dev(a), (dev(b) if with_b else None)
    L.call("ladder_iw_gauss_rows", p(ad), p(bd), float(s), n, W, p(out), gpu_ctx.stream)
    torch.cuda.synchronize()
    assert (out[n:] == SENTINEL).all()
    d = a.astype(np.float64) - (b.astype(np.float64) if with_b else 0.0)
    q = (d * d).sum(1) / (2 * s * s)
    ref = -q - W * math.log(s) - W * HALF_LOG_2PI
    bound = (W + 3) * EPS64 * (q + W * abs(math.log(s)) + W * HALF_LOG_2PI) + LOG_REL * W * abs(math.log(s))
    err = np.abs(out[:n].cpu().numpy() - ref)
    print("gauss_rows W=%d n=%d s=%g: max err %.3e, bound there %.3e" % (W, n, s, err.max(), bound[err.argmax()]))
    assert (err <= bound).all()


# ------------------------------------------------------------------------------------------------ diagonal mixture rows
@pytest.mark.parametrize("K,Z", [(1, 2), (3, 40), (500, 40), (1024, 256)])
def test_diag_mixture_rows(gpu_ctx, K, Z):
    L, n = _lib(), 37                                                        # not a multiple of the 16 rows of a workgroup
    rng = np.random.default_rng(K + Z)
    base = rng.standard_normal(Z)
    cm = base + 0.3 * rng.standard_normal((K, Z))
    cs = 0.5 + rng.random((K, Z))
    cm[K // 2] += 50.0                                                       # one component far from every point: responsibility 0 everywhere
    z = base + 0.5 * rng.standard_normal((n, Z))
    z, cm, cs = (np.ascontiguousarray(a, np.float32) for a in (z, cm, cs))
    nws = L.query("ladder_diag_mixture_logprob_rows_workspace_bytes", n, Z, K)
    assert nws > 0
    outs = []
    zd, cmd, csd = dev(z), dev(cm), dev(cs)
    for junk in (0, 255):                                                    # the result does not depend on what the workspace held
        ws = torch.full((nws + 4,), junk, dtype=torch.uint8, device="cuda")
        out = torch.full((n + 8,), SENTINEL, device="cuda")
        L.call("ladder_diag_mixture_logprob_rows", p(zd), p(cmd), p(csd), n, Z, K, p(out), p(ws) + 4, nws, gpu_ctx.stream)
        torch.cuda.synchronize()
        assert (out[n:] == SENTINEL).all()
        outs.append(out[:n].cpu().numpy())
    assert np.array_equal(outs[0], outs[1])
    u = (z.astype(np.float64)[:, None, :] - cm.astype(np.float64)) / cs.astype(np.float64)
    lp = -0.5 * (u ** 2).sum(-1) - np.log(cs.astype(np.float64)).sum(-1) - Z * HALF_LOG_2PI - math.log(K)
    ref = torch.logsumexp(torch.as_tensor(lp), -1).numpy()
    if K > 1:
        assert (lp[:, K // 2] - ref < -700).all()                            # ... its weight underflows even in float64
    err = np.abs(outs[0].astype(np.float64) - ref)
    print("diag rows K=%d Z=%d: max err %.3e (|ref| %.3e, bar %.3e)" % (K, Z, err.max(), np.abs(ref).max(), (DIAG_ROW_RTOL * np.abs(ref) + DIAG_ROW_ATOL).min()))
    assert np.isfinite(outs[0]).all() and (err < DIAG_ROW_RTOL * np.abs(ref) + DIAG_ROW_ATOL).all()


# ------------------------------------------------------------------------------------------------ add_term, accumulate, finish
def _stream_estimate(L, st, logw, split, junk_state=False):
    """logw [B, S] host float64, fed chunk by chunk (image-major rows per chunk) -> out [B, 4] host, raw state"""
    B, S = logw.shape
    assert sum(split) == S
    state = torch.zeros(B * 5 + 8, dtype=torch.float64, device="cuda")
    state[B * 5:] = SENTINEL
    if junk_state:                                                           # a row whose count is 0 is empty whatever else it holds
        state[:B * 5].reshape(B, 5)[:, :4] = float("nan")
    out, s0 = f64(B * 4 + 8), 0
    for c in split:
        chunk = dev(logw[:, s0:s0 + c].reshape(-1), np.float64)
        L.call("ladder_iw_accumulate", p(chunk), B, c, p(state), st)
        s0 += c
    L.call("ladder_iw_finish", p(state), B, p(out), st)
    torch.cuda.synchronize()
    assert (state[B * 5:] == SENTINEL).all() and (out[B * 4:] == SENTINEL).all()
    return out[:B * 4].reshape(B, 4).cpu().numpy()


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    same_inf = np.isinf(a) & (a == b)
    with np.errstate(invalid="ignore"):
        return bool(np.all(same_inf | (np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b)))))


def test_accumulate_and_finish(gpu_ctx):
    L, st = _lib(), gpu_ctx.stream
    rng = np.random.default_rng(11)
    B, S = 6, 8
    logw = -70000.0 + 50.0 * rng.standard_normal((B, S))                    # CelebA scale: differences of order 1 .. 100 on 7e4
    logw[1, [0, 3, 7]] = -np.inf                                             # zero weights among live ones
    logw[2, :] = -np.inf                                                     # an image whose weights are all zero
    logw[3, :5] = -np.inf                                                    # the first chunks of a split see nothing but zeros
    ref = iw_ref.finish(logw)
    assert ref[2, 0] == -np.inf and ref[2, 2] == 0.0
    splits = [(8,), (3, 3, 2), (1,) * 8]
    got = [_stream_estimate(L, st, logw, sp) for sp in splits]
    for sp, g in zip(splits, got):
        assert not np.isnan(g).any(), sp
        assert _close(g, ref), (sp, g, ref)                                  # log_px, elbo_1 (-inf where a weight is 0), ess, S against one shot
        assert (g[:, 3] == S).all()
        live = np.isfinite(ref[:, 1])
        assert (g[live, 1] <= g[live, 0] + 1e-9).all()
    assert got[0][2, 0] == -np.inf and got[0][2, 2] == 0.0 and got[0][1, 1] == -np.inf
    assert _close(got[1], got[0]) and _close(got[2], got[0])                 # any chunking
    assert np.array_equal(_stream_estimate(L, st, logw, (3, 3, 2)), got[1])  # the same split twice: the same bits
    assert np.array_equal(_stream_estimate(L, st, logw, (3, 3, 2), junk_state=True), got[1])
    empty = f64(4)
    none = torch.zeros(5, dtype=torch.float64, device="cuda")
    L.call("ladder_iw_finish", p(none), 1, p(empty), st)
    e = empty.cpu().numpy()
    assert np.isnan(e[:3]).all() and e[3] == 0.0                             # no sample: nothing was estimated
    wide = -300.0 * np.arange(130, dtype=np.float64)[None, :] * np.ones((3, 1))          # more rows than a wavefront; most weights underflow
    assert _close(_stream_estimate(L, st, wide, (130,)), iw_ref.finish(wide)) and _close(_stream_estimate(L, st, wide, (64, 1, 65)), iw_ref.finish(wide))


def test_add_term(gpu_ctx):
    L, st, n = _lib(), gpu_ctx.stream, 300
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal(n) * 1e4, rng.standard_normal(n).astype(np.float32)
    logw = f64(n + 8)
    ad, bd = dev(a, np.float64), dev(b)
    L.call("ladder_iw_add_term", p(ad), 0, 1.0, n, 1, p(logw), st)
    L.call("ladder_iw_add_term", p(bd), 1, -1.0, n, 0, p(logw), st)
    torch.cuda.synchronize()
    assert (logw[n:] == SENTINEL).all() and np.array_equal(logw[:n].cpu().numpy(), a - b.astype(np.float64))


def test_randn_rows_do_not_depend_on_the_chunking(gpu_ctx):
    L, st, W = _lib(), gpu_ctx.stream, 10
    full = torch.full((6 * 7 * W + 8,), SENTINEL, device="cuda")
    L.call("ladder_iw_randn_rows", p(full), 6, 7, W, 100, 0, 5, 0, st)
    part = torch.empty(2 * 3 * W, device="cuda")
    L.call("ladder_iw_randn_rows", p(part), 2, 3, W, 103, 2, 5, 0, st)       # images 103, 104; samples 2 .. 4
    other = torch.empty(6 * 7 * W, device="cuda")
    L.call("ladder_iw_randn_rows", p(other), 6, 7, W, 100, 0, 5, 1, st)      # the t level draws other numbers
    torch.cuda.synchronize()
    assert (full[6 * 7 * W:] == SENTINEL).all()
    f = full[:6 * 7 * W].reshape(6, 7, W)
    assert torch.equal(part.reshape(2, 3, W), f[3:5, 2:5]) and not torch.equal(other.reshape(6, 7, W), f)
    v = f.cpu().numpy().astype(np.float64)
    assert np.isfinite(v).all() and abs(v.mean()) < 0.25 and 0.7 < v.std() < 1.3 and len(np.unique(v)) == v.size


# ------------------------------------------------------------------------------------------------ ABI limits
def test_abi_limits(gpu_ctx):
    """Every refusal of the header: LADDER_E_SHAPE for a bad shape or a NULL array, LADDER_E_ALIGN for a float64 array off 8 bytes, LADDER_E_WORKSPACE for a
    NULL or short workspace; a refused call launches nothing (the sentinel-filled outputs stay as they were)."""
    L, st = _lib(), gpu_ctx.stream
    q = L.query
    f = torch.zeros(1 << 16, device="cuda")
    outs32, outs64 = torch.full((4096,), SENTINEL, device="cuda"), f64(4096)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    F, O32, O64, W = p(f), p(outs32), p(outs64), p(ws)
    calls = []
    # sample_rows(mu, sd, eps, n, per, W, sample, logq)
    ok = [F, F, F, 6, 3, 8, O32, O64, st]
    for i in (0, 1, 2, 6, 7):
        calls.append(("ladder_iw_sample_rows", ok[:i] + [None] + ok[i + 1:], E_SHAPE))
    for i, v in ((3, 0), (3, -1), (3, 7), (4, 0), (5, 0), (5, 65537)):
        calls.append(("ladder_iw_sample_rows", ok[:i] + [v] + ok[i + 1:], E_SHAPE))
    calls.append(("ladder_iw_sample_rows", ok[:7] + [O64 + 4] + ok[8:], E_ALIGN))
    # laplace_rows(x, xhat, n, per, D, sigma, out, ws, ws_bytes)
    ok = [F, F, 2, 1, 4096, 0.5, O64, W, 1 << 20, st]
    need = q("ladder_iw_laplace_rows_workspace_bytes", 2, 4096)
    assert need > 0 and q("ladder_iw_laplace_rows_workspace_bytes", 256, 4096) == 0 and q("ladder_iw_laplace_rows_workspace_bytes", 0, 4096) == 0
    assert q("ladder_iw_laplace_rows_workspace_bytes", 2, 0) == 0 and q("ladder_iw_laplace_rows_workspace_bytes", 2, (1 << 22) + 1) == 0
    for i in (0, 1, 6):
        calls.append(("ladder_iw_laplace_rows", ok[:i] + [None] + ok[i + 1:], E_SHAPE))
    for i, v in ((2, 0), (3, 0), (3, 3), (4, 0), (4, (1 << 22) + 1), (5, 0.0), (5, -1.0), (5, float("nan")), (5, float("inf"))):
        calls.append(("ladder_iw_laplace_rows", ok[:i] + [v] + ok[i + 1:], E_SHAPE))
    calls.append(("ladder_iw_laplace_rows", ok[:6] + [O64 + 4] + ok[7:], E_ALIGN))
    calls.append(("ladder_iw_laplace_rows", ok[:7] + [None, 1 << 20, st], E_WORKSPACE))
    calls.append(("ladder_iw_laplace_rows", ok[:7] + [W, need - 1, st], E_WORKSPACE))
    # gauss_rows(a, b, s, n, W, out)
    ok = [F, F, 1.0, 5, 8, O64, st]
    for i in (0, 5):
        calls.append(("ladder_iw_gauss_rows", ok[:i] + [None] + ok[i + 1:], E_SHAPE))
    for i, v in ((2, 0.0), (2, -2.0), (2, float("nan")), (3, 0), (4, 0), (4, 65537)):
        calls.append(("ladder_iw_gauss_rows", ok[:i] + [v] + ok[i + 1:], E_SHAPE))
    calls.append(("ladder_iw_gauss_rows", ok[:5] + [O64 + 4, st], E_ALIGN))
    # diag_mixture_logprob_rows(z, comp_mean, comp_sd, n, Z, K, logp, ws, ws_bytes)
    ok = [F, F, F, 5, 40, 7, O32, W, 1 << 20, st]
    need = q("ladder_diag_mixture_logprob_rows_workspace_bytes", 5, 40, 7)
    assert need > 0 and all(q("ladder_diag_mixture_logprob_rows_workspace_bytes", *bad) == 0 for bad in ((0, 40, 7), (5, 0, 7), (5, 257, 7), (5, 40, 0), (5, 40, 1025)))
    for i in (0, 1, 2, 6):
        calls.append(("ladder_diag_mixture_logprob_rows", ok[:i] + [None] + ok[i + 1:], E_SHAPE))
    for i, v in ((3, 0), (4, 0), (4, 257), (5, 0), (5, 1025)):
        calls.append(("ladder_diag_mixture_logprob_rows", ok[:i] + [v] + ok[i + 1:], E_SHAPE))
    calls.append(("ladder_diag_mixture_logprob_rows", ok[:7] + [None, 1 << 20, st], E_WORKSPACE))
    calls.append(("ladder_diag_mixture_logprob_rows", ok[:7] + [W, need - 1, st], E_WORKSPACE))
    # add_term(term, term_is_f32, sign, n, init, logw)
    ok = [F, 1, 1.0, 5, 1, O64, st]
    calls += [("ladder_iw_add_term", [None] + ok[1:], E_SHAPE), ("ladder_iw_add_term", ok[:5] + [None, st], E_SHAPE),
              ("ladder_iw_add_term", ok[:3] + [0] + ok[4:], E_SHAPE), ("ladder_iw_add_term", ok[:5] + [O64 + 4, st], E_ALIGN),
              ("ladder_iw_add_term", [F + 4, 0] + ok[2:], E_ALIGN)]
    # accumulate(logw, B, C, state), finish(state, B, out)
    calls += [("ladder_iw_accumulate", [None, 2, 3, O64, st], E_SHAPE), ("ladder_iw_accumulate", [F, 2, 3, None, st], E_SHAPE),
              ("ladder_iw_accumulate", [F, 0, 3, O64, st], E_SHAPE), ("ladder_iw_accumulate", [F, 2, 0, O64, st], E_SHAPE),
              ("ladder_iw_accumulate", [F, 1 << 13, 1 << 12, O64, st], E_SHAPE), ("ladder_iw_accumulate", [F + 4, 2, 3, O64, st], E_ALIGN),
              ("ladder_iw_accumulate", [F, 2, 3, O64 + 4, st], E_ALIGN),
              ("ladder_iw_finish", [None, 2, O64, st], E_SHAPE), ("ladder_iw_finish", [F, 2, None, st], E_SHAPE), ("ladder_iw_finish", [F, 0, O64, st], E_SHAPE),
              ("ladder_iw_finish", [F, 2, O64 + 4, st], E_ALIGN)]
    # randn_rows(out, B, C, W, image0, sample0, seed, level)
    ok = [O32, 2, 3, 8, 0, 0, 1, 0, st]
    calls.append(("ladder_iw_randn_rows", [None] + ok[1:], E_SHAPE))
    for i, v in ((1, 0), (2, 0), (3, 0), (3, 65537), (7, -1), (7, 16)):
        calls.append(("ladder_iw_randn_rows", ok[:i] + [v] + ok[i + 1:], E_SHAPE))
    for name, args, want in calls:
        assert q(name, *args) == want, (name, args, want)
    torch.cuda.synchronize()
    assert (outs32 == SENTINEL).all() and (outs64 == SENTINEL).all(), "a refused call wrote to its outputs"
