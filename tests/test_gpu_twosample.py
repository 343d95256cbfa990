"""Two-sample metrics on the device (csrc/twosample.hip, ladder_latent_data_distribution_modelling_amd/two_sample.py) against the float64 numpy
reference of twosample_ref.py: k-NN radii, ball counts and polynomial-kernel sums (exact on dyadic data, inside written-out rounding bounds on normal
data), the refusals, the Python owners, metrics_from_arrays / the command line end to end, and the trainer's compute_sample_metrics / latent_match."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fid_ref as FR  # noqa: E402
import twosample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53
SENT, ISENT = -7.0e33, -77777
E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3
DIMS = [1, 3, 4, 17, 80, 512]                      # D < 4, D % 4 != 0, more than one 32-column chunk
ROWS = [2, 4, 5, 9, 63, 64, 65, 130, 257]          # k + 1 for k = 1, 3, 8; around the 64-row tile; 3 and 5 column splits
KS = [1, 3, 8]


def _L():
    from ladder_latent_data_distribution_modelling_amd import _lib
    _lib.load()
    return _lib


def _st():
    return torch.cuda.current_stream().cuda_stream


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _guarded(n, dtype=torch.float64, pad=64):
    sent = ISENT if dtype == torch.int32 else SENT
    buf = torch.full((n + pad,), sent, dtype=dtype, device="cuda")
    return buf, buf[:n], sent


def _intact(buf, n, sent):
    return bool((buf[n:] == sent).all().item())


def _ptr(t):
    return 0 if t is None else t.data_ptr()


def run_norms(x, shift):
    L = _L()
    n, D = x.shape
    buf, out, sent = _guarded(n)
    xd = dev(x)                                                     # (held until the synchronisation below)
    L.call("ladder_pairs_row_norms", xd.data_ptr(), n, D, _ptr(shift), out.data_ptr(), _st())
    torch.cuda.synchronize()
    assert _intact(buf, n, sent)
    return out


def run_radii(a, shift, k, norms=None):
    """-> r2 [n] float64 numpy; the inputs hold exactly n * D floats, output and workspace sit in front of sentinels."""
    L = _L()
    n, D = a.shape
    ad = dev(a)
    norms = run_norms(a, shift) if norms is None else norms
    nb = L.query("ladder_pairs_workspace_bytes", n, n, D, k, 0)
    assert nb > 0 and nb % 8 == 0
    wbuf, ws, wsent = _guarded(nb // 8)
    buf, r2, sent = _guarded(n)
    L.call("ladder_pairs_knn_radii", ad.data_ptr(), norms.data_ptr(), n, D, _ptr(shift), k, r2.data_ptr(), ws.data_ptr(), nb, _st())
    torch.cuda.synchronize()
    assert _intact(buf, n, sent) and _intact(wbuf, nb // 8, wsent)
    return r2.cpu().numpy()


def run_counts(q, a, r2, shift):
    L = _L()
    (m, D), n = q.shape, a.shape[0]
    qd, ad = dev(q), dev(a)
    nq, na = run_norms(q, shift), run_norms(a, shift)
    nb = L.query("ladder_pairs_workspace_bytes", m, n, D, 0, 0)
    assert nb > 0 and nb % 4 == 0
    wbuf, ws, wsent = _guarded(nb // 4, torch.int32)
    buf, counts, sent = _guarded(m, torch.int32)
    rd = dev(np.asarray(r2, np.float64))
    L.call("ladder_pairs_ball_counts", qd.data_ptr(), nq.data_ptr(), m, ad.data_ptr(), na.data_ptr(), rd.data_ptr(), n, D,
           _ptr(shift), counts.data_ptr(), ws.data_ptr(), nb, _st())
    torch.cuda.synchronize()
    assert _intact(buf, m, sent) and _intact(wbuf, nb // 4, wsent)
    return counts.cpu().numpy()


def run_poly(x, sx, y, sy, nb, degree, gamma, coef0):
    L = _L()
    D = x.shape[1]
    assert x.shape[0] == nb * sx and y.shape[0] == nb * sy
    nbytes = L.query("ladder_pairs_workspace_bytes", sx, sy, D, 0, nb)
    assert nbytes > 0 and nbytes % 8 == 0
    wbuf, ws, wsent = _guarded(nbytes // 8)
    buf, sums, sent = _guarded(3 * nb)
    xd, yd = dev(x), dev(y)
    L.call("ladder_pairs_poly_sums", xd.data_ptr(), sx, yd.data_ptr(), sy, nb, D, degree, float(gamma), float(coef0), sums.data_ptr(), ws.data_ptr(),
           nbytes, _st())
    torch.cuda.synchronize()
    assert _intact(buf, 3 * nb, sent) and _intact(wbuf, nbytes // 8, wsent)
    return sums.cpu().numpy().reshape(nb, 3)


# ------------------------------------------------------------------------------------------------ 1. exact on dyadic data
def dyadic_set(D, n, seed):
    """Integer-valued fp32 rows in [-8, 8] whose last row repeats the first, and an integer shift in [-2, 2].  Bit budget: |x - c| <= 10 < 2^4, a
    product < 2^7, a norm or a dot product over D <= 512 terms < 2^16, d = n_i + n_j - 2 G < 2^18, all integers: every product, every partial sum in
    any order and the final combination are exact in float64's 53 bits, so the device must give the reference's bits."""
    rng = np.random.default_rng(seed)
    a = rng.integers(-8, 9, (n, D)).astype(np.float32)
    a[n - 1] = a[0]
    return a, rng.integers(-2, 3, D).astype(np.float32)


@pytest.mark.parametrize("D,n", [(D, n) for D in DIMS for n in ROWS] + [(4, 2112)])
def test_radii_and_counts_exact_on_dyadic_data(gpu_ctx, D, n):
    """n = 2112 (33 row tiles, 11 splits of 3 column tiles) makes a workgroup walk more than one tile between two epilogues."""
    a, shift = dyadic_set(D, n, 1000 * D + n)
    m = max(2, (2 * n) // 3 + 1) if n < 2112 else 70
    rng = np.random.default_rng(n + D)
    q = np.concatenate([a[:m // 2], rng.integers(-8, 9, (m - m // 2, D)).astype(np.float32)])      # half of the queries ARE reference rows
    daa, dqa = R.sqdist(a, a), R.sqdist(q, a)
    sd = dev(shift)
    norms = run_norms(a, sd)
    assert np.array_equal(norms.cpu().numpy(), ((a.astype(np.float64) - shift) ** 2).sum(1))
    for k in [k for k in KS if k <= n - 1]:
        want = R.knn_radii(a, k, daa)
        got = run_radii(a, sd, k, norms)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (D, n, k)
        if k == 1:
            assert got[0] == 0.0 and got[n - 1] == 0.0                                            # duplicate rows: self goes by index, the twin stays
        # q = a: row j's k-th neighbour i sits exactly ON ball j (d_ij == r2_j): the non-strict test must count it, and every row counts itself
        ties = (daa == want[None, :]) & ~np.eye(n, dtype=bool)
        assert ties.any(1).sum() >= 1 and ties.any(0).all()
        self_counts = run_counts(a, a, got, sd)
        assert np.array_equal(self_counts, R.ball_counts(a, a, want, daa)) and self_counts.min() >= 1
        assert np.array_equal(run_counts(q, a, got, sd), R.ball_counts(q, a, want, dqa))
    assert np.array_equal(run_radii(a, None, 1), R.knn_radii(a, 1, daa))                           # no shift at all: still exact


# ------------------------------------------------------------------------------------------------ 2. radii on normal data with an offset of 50
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("D", DIMS)
def test_radii_normal_data_with_offset(gpu_ctx, D, n):
    """|r2_i - ref_i| <= max_{j != i} (E_ij + the reference's own rounding): the k-th smallest of perturbed values moves by at most the largest
    perturbation.  E_ij = (D + 3) 2^-53 (norms_i + norms_j + 2 sum_k |a~_ik| |a~_jk|) about the fp32 column mean (twosample_ref.distance_error_bound
    derives it); the reference forms d from the differences themselves and carries (D + 2) 2^-53 d_ij."""
    a = (50.0 + np.random.default_rng(7 * D + n).standard_normal((n, D))).astype(np.float32)
    shift = a.astype(np.float64).mean(0).astype(np.float32)
    daa = R.sqdist(a, a)
    tol = R.distance_error_bound(a, a, shift.astype(np.float64)) + R.reference_distance_error(daa, D)
    tol = np.where(np.eye(n, dtype=bool), 0.0, tol).max(1)
    sd = dev(shift)
    norms = run_norms(a, sd)
    nref = ((a.astype(np.float64) - shift.astype(np.float64)) ** 2).sum(1)
    assert (np.abs(norms.cpu().numpy() - nref) <= 2 * (D + 1) * U64 * nref).all()                  # D squares, D - 1 additions, either side
    for k in [k for k in KS if k <= n - 1]:
        got, want = run_radii(a, sd, k, norms), R.knn_radii(a, k, daa)
        again = run_radii(a, sd, k, norms)
        err = np.abs(got - want)
        print("D %d n %d k %d: max err / bound %.3g, max rel err %.3g" % (D, n, k, (err / tol).max(), (err / want).max()))
        assert np.array_equal(got.view(np.uint64), again.view(np.uint64))                          # same call, same bits
        assert (err <= tol).all()


# ------------------------------------------------------------------------------------------------ 3. counts on normal data
COUNT_PAIRS = [(5, 9), (63, 65), (64, 64), (65, 130), (130, 63), (257, 257), (5, 257), (257, 5)]    # (queries, balls)
COUNT_SEED = 0
# Seeds were tried on the CPU with the reference alone (twosample_ref.counts_case / counts_case_margins), first seed first: seed 0 meets the input
# condition for every (D, pair, k) below.  Nearest gaps min |d_ij - r2_j| / E_ij of seed 0, smallest k listed: D 1: 8.81e7 (257 x 257, k 1);
# D 3: 2.27e9 (257 x 257, k 3); D 4: 5.68e9 (257 x 257, k 8); D 17: 3.09e8 (130 x 63, k 1); D 80: 6.20e8 (65 x 130, k 8); D 512: 1.74e8 (65 x 130, k 3);
# the condition asks for 16.  Reference precision of seed 0 lies between 0.328 and 0.529 throughout.


@pytest.mark.parametrize("pair", COUNT_PAIRS)
@pytest.mark.parametrize("D", DIMS)
def test_counts_normal_data(gpu_ctx, D, pair):
    """Flags compared exactly, for EVERY pair, under a condition on the inputs that is asserted on the reference alone: |d_ij - r2_j| >= 16 E_ij for
    all i, j (E_ij: the device bound of test 2 plus the reference's rounding of d_ij and of r2_j).  With the reference's radii fed to the device only
    d_ij carries device error, at most E_ij; with the device's own radii r2_j moves by at most max_l E_jl as well, and the inputs are asserted to
    leave room for that too (gap_with_radius > 1)."""
    m, n = pair
    q, a, shift = R.counts_case(D, m, n, COUNT_SEED)
    sd = dev(shift.astype(np.float32))
    for k in [k for k in KS if k <= n - 1]:
        r2, want, precision, gap, gap_r = R.counts_case_margins(q, a, shift, k)
        print("D %d %d x %d k %d: reference precision %.3f, nearest gap %.3g E (with the radius' own error %.3g)" % (D, m, n, k, precision, gap, gap_r))
        assert gap >= 16.0 and gap_r > 1.0 and 0.2 < precision < 0.8
        assert np.array_equal(run_counts(q, a, r2, sd), want)
        assert np.array_equal(run_counts(q, a, run_radii(a, sd, k), sd), want)


# ------------------------------------------------------------------------------------------------ 4. polynomial sums
POLY_SHAPES = [(5, 9), (64, 65), (130, 63), (257, 64)]                                            # sx != sy; one tile, a tile edge, 3 and 5 row tiles


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("sx,sy", POLY_SHAPES)
def test_poly_sums_exact_on_dyadic_data(gpu_ctx, sx, sy, degree):
    """Values in {-2 .. 2}, D = 64, gamma = 1 / 64, coef0 = 1.  Bit budget: a dot product is an integer of magnitude <= 256, t = dot / 64 + 1 a multiple of
    2^-6 with |t| <= 5, t^degree a multiple of 2^-24 below 2^10 (34 bits at degree 4), and a sum of at most 257^2 < 2^17 of them needs 51 bits: nothing
    rounds in any order.  Three blocks in one launch equal the three launched alone, bit for bit."""
    nb, D = 3, 64
    rng = np.random.default_rng(sx * 100 + sy + degree)
    x, y = rng.integers(-2, 3, (nb * sx, D)).astype(np.float32), rng.integers(-2, 3, (nb * sy, D)).astype(np.float32)
    got = run_poly(x, sx, y, sy, nb, degree, 1.0 / 64, 1.0)
    for b in range(nb):
        xb, yb = x[b * sx:(b + 1) * sx], y[b * sy:(b + 1) * sy]
        want = R.poly_sums(xb, yb, degree, 1.0 / 64, 1.0)
        assert np.array_equal(got[b].view(np.uint64), want.view(np.uint64)), (b, got[b], want)
        assert np.array_equal(run_poly(xb, sx, yb, sy, 1, degree, 1.0 / 64, 1.0)[0].view(np.uint64), got[b].view(np.uint64))


@pytest.mark.parametrize("degree", [1, 2, 3, 4])
@pytest.mark.parametrize("D", [3, 17, 80, 512])
def test_poly_sums_normal_data(gpu_ctx, D, degree):
    """|S_device - S_reference| <= the bound of twosample_ref.poly_sum_bounds: |d dot_ij| <= D 2^-53 sum_k |x_ik| |y_jk| on either side, carried through
    kappa' = degree t^(degree - 1) gamma, plus (degree + 1) roundings of kappa itself on either side, plus the summation term
    (16 column tiles + 9 + row tiles + 64) 2^-53 sum |kappa|.  Blocks are independent of their launch, and a repeated call gives the same bits."""
    nb, sx, sy = 3, 130, 70
    rng = np.random.default_rng(D + degree)
    x, y = rng.standard_normal((nb * sx, D)).astype(np.float32), (0.5 + rng.standard_normal((nb * sy, D))).astype(np.float32)
    gamma, coef0 = 1.0 / D, 1.0
    got, again = run_poly(x, sx, y, sy, nb, degree, gamma, coef0), run_poly(x, sx, y, sy, nb, degree, gamma, coef0)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64))
    for b in range(nb):
        xb, yb = x[b * sx:(b + 1) * sx], y[b * sy:(b + 1) * sy]
        want, tol = R.poly_sums(xb, yb, degree, gamma, coef0), R.poly_sum_bounds(xb, yb, degree, gamma, coef0)
        err = np.abs(got[b] - want)
        print("D %d degree %d block %d: err / bound %s, rel err %s" % (D, degree, b, err / tol, err / np.abs(want)))
        assert (err <= tol).all()
        alone = run_poly(xb, sx, yb, sy, 1, degree, gamma, coef0)[0]
        assert np.array_equal(alone.view(np.uint64), got[b].view(np.uint64))


# ------------------------------------------------------------------------------------------------ 5. refusals and the workspace query
def test_refusals_leave_the_outputs_alone(gpu_ctx):
    L = _L()
    q, st = L.query, _st()
    x = torch.zeros(16 * 8, device="cuda")
    nrm = torch.zeros(64, dtype=torch.float64, device="cuda")
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    buf, out, sent = _guarded(64)
    ibuf, iout, isent = _guarded(64, torch.int32)
    big = (1 << 24) + 1

    def norms(n, D):
        return q("ladder_pairs_row_norms", x.data_ptr(), n, D, None, out.data_ptr(), st)

    def radii(n, D, k, nbytes=ws.numel()):
        return q("ladder_pairs_knn_radii", x.data_ptr(), nrm.data_ptr(), n, D, None, k, out.data_ptr(), ws.data_ptr(), nbytes, st)

    def counts(m, n, D, nbytes=ws.numel()):
        return q("ladder_pairs_ball_counts", x.data_ptr(), nrm.data_ptr(), m, x.data_ptr(), nrm.data_ptr(), nrm.data_ptr(), n, D, None, iout.data_ptr(),
                 ws.data_ptr(), nbytes, st)

    def poly(sx, sy, nb, D, degree, nbytes=ws.numel()):
        return q("ladder_pairs_poly_sums", x.data_ptr(), sx, x.data_ptr(), sy, nb, D, degree, 0.5, 1.0, out.data_ptr(), ws.data_ptr(), nbytes, st)

    for n, D in ((0, 8), (-1, 8), (big, 8), (16, 0), (16, 32769)):
        assert norms(n, D) == E_SHAPE
    for n, D, k in ((0, 8, 1), (big, 8, 1), (16, 0, 1), (16, 32769, 1), (16, 8, 0), (16, 8, 9), (8, 8, 8), (1, 8, 1)):          # k <= 8 and k <= n - 1
        assert radii(n, D, k) == E_SHAPE
    for m, n, D in ((0, 16, 8), (16, 0, 8), (big, 16, 8), (16, big, 8), (16, 16, 0), (16, 16, 32769)):
        assert counts(m, n, D) == E_SHAPE
    for sx, sy, nb, D, deg in ((0, 4, 2, 8, 3), (4, 0, 2, 8, 3), (4, 4, 0, 8, 3), (4, 4, 65536, 8, 3), (4, 4, 2, 0, 3), (4, 4, 2, 32769, 3), (4, 4, 2, 8, 0),
                               (4, 4, 2, 8, 5), (1 << 23, 4, 3, 8, 3), (4, 1 << 23, 3, 8, 3)):                                    # blocks x rows <= 2^24
        assert poly(sx, sy, nb, D, deg) == E_SHAPE
    assert q("ladder_pairs_knn_radii", None, nrm.data_ptr(), 16, 8, None, 1, out.data_ptr(), ws.data_ptr(), ws.numel(), st) == E_SHAPE
    assert q("ladder_pairs_knn_radii", x.data_ptr(), nrm.data_ptr() + 4, 16, 8, None, 1, out.data_ptr(), ws.data_ptr(), ws.numel(), st) == E_ALIGN
    # a workspace one byte short of the query's answer
    assert radii(16, 8, 3, q("ladder_pairs_workspace_bytes", 16, 16, 8, 3, 0) - 1) == E_WORKSPACE
    assert counts(16, 16, 8, q("ladder_pairs_workspace_bytes", 16, 16, 8, 0, 0) - 1) == E_WORKSPACE
    assert poly(4, 4, 2, 8, 3, q("ladder_pairs_workspace_bytes", 4, 4, 8, 0, 2) - 1) == E_WORKSPACE
    assert q("ladder_pairs_knn_radii", x.data_ptr(), nrm.data_ptr(), 16, 8, None, 3, out.data_ptr(), None, 1 << 16, st) == E_WORKSPACE
    torch.cuda.synchronize()
    assert bool((buf == sent).all().item()) and bool((ibuf == isent).all().item())                   # nothing was launched
    # the same calls inside the limits run
    assert norms(16, 8) == 0 and radii(16, 8, 3) == 0 and counts(16, 16, 8) == 0 and poly(4, 4, 2, 8, 3) == 0
    torch.cuda.synchronize()
    assert _intact(buf, 16, sent) and _intact(ibuf, 16, isent)


def test_workspace_query(gpu_ctx):
    wb = functools.partial(_L().query, "ladder_pairs_workspace_bytes")
    assert wb(257, 257, 512, 3, 0) == 5 * 3 * 320 * 8                                                # 5 splits x k x 5 padded row tiles of doubles
    assert wb(130, 257, 17, 0, 0) == 5 * 192 * 4 and wb(130, 63, 17, 0, 3) == 3 * (2 * 3 + 1) * 8
    assert wb(2112, 2112, 4, 3, 0) == 11 * 3 * 2112 * 8                                              # 15 splits would leave 3 tiles each: 11 do
    for args in ((0, 0, 8, 1, 0), (16, 16, 0, 1, 0), (16, 16, 32769, 1, 0), (16, 16, 8, 9, 0), (16, 16, 8, 16, 0), (16, 17, 8, 1, 0), (16, 16, 8, -1, 0),
                 ((1 << 24) + 1, 16, 8, 0, 0), (16, 16, 8, 1, 2), (16, 16, 8, 0, -1), (16, 16, 8, 0, 65536), (1 << 23, 4, 8, 0, 3)):
        assert wb(*args) == 0, args


# ------------------------------------------------------------------------------------------------ 6. the Python owners
def test_precision_recall_owner(gpu_ctx):
    """precision_recall on device tensors == the reference on the same rows; the shift is the device's own fp32 column mean, copied back for the input
    condition (both directions, as in test 3)."""
    from ladder_latent_data_distribution_modelling_amd import two_sample as T
    k = 3
    gen, real, _ = R.counts_case(17, 130, 63, COUNT_SEED)
    rd, gd = dev(real), dev(gen)
    shift = rd.mean(0).cpu().numpy().astype(np.float64)
    for qq, aa in ((gen, real), (real, gen)):
        _, _, _, gap, gap_r = R.counts_case_margins(qq, aa, shift, k)
        assert gap >= 16.0 and gap_r > 1.0
    got, want = T.precision_recall(rd, gd, k=k), R.precision_recall(real, gen, k)
    print("precision %.4f recall %.4f density %.4f" % (got["precision"], got["recall"], got["density"]))
    assert np.array_equal(got["counts_gen"], want["counts_gen"]) and np.array_equal(got["counts_real"], want["counts_real"])
    assert got["counts_gen"].dtype == np.int32 and got["counts_gen"].shape == (130,) and got["counts_real"].shape == (63,)
    for key in ("precision", "recall", "density"):
        assert got[key] == want[key] and isinstance(got[key], float)
    assert 0.2 < got["precision"] < 0.8


def test_kid_owner_and_feature_bank(gpu_ctx):
    from ladder_latent_data_distribution_modelling_amd import two_sample as T
    D, nsub, s = 80, 5, 64
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal((200, D)).astype(np.float32), (0.3 + rng.standard_normal((150, D))).astype(np.float32)
    xd, yd = dev(x), dev(y)
    mean, std, per = T.kid(xd, yd, n_subsets=nsub, subset_size=s, seed=4)
    wmean, wstd, wper = R.kid(x, y, nsub, s, 4)
    ix, iy = R.subset_plan(200, 150, nsub, s, 4)
    # per subset: the three sums inside poly_sum_bounds, divided as the estimator divides them, plus its own four roundings
    for b in range(nsub):
        bxx, byy, bxy = R.poly_sum_bounds(x[ix[b]], y[iy[b]], 3, 1.0 / D, 1.0)
        sxx, syy, sxy = R.poly_sums(x[ix[b]], y[iy[b]], 3, 1.0 / D, 1.0)
        tol = (bxx + byy) / (s * (s - 1)) + 2 * bxy / (s * s) + 8 * U64 * ((abs(sxx) + abs(syy)) / (s * (s - 1)) + 2 * abs(sxy) / (s * s))
        print("subset %d: MMD^2 %.6g, err %.3g, bound %.3g" % (b, per[b], abs(per[b] - wper[b]), tol))
        assert abs(per[b] - wper[b]) <= tol
    assert per.shape == (nsub,) and mean == float(per.mean()) and std == float(per.std()) and abs(mean - wmean) <= 1e-9 * abs(wmean) + 1e-12
    assert mean > 3 * std / np.sqrt(nsub)                                                           # the sets differ: the offset of 0.3 shows
    # a bank grown over uneven chunks is the concatenation, and KID does not see the chunking
    banks = []
    for chunks in ([3, 1, 70, 5, 121], [200], [64, 64, 72]):
        bank, lo = T.FeatureBank(gpu_ctx, D, capacity=4), 0
        for c in chunks:
            bank.add(xd[lo:lo + c])
            lo += c
        assert bank.n == 200 and tuple(bank.rows.shape) == (200, D) and torch.equal(bank.rows, xd)
        banks.append(bank)
        per_b = T.kid(bank, yd, n_subsets=nsub, subset_size=s, seed=4)[2]
        assert np.array_equal(per_b.view(np.uint64), per.view(np.uint64))
    with pytest.raises(ValueError, match="fp32"):
        banks[0].add(xd[:2, :5])
    assert tuple(T.FeatureBank(gpu_ctx, D).rows.shape) == (0, D)


# ------------------------------------------------------------------------------------------------ 7. end to end
@functools.lru_cache(maxsize=None)
def weights():
    return FR.random_weights(0)


@functools.lru_cache(maxsize=None)
def e2e_sets():
    """24 uint8 and 31 float images of 16 x 16 and their features through the float64 and the fp32 CPU pipeline (computed once, never modified).  The
    first 15 generated images are real ones (x / 255) under noise of 0.05, the rest uniform noise: generated rows fall inside and outside the real
    balls (the fp32 CPU pipeline gives precision 0.48, recall 0.96), so the exact comparison of the counts sees both outcomes."""
    rng = np.random.default_rng(11)
    real = rng.integers(0, 256, (24, 16, 16, 3), dtype=np.uint8)
    gen = rng.uniform(-0.2, 1.3, (31, 16, 16, 3))
    gen[:15] = real[rng.integers(0, 24, 15)] / 255.0 + 0.05 * np.random.default_rng(1).standard_normal((15, 16, 16, 3))
    gen = gen.astype(np.float32)
    feats = {dt: (FR.vgg_ref(FR.preprocess_ref(real, "original", 32, 32, dt), weights(), "avg", dt),
                  FR.vgg_ref(FR.preprocess_ref(gen, "generated", 32, 32, dt), weights(), "avg", dt)) for dt in (torch.float64, torch.float32)}
    return real, gen, feats


KID_ARGS = dict(n_subsets=10, subset_size=1000, seed=2)


def test_metrics_from_arrays_end_to_end(gpu_ctx, tmp_path):
    """FID: fid_from_arrays' bits.  Precision / recall: the reference applied to the device's own features, flags compared exactly under the input
    condition of test 3.  KID: the bar is 4 x the distance of the fp32 CPU pipeline from the float64 pipeline, the convention of the FID tests.
    Measured: KID mean over 10 subsets of 24 in the float64 pipeline 0.0228103919656, fp32 CPU deviation 8.08e-09 (bar 3.23e-08), device deviation
    1.28e-08; precision 0.4839, recall 0.7917, density 0.6452; nearest gaps 1.42e+10 E and 4.98e+09 E."""
    from ladder_latent_data_distribution_modelling_amd import fid as F
    real, gen, feats = e2e_sets()
    features = F.VGG16Features(gpu_ctx, weights(), "avg", input_size=32)
    out = F.metrics_from_arrays(real, gen, features, metrics=("fid", "kid", "pr"), k=3, **KID_ARGS)
    assert out["fid"] == F.fid_from_arrays(real, gen, features) and set(F.metrics_from_arrays(real, gen, features)) == {"fid"}
    # precision / recall on the device's own features
    fr, fg = features(real, "original").cpu().numpy(), features(gen, "generated").cpu().numpy()
    shift = torch.as_tensor(fr).cuda().mean(0).cpu().numpy().astype(np.float64)
    for qq, aa in ((fg, fr), (fr, fg)):
        _, _, _, gap, gap_r = R.counts_case_margins(qq, aa, shift, 3)
        print("e2e: nearest gap %.3g E (with the radius' own error %.3g)" % (gap, gap_r))
        assert gap >= 16.0 and gap_r > 1.0
    want = R.precision_recall(fr, fg, 3)
    assert 0.0 < want["precision"] < 1.0 and 0.0 < want["recall"] < 1.0                           # both outcomes occur, in both directions
    assert np.array_equal(out["counts_gen"], want["counts_gen"]) and np.array_equal(out["counts_real"], want["counts_real"])
    assert (out["precision"], out["recall"], out["density"]) == (want["precision"], want["recall"], want["density"])
    # KID against the float64 pipeline
    k64 = R.kid(*feats[torch.float64], KID_ARGS["n_subsets"], KID_ARGS["subset_size"], KID_ARGS["seed"])[0]
    k32 = R.kid(*feats[torch.float32], KID_ARGS["n_subsets"], KID_ARGS["subset_size"], KID_ARGS["seed"])[0]
    d = abs(k32 - k64)
    print("e2e KID: float64 %.12g, fp32 CPU deviation %.3g (bar %.3g), device deviation %.3g; precision %.4f recall %.4f density %.4f"
          % (k64, d, 4 * d, abs(out["kid_mean"] - k64), out["precision"], out["recall"], out["density"]))
    assert out["kid_per_subset"].shape == (10,) and abs(out["kid_mean"] - k64) <= 4 * d


def test_cli_round_trip(gpu_ctx, tmp_path, capsys):
    """fid.py --metrics fid,kid,pr on two archives prints the FID line of today and one line per further metric, with the values metrics_from_arrays
    gives in this process; with the default flags the output is the FID line alone."""
    from ladder_latent_data_distribution_modelling_amd import fid as F
    real, gen, _ = e2e_sets()
    a, b, w = str(tmp_path / "real.npz"), str(tmp_path / "gen.npz"), str(tmp_path / "w.npz")
    np.savez(a, sampled_images=real)
    np.savez(b, sampled_images=gen)
    np.savez(w, **weights())
    features = F.VGG16Features(gpu_ctx, weights(), "avg", input_size=32)
    want = F.metrics_from_arrays(real, gen, features, metrics=("fid", "kid", "pr"), k=2, n_subsets=4, subset_size=12, seed=5)
    capsys.readouterr()
    score = F.main(["--real", a, "--generated", b, "--weights", w, "--input-size", "32"])
    assert capsys.readouterr().out == "FID score between {} and {} is:\n{}\n".format(a, b, score) and score == want["fid"]
    cmd = [sys.executable, os.path.join(ROOT, "fid.py"), "--real", a, "--generated", b, "--weights", w, "--input-size", "32", "--metrics", "fid,kid,pr",
           "--k", "2", "--kid-subsets", "4", "--kid-subset-size", "12", "--seed", "5"]
    run = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    assert lines[0] == "FID score between {} and {} is:".format(a, b) and lines[1] == str(want["fid"])
    assert lines[2] == "KID between {} and {} (4 subsets of 12) is:".format(a, b) and lines[3] == "{} +- {}".format(want["kid_mean"], want["kid_std"])
    assert lines[4] == "Precision / recall / density (k = 2) between {} and {} are:".format(a, b)
    assert lines[5] == "{} / {} / {}".format(want["precision"], want["recall"], want["density"]) and len(lines) == 6


# ------------------------------------------------------------------------------------------------ 8. the trainer
def test_trainer_compute_sample_metrics_keeps_the_images_on_the_device(golden_dir, monkeypatch):
    """compute_sample_metrics follows compute_FID: same sampler, same chunks, so its "fid" is compute_FID's value for the same seed, and every
    generate call hands its images to a sink (nothing is copied to the host).  On the CelebA golden model, as the compute_FID test: the feature
    network takes three channels, the MNIST models decode one (latent_match below runs on the MNIST-digit model)."""
    from oracle import ladder_oracle as O
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
    n, sinks, generate = 10, [], model.engine.generate

    def watched(*args, **kw):
        sinks.append(kw.get("sink"))
        return generate(*args, **kw)

    monkeypatch.setattr(model.engine, "generate", watched)
    out = tr.compute_sample_metrics(real, n, weights(), chunk=4, seed=42, input_size=32, k=3, n_subsets=6, subset_size=8)
    assert len(sinks) == 1 and sinks[0] is not None and model.engine.ctx.keep_activations is True
    assert out["fid"] == tr.compute_FID(real, n, weights(), pooling="avg", chunk=4, seed=42, input_size=32)
    assert out["counts_gen"].shape == (n,) and out["counts_real"].shape == (12,) and out["kid_per_subset"].shape == (6,)
    for key in ("fid", "kid_mean", "kid_std", "precision", "recall", "density"):
        assert np.isfinite(out[key]), key
    assert 0.0 <= out["precision"] <= 1.0 and 0.0 <= out["recall"] <= 1.0 and out["density"] >= 0.0 and out["kid_std"] >= 0.0
    assert set(tr.compute_sample_metrics(real, n, weights(), metrics=("pr",), chunk=4, seed=42, input_size=32)) == {
        "precision", "recall", "density", "counts_gen", "counts_real"}
    with pytest.raises(ValueError, match="metrics"):
        tr.compute_sample_metrics(real, n, weights(), metrics=("coverage",))


def test_trainer_latent_match(golden_dir, monkeypatch):
    """latent_match on the MNIST-digit golden model with its mixture on t: shapes, finiteness, ranges.  Then the posterior side is replaced by a second,
    disjoint draw of the prior's own sampler: the two sets have one distribution, and the KID mean lies within 3 standard errors (std / sqrt(subsets))
    of zero."""
    from oracle import ladder_oracle as O
    from ladder_latent_data_distribution_modelling_amd.codes import models as M
    from ladder_latent_data_distribution_modelling_amd.codes.base import BaseTrain_joint
    from ladder_latent_data_distribution_modelling_amd.codes.data_loader import BatchIterator
    from ladder_latent_data_distribution_modelling_amd.codes.session import Session
    d = np.load(os.path.join(golden_dir, "oracle_mnist_digit.npz"))
    cfg = json.loads(str(d["config"]))
    cfg.update(checkpoint_dir="/tmp/", result_dir="/tmp/res/")
    model = M.MNISTModel_digit(cfg, device="cuda:0", values=O.init_params(cfg, seed=5))
    tr = BaseTrain_joint(Session(), model, None, cfg)
    tr.cur_epoch = 3
    tr.gm_params = tr.gm_final_params = tuple(np.asarray(d[key], np.float32) for key in ("gm_w", "gm_m", "gm_c"))
    bs = int(cfg["batch_size"])
    images = np.random.default_rng(0).uniform(0.0, 1.0, (16 * bs, 28, 28, 1)).astype(np.float32)
    out = tr.latent_match(BatchIterator(images, bs, seed=1), 10 * bs + 1, k=3, n_subsets=5, subset_size=16, seed=7)
    assert set(out) == {"kid_mean", "kid_std", "precision", "recall", "density"}
    assert all(isinstance(v, float) and np.isfinite(v) for v in out.values())
    assert 0.0 <= out["precision"] <= 1.0 and 0.0 <= out["recall"] <= 1.0 and out["density"] >= 0.0
    with pytest.raises(ValueError, match="more than k rows"):
        tr.latent_match(BatchIterator(images, bs, seed=1), 3, k=3)
    # the prior against its own second draw
    n, nsub = 2000, 20
    _, twin = tr._prior_sampler("accurate-GM", None, 7)
    drawn = [0]

    def second_draw(_x):
        code = twin.sample(bs, first=10 ** 6 + drawn[0])[0]
        drawn[0] += bs
        return code

    monkeypatch.setattr(model.engine, "sample_code", second_draw)
    same = tr.latent_match(BatchIterator(images, bs, seed=1), n, k=3, n_subsets=nsub, subset_size=200, seed=7)
    print("prior against its own second draw: KID %.3g +- %.3g over %d subsets; precision %.3f recall %.3f" % (
        same["kid_mean"], same["kid_std"], nsub, same["precision"], same["recall"]))
    assert drawn[0] >= n and abs(same["kid_mean"]) <= 3 * same["kid_std"] / np.sqrt(nsub)
