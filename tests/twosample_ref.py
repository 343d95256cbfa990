"""Float64 numpy references for the two-sample metrics (test_twosample_cpu.py, test_gpu_twosample.py): squared distances from explicit differences
(never from a Gram matrix), k-NN radii by sorting with the diagonal excluded by index, ball counts, the polynomial-kernel sums, the KID estimator, the
subset index plan, and the rounding-error bounds the device tests hold the kernels to."""
import numpy as np

U64 = 2.0 ** -53


def sqdist(a, b, block=64):
    """d[i, j] = sum_k (a_ik - b_jk)^2 in float64 from the differences themselves; a [n, D], b [m, D]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((a.shape[0], b.shape[0]))
    for lo in range(0, a.shape[0], block):
        diff = a[lo:lo + block, None, :] - b[None, :, :]
        out[lo:lo + block] = (diff * diff).sum(-1)
    return out


def knn_radii(a, k, d=None):
    """r2[i] = the k-th smallest d[i, j] over j != i: the diagonal is removed by INDEX, the rest sorted."""
    d = sqdist(a, a) if d is None else d
    n = d.shape[0]
    off = d[~np.eye(n, dtype=bool)].reshape(n, n - 1)
    return np.sort(off, axis=1)[:, k - 1]


def ball_counts(q, a, r2, d=None):
    """counts[i] = #{j : d(q_i, a_j) <= r2[j]} (non-strict)."""
    d = sqdist(q, a) if d is None else d
    return (d <= np.asarray(r2)[None, :]).sum(1).astype(np.int32)


def precision_recall(real, gen, k):
    """The definitions of two_sample.precision_recall on float64 distances."""
    real, gen = np.asarray(real, np.float64), np.asarray(gen, np.float64)
    r2_real, r2_gen = knn_radii(real, k), knn_radii(gen, k)
    cg, cr = ball_counts(gen, real, r2_real), ball_counts(real, gen, r2_gen)
    return dict(precision=float((cg > 0).mean()), recall=float((cr > 0).mean()), density=float(cg.sum() / (k * gen.shape[0])), counts_gen=cg, counts_real=cr,
                r2_real=r2_real, r2_gen=r2_gen)


def poly_kernel(x, y, degree, gamma, coef0):
    """(gamma x.y + coef0)^degree, float64, on raw dot products; the power by repeated multiplication, so that exact inputs give exact values."""
    t = gamma * (np.asarray(x, np.float64) @ np.asarray(y, np.float64).T) + coef0
    out = t.copy()
    for _ in range(degree - 1):
        out = out * t
    return out


def poly_sums(x, y, degree, gamma, coef0):
    """(sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{ij} k(x_i, y_j)) of one block."""
    kxx, kyy, kxy = poly_kernel(x, x, degree, gamma, coef0), poly_kernel(y, y, degree, gamma, coef0), poly_kernel(x, y, degree, gamma, coef0)
    return np.array([kxx.sum() - np.trace(kxx), kyy.sum() - np.trace(kyy), kxy.sum()])


def mmd2_direct(x, y, degree, gamma, coef0):
    """The unbiased estimator written out pair by pair (Binkowski et al., 2018, eq. 3 with m = n allowed to differ)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    sx, sy = x.shape[0], y.shape[0]
    k = lambda u, v: (gamma * float(u @ v) + coef0) ** degree  # noqa: E731
    txx = sum(k(x[i], x[j]) for i in range(sx) for j in range(sx) if i != j) / (sx * (sx - 1))
    tyy = sum(k(y[i], y[j]) for i in range(sy) for j in range(sy) if i != j) / (sy * (sy - 1))
    txy = sum(k(x[i], y[j]) for i in range(sx) for j in range(sy)) / (sx * sy)
    return txx + tyy - 2.0 * txy


def subset_plan(n, m, n_subsets, subset_size, seed):
    """Subset b: rng.choice(n, s, replace=False), then rng.choice(m, s, replace=False), one np.random.default_rng(seed)."""
    s = min(subset_size, n, m)
    rng = np.random.default_rng(seed)
    ix, iy = [], []
    for _ in range(n_subsets):
        ix.append(rng.choice(n, s, replace=False))
        iy.append(rng.choice(m, s, replace=False))
    return np.array(ix), np.array(iy)


def kid(x, y, n_subsets, subset_size, seed, degree=3, gamma=None, coef0=1.0):
    """(mean, std, per_subset) of the unbiased MMD^2 over the subsets of subset_plan."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    gamma = 1.0 / x.shape[1] if gamma is None else gamma
    ix, iy = subset_plan(x.shape[0], y.shape[0], n_subsets, subset_size, seed)
    s = ix.shape[1]
    per = np.empty(n_subsets)
    for b in range(n_subsets):
        sxx, syy, sxy = poly_sums(x[ix[b]], y[iy[b]], degree, gamma, coef0)
        per[b] = sxx / (s * (s - 1)) + syy / (s * (s - 1)) - 2.0 * sxy / (s * s)
    return float(per.mean()), float(per.std()), per


# ------------------------------------------------------------------------------------------------ error bounds
def distance_error_bound(a, b, shift):
    """E[i, j] bounding |d_device - d_exact| for d = max(na_i + nb_j - 2 G_ij, 0) about the fp32 `shift`, u = 2^-53:

        E_ij = (D + 3) u (na_i + nb_j + 2 sum_k |a~_ik| |b~_jk|),    a~ = a - shift, b~ = b - shift (exact in float64).

    A norm is a sum of D squares taken in index order: each square rounds once and at most D - 1 additions touch it, |dn| <= D u n.  G_ij is a sum of D
    exact products (2 x 25 bits at most) accumulated over D / 4 MFMA steps: |dG| <= D u sum_k |a~||b~|.  The three-term combination adds two roundings on
    numbers no larger than na + nb + 2 |G|, and |G| <= sum |a~||b~|: together (D + 2) u (...) to first order; (D + 3) covers the second-order terms for
    every D <= 32768.  The clamp at zero moves a value towards the exact one (d_exact >= 0)."""
    a, b = np.asarray(a, np.float64) - shift, np.asarray(b, np.float64) - shift
    D = a.shape[1]
    na, nb = (a * a).sum(1), (b * b).sum(1)
    return (D + 3) * U64 * (na[:, None] + nb[None, :] + 2.0 * (np.abs(a) @ np.abs(b).T))


def poly_sum_bounds(x, y, degree, gamma, coef0):
    """Bounds on |S_device - S_reference| for the three sums of poly_sums, u = 2^-53, one block.

    A dot product of D exact products (fp32 operands: 48 bits) summed in any order: |d dot_ij| <= D u sum_k |x_ik| |y_jk| =: e_ij, on the device and in
    the reference's matrix product alike (2 e_ij between them).  t = gamma dot + coef0 adds two roundings, the power degree - 1 more: a relative
    (degree + 1) u on kappa, each side.  Through the kernel, |d kappa| <= degree (|t| + gamma e)^(degree - 1) gamma e.  Summation: on the device a
    term passes 16 additions per column tile inside its lane, 6 butterfly levels, 3 wavefront additions and one per row tile; numpy sums pairwise,
    under 64 levels: (16 ct + 9 + rt + 64) u sum |kappa|."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    D = x.shape[1]

    def one(p, q, off_diagonal):
        e = D * U64 * (np.abs(p) @ np.abs(q).T)
        t = np.abs(gamma * (p @ q.T) + coef0)
        kap = t ** degree
        per = 2.0 * degree * (t + gamma * e) ** (degree - 1) * gamma * e + 2.0 * (degree + 1) * U64 * kap
        if off_diagonal:
            per, kap = per - np.diag(np.diag(per)), kap - np.diag(np.diag(kap))
        rt, ct = -(-p.shape[0] // 64), -(-q.shape[0] // 64)
        return per.sum() + (16 * ct + 9 + rt + 64) * U64 * kap.sum()

    return np.array([one(x, x, True), one(y, y, True), one(x, y, False)])


def counts_case(D, m, n, seed):
    """Normal data with an offset of 50 for the ball-count tests: n reference rows a, m queries q of which m // 2 sit near a reference row (a_j + 0.25 N:
    inside ball j in high dimensions, inside some ball in low ones) and the rest six units away in every coordinate (outside every ball), so both
    outcomes occur.  -> (q, a, shift): fp32 arrays and the fp32 column mean of a as float64."""
    rng = np.random.default_rng(seed)
    a = (50.0 + rng.standard_normal((n, D))).astype(np.float32)
    near = m // 2
    q = np.concatenate([a[rng.integers(0, n, near)] + 0.25 * rng.standard_normal((near, D)), 56.0 + rng.standard_normal((m - near, D))]).astype(np.float32)
    shift = a.astype(np.float64).mean(0).astype(np.float32).astype(np.float64)
    return q, a, shift


def counts_case_margins(q, a, shift, k):
    """What the exact-flag comparison needs of the INPUTS, from the reference alone.  -> (r2, counts, precision, gap, gap_with_radius):
    gap = min_ij |d_ij - r2_j| / E_ij with E the device bound plus the reference's own rounding of d_ij and r2_j (the issue's condition is gap >= 16);
    gap_with_radius = the same with the device's error in r2_j itself (max_l E^aa_jl) added to E_ij: above 1, the flags also agree when the device
    computed the radii."""
    D = a.shape[1]
    daa, dqa = sqdist(a, a), sqdist(q, a)
    r2 = knn_radii(a, k, daa)
    counts = ball_counts(q, a, r2, dqa)
    E = distance_error_bound(q, a, shift) + reference_distance_error(dqa, D) + reference_distance_error(r2, D)[None, :]
    Erad = (distance_error_bound(a, a, shift) + reference_distance_error(daa, D)).max(1)
    diff = np.abs(dqa - r2[None, :])
    return r2, counts, float((counts > 0).mean()), float((diff / E).min()), float((diff / (E + Erad[None, :])).min())


def reference_distance_error(d, D):
    """The float64 reference's own rounding: every difference, its square and the D - 1 additions round once each on terms that sum to d."""
    return (D + 2) * U64 * d
