"""Two-sample metrics on the device (csrc/twosample.hip): improved precision / recall and the kernel inception distance between two row sets.

    bank_r, bank_g = FeatureBank(ctx, 512), FeatureBank(ctx, 512)
    bank_r.add(features(real_chunk, "original")); bank_g.add(features(generated_chunk, "generated")); ...
    pr = precision_recall(bank_r, bank_g, k=3)          # dict(precision, recall, density, counts_gen, counts_real)
    mean, std, per_subset = kid(bank_r, bank_g)         # 100 subsets of 1000 rows, cubic kernel

The rows are fp32 [n, D] on the device: VGG16 features (fid.VGG16Features) or latent codes alike.  What is decided here ("Two-sample metrics on
the device"):

  precision / recall (Kynkaanniemi et al., 2019)  every row of a set gets the squared distance to its k-th nearest OTHER row of the same set as the
      radius of a ball; precision = the share of generated rows inside at least one real ball, recall = the share of real rows inside at least one
      generated ball, density (Naeem et al., 2020) = the number of real balls a generated row sits in, averaged and divided by k.  Membership is
      d <= r2, non-strict, as in the published implementation.  All distances are taken about ONE shift, the fp32 column mean of the real set.
  KID (Binkowski et al., 2018)  the unbiased MMD^2 with the kernel (gamma u.v + coef0)^degree (cubic, gamma = 1 / D, coef0 = 1) on n_subsets random
      subsets of s = min(subset_size, n, m) rows of either set, drawn without replacement from ONE numpy Generator -- x's rows first, then y's, subset
      after subset (subset_plan) --, gathered on the device and summed in ONE launch; mean and standard deviation over the subsets.

`kid_from_sums`, `subset_plan`, `check_metrics` and the argument checks need neither a GPU nor the native library; everything that touches the device
imports torch and the library on first use.
"""
import numpy as np

METRICS = ("fid", "kid", "pr")
MAX_K, MAX_D, MAX_ROWS, MAX_BLOCKS = 8, 32768, 1 << 24, 65535          # the limits of include/ladder_hip.h, N24


def check_metrics(metrics):
    """A tuple of metric names out of METRICS (a comma-separated string is split); an unknown or missing name raises ValueError."""
    names = tuple(s.strip() for s in metrics.split(",")) if isinstance(metrics, str) else tuple(metrics)
    bad = [m for m in names if m not in METRICS]
    if bad or not names:
        raise ValueError("metrics must name some of %s (got %r)" % (list(METRICS), metrics))
    return names


def _rows_of(x, what):
    """(n, D) of a FeatureBank or a 2-d array / tensor; no device access."""
    shape = (x.n, x.D) if isinstance(x, FeatureBank) else tuple(int(v) for v in getattr(x, "shape", ()))
    if len(shape) != 2:
        raise ValueError("%s must be rows [n, D] (got shape %s)" % (what, shape))
    return shape


def check_pair(a, b, names=("real", "gen")):
    """Both sets non-empty, of one width inside the limits.  -> (n, m, D)."""
    (n, D), (m, D2) = _rows_of(a, names[0]), _rows_of(b, names[1])
    if n < 1 or m < 1:
        raise ValueError("%s and %s must not be empty (got %d and %d rows)" % (names[0], names[1], n, m))
    if D != D2:
        raise ValueError("%s and %s differ in width: %d and %d" % (names[0], names[1], D, D2))
    if not 1 <= D <= MAX_D or max(n, m) > MAX_ROWS:
        raise ValueError("two-sample metrics take 1 <= D <= %d and at most %d rows per set (got D = %d, %d and %d rows)" % (MAX_D, MAX_ROWS, D, n, m))
    return n, m, D


def check_k(k, n, m):
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError("k must be in 1 .. %d (got %d)" % (MAX_K, k))
    if k >= min(n, m):
        raise ValueError("k = %d needs more than k rows in either set (got %d and %d): the k-th neighbour excludes the row itself" % (k, n, m))
    return k


def subset_plan(n, m, n_subsets, subset_size, seed=0):
    """Row indices of the KID subsets: s = min(subset_size, n, m); for subset b, rng.choice(n, s, replace=False) first, then rng.choice(m, s,
    replace=False), from one np.random.default_rng(seed).  -> (ix [n_subsets, s], iy [n_subsets, s]) int64."""
    n_subsets, s = int(n_subsets), min(int(subset_size), int(n), int(m))
    if n_subsets < 1 or n_subsets > MAX_BLOCKS:
        raise ValueError("n_subsets must be in 1 .. %d (got %d)" % (MAX_BLOCKS, n_subsets))
    if s < 2:
        raise ValueError("KID needs subsets of at least 2 rows (subset_size %d, %d and %d rows)" % (subset_size, n, m))
    if n_subsets * s > MAX_ROWS:
        raise ValueError("n_subsets * subset size = %d exceeds %d gathered rows" % (n_subsets * s, MAX_ROWS))
    rng = np.random.default_rng(seed)
    ix, iy = np.empty((n_subsets, s), np.int64), np.empty((n_subsets, s), np.int64)
    for b in range(n_subsets):
        ix[b] = rng.choice(n, s, replace=False)
        iy[b] = rng.choice(m, s, replace=False)
    return ix, iy


def kid_from_sums(sums, sx, sy=None):
    """sums [n_subsets, 3] = (sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{ij} k(x_i, y_j)) -> (mean, std, per_subset) of
    MMD^2_b = Sxx / (sx (sx - 1)) + Syy / (sy (sy - 1)) - 2 Sxy / (sx sy), float64 on the host."""
    sums = np.asarray(sums, np.float64).reshape(-1, 3)
    sx = int(sx)
    sy = sx if sy is None else int(sy)
    if sx < 2 or sy < 2:
        raise ValueError("the unbiased MMD^2 needs at least 2 rows per subset (got %d and %d)" % (sx, sy))
    per = sums[:, 0] / (sx * (sx - 1)) + sums[:, 1] / (sy * (sy - 1)) - 2.0 * sums[:, 2] / (sx * sy)
    return float(per.mean()), float(per.std()), per


def check_kernel(degree, D, gamma, coef0):
    degree = int(degree)
    if not 1 <= degree <= 4:
        raise ValueError("degree must be in 1 .. 4 (got %d)" % degree)
    return degree, (1.0 / D if gamma is None else float(gamma)), float(coef0)


# ------------------------------------------------------------------------------------------------ device
def _stream(t):
    import torch
    return torch.cuda.current_stream(t.device).cuda_stream


def _rows(x, what):
    """The fp32 contiguous device view [n, D] of a FeatureBank or tensor."""
    import torch
    t = x.rows if isinstance(x, FeatureBank) else x
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32:
        raise ValueError("%s must be a FeatureBank or an fp32 device tensor [n, D]" % what)
    return t.contiguous()


class FeatureBank:
    """Feature rows [n, D] collected on the device chunk by chunk.  Appends are enqueued on the current stream and never synchronise; the buffer grows
    by doubling (the copy into the new buffer is stream-ordered behind the appends so far)."""

    def __init__(self, ctx, D, capacity=1024):
        self.ctx, self.D, self.n = ctx, int(D), 0
        if not 1 <= self.D <= MAX_D:
            raise ValueError("FeatureBank: 1 <= D <= %d (got %d)" % (MAX_D, self.D))
        self._cap0, self._buf = max(1, int(capacity)), None

    def add(self, features):
        import torch
        if features.dim() != 2 or int(features.shape[1]) != self.D or features.dtype != torch.float32:
            raise ValueError("FeatureBank.add: expected fp32 [b, %d] (got %s %s)" % (self.D, features.dtype, tuple(features.shape)))
        b = int(features.shape[0])
        if self.n + b > MAX_ROWS:
            raise ValueError("FeatureBank: at most %d rows" % MAX_ROWS)
        if self._buf is None or self.n + b > int(self._buf.shape[0]):
            cap = max(self._cap0, self.n + b, 2 * (0 if self._buf is None else int(self._buf.shape[0])))
            grown = torch.empty(cap, self.D, dtype=torch.float32, device=self.ctx.device)
            if self.n:
                grown[:self.n].copy_(self._buf[:self.n])
            self._buf = grown
        self._buf[self.n:self.n + b].copy_(features)
        self.n += b

    @property
    def rows(self):
        import torch
        return self._buf[:self.n] if self._buf is not None else torch.empty(0, self.D, dtype=torch.float32, device=self.ctx.device)


def row_norms(x, shift=None):
    """norms [n] float64 on the device: sum_k (x_ik - shift_k)^2."""
    import torch
    from . import _lib as L
    n, D = (int(v) for v in x.shape)
    out = torch.empty(n, dtype=torch.float64, device=x.device)
    L.call("ladder_pairs_row_norms", x.data_ptr(), n, D, 0 if shift is None else shift.data_ptr(), out.data_ptr(), _stream(x))
    return out


def _workspace(x, nbytes):
    import torch
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=x.device)


def knn_radii(a, norms, shift, k):
    """r2 [n] float64 on the device: the squared distance of every row of `a` to its k-th nearest other row."""
    import torch
    from . import _lib as L
    n, D = (int(v) for v in a.shape)
    ws = _workspace(a, L.query("ladder_pairs_workspace_bytes", n, n, D, k, 0))
    r2 = torch.empty(n, dtype=torch.float64, device=a.device)
    L.call("ladder_pairs_knn_radii", a.data_ptr(), norms.data_ptr(), n, D, 0 if shift is None else shift.data_ptr(), k, r2.data_ptr(), ws.data_ptr(),
           ws.numel(), _stream(a))
    return r2


def ball_counts(q, norms_q, a, norms_a, r2, shift):
    """counts [m] int32 on the device: for every query row the number of balls (a_j, r2_j) that hold it."""
    import torch
    from . import _lib as L
    (m, D), n = (int(v) for v in q.shape), int(a.shape[0])
    ws = _workspace(q, L.query("ladder_pairs_workspace_bytes", m, n, D, 0, 0))
    counts = torch.empty(m, dtype=torch.int32, device=q.device)
    L.call("ladder_pairs_ball_counts", q.data_ptr(), norms_q.data_ptr(), m, a.data_ptr(), norms_a.data_ptr(), r2.data_ptr(), n, D,
           0 if shift is None else shift.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), _stream(q))
    return counts


def poly_sums(x, sx, y, sy, n_blocks, degree, gamma, coef0):
    """sums [n_blocks, 3] float64 on the device from gathered blocks x [n_blocks * sx, D], y [n_blocks * sy, D]."""
    import torch
    from . import _lib as L
    D = int(x.shape[1])
    ws = _workspace(x, L.query("ladder_pairs_workspace_bytes", sx, sy, D, 0, n_blocks))
    sums = torch.empty(n_blocks, 3, dtype=torch.float64, device=x.device)
    L.call("ladder_pairs_poly_sums", x.data_ptr(), sx, y.data_ptr(), sy, n_blocks, D, degree, gamma, coef0, sums.data_ptr(), ws.data_ptr(), ws.numel(),
           _stream(x))
    return sums


def precision_recall(real, gen, k=3):
    """dict(precision, recall, density, counts_gen [m], counts_real [n]) for fp32 device rows real [n, D], gen [m, D] (FeatureBanks or tensors).  Two
    radii passes, two count passes, one copy to the host at the end."""
    import torch
    n, m, _ = check_pair(real, gen)
    k = check_k(k, n, m)
    real, gen = _rows(real, "real"), _rows(gen, "gen")
    shift = real.mean(0).contiguous()                                 # fp32, the same vector for all four walks
    nr, ng = row_norms(real, shift), row_norms(gen, shift)
    r2_real, r2_gen = knn_radii(real, nr, shift, k), knn_radii(gen, ng, shift, k)
    counts_gen = ball_counts(gen, ng, real, nr, r2_real, shift)       # generated rows inside real balls: precision, density
    counts_real = ball_counts(real, nr, gen, ng, r2_gen, shift)       # real rows inside generated balls: recall
    both = torch.cat([counts_gen, counts_real]).cpu().numpy()
    cg, cr = both[:m], both[m:]
    return dict(precision=float((cg > 0).mean()), recall=float((cr > 0).mean()), density=float(cg.sum(dtype=np.int64) / (k * m)), counts_gen=cg,
                counts_real=cr)


def kid(x, y, n_subsets=100, subset_size=1000, seed=0, degree=3, gamma=None, coef0=1.0):
    """(mean, std, per_subset [n_subsets]) of the unbiased MMD^2 between fp32 device rows x [n, D] and y [m, D] over the subsets of subset_plan."""
    import torch
    n, m, D = check_pair(x, y, ("x", "y"))
    degree, gamma, coef0 = check_kernel(degree, D, gamma, coef0)
    ix, iy = subset_plan(n, m, n_subsets, subset_size, seed)
    x, y = _rows(x, "x"), _rows(y, "y")
    nb, s = ix.shape
    gx = x.index_select(0, torch.as_tensor(ix.reshape(-1)).to(x.device, non_blocking=True))
    gy = y.index_select(0, torch.as_tensor(iy.reshape(-1)).to(y.device, non_blocking=True))
    sums = poly_sums(gx, s, gy, s, nb, degree, gamma, coef0)
    return kid_from_sums(sums.cpu().numpy(), s)
