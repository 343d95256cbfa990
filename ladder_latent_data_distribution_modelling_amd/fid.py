"""FID evaluation on the device: VGG16 features and the Frechet distance of the reference's `compute_FID_score` (reference codes/utils.py:127-200).

    features = VGG16Features(ctx, "vgg16.npz", pooling="avg")
    score = fid_from_arrays(real_images, generated_images, features)

What is decided here ("FID"): the feature network is VGG16 only; both sets are resized to 64x64 (the reference's `tf.image.resize_images`,
TF1 legacy bilinear) and fed as such; set 1 is always preprocessed as "original" (x/255), set 2 as "generated" (clip to [0, 1]) unless told otherwise;
the weights come from the caller as an npz / dict keyed by the Keras layer names.  The statistics stay on the device in float64 (FrechetStats); the two
D x D eigenproblems of the distance run on the host in numpy float64.

`frechet_distance`, `sqrtm_sym`, `load_vgg16_weights` and `second_set_for` need neither a GPU nor the native library; everything that touches the device
imports torch and the library on first use.

    python3 fid.py --real a.npz --generated b.npz --weights vgg16.npz [--pooling avg|max|none] [--chunk 256]
                   [--metrics fid,kid,pr] [--k 3] [--kid-subsets 100] [--kid-subset-size 1000] [--seed 0]

`metrics_from_arrays` adds KID and precision / recall / density on the same features (two_sample.py): each set still goes through the network once.
"""
import argparse

import numpy as np

# tf.keras.applications.VGG16(include_top=False): (block, convolutions, channels); every convolution 3x3 / SAME / bias / ReLU, a 2x2 / stride-2 VALID
# max pool behind every block
VGG16_BLOCKS = ((1, 2, 64), (2, 2, 128), (3, 3, 256), (4, 3, 512), (5, 3, 512))
POOLINGS = (None, "avg", "max")
MIN_INPUT = 32                        # five pools: anything smaller has no pixel left
SQRT_EPS = 1e-10                      # tf.contrib.gan's _symmetric_matrix_square_root: singular values below it are left as they are
WEIGHTS_HELP = ("pass weights= an .npz (or a dict) keyed by the Keras layer names, block{b}_conv{i}/kernel [3,3,Cin,Cout] (HWIO) and "
                "block{b}_conv{i}/bias [Cout]; INTEGRATION.md (FID) shows how to dump one from tf.keras.applications.VGG16")


def vgg16_layers():
    """[(name, cin, cout)] of the 13 convolutions in order."""
    out, cin = [], 3
    for b, n, c in VGG16_BLOCKS:
        for i in range(1, n + 1):
            out.append(("block%d_conv%d" % (b, i), cin, c))
            cin = c
    return out


class _Validated(dict):
    """What load_vgg16_weights returns: handed to it again, it is passed through (compute_FID_score validates before it touches the device)."""


def load_vgg16_weights(weights):
    """{key: float32 array} of the 26 entries, validated: a missing entry raises KeyError, a mis-shaped one ValueError, both naming the key."""
    if isinstance(weights, _Validated):
        return weights
    if weights is None:
        raise ValueError("no VGG16 weights: none ship with this project and none are fetched -- " + WEIGHTS_HELP)
    src = np.load(weights) if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__") else weights
    out = _Validated()
    for name, cin, cout in vgg16_layers():
        for key, shape in ((name + "/kernel", (3, 3, cin, cout)), (name + "/bias", (cout,))):
            try:
                a = src[key]
            except KeyError:
                raise KeyError("VGG16 weights: missing entry %r" % key) from None
            a = np.asarray(a)
            if tuple(a.shape) != shape:
                raise ValueError("VGG16 weights: entry %r has shape %s, expected %s" % (key, tuple(a.shape), shape))
            out[key] = np.ascontiguousarray(a, np.float32)
    return out


def random_weights(seed=0):
    """Seeded stand-in weights for tests and profiles (none are committed): He-normal kernels (std sqrt(2 / (9 Cin))) and small normal biases, keyed like
    the Keras dump, so that no layer goes dead and no activation explodes."""
    rng, out = np.random.default_rng(seed), {}
    for name, cin, cout in vgg16_layers():
        out[name + "/kernel"] = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        out[name + "/bias"] = (0.05 * rng.standard_normal(cout)).astype(np.float32)
    return out


def check_network(FID_network):
    if FID_network == "inception":
        raise NotImplementedError('FID_network "inception" is not available: only "VGG" (VGG16) is implemented.')
    if FID_network != "VGG":
        raise ValueError('unknown FID_network %r: only "VGG" is implemented' % (FID_network,))


def check_pooling(pooling):
    pooling = None if pooling in (None, "none", "None") else pooling
    if pooling not in POOLINGS:
        raise ValueError("pooling must be None, 'avg' or 'max' (got %r)" % (pooling,))
    return pooling


def input_hw(input_size):
    h, w = (int(input_size),) * 2 if np.ndim(input_size) == 0 else (int(v) for v in input_size)
    if min(h, w) < MIN_INPUT:
        raise ValueError("input_size %s: the five 2x2 pools of VGG16 need at least %d pixels per side" % (input_size, MIN_INPUT))
    return h, w


def second_set_for(array, second_set=None):
    """How the CLI reads the second archive when the caller did not say: bytes (generate.py --uint8) are on the 0..255 scale, so they are "original";
    floats are raw decoder output, "generated".  -> (second_set, note or None)."""
    if second_set is not None:
        return second_set, None
    if np.asarray(array[:0]).dtype == np.uint8:
        return "original", "the generated archive holds uint8 (0..255): preprocessed as 'original' (x/255), not clipped to [0, 1]"
    return "generated", None


# ------------------------------------------------------------------------------------------------ host float64: the distance
def sqrtm_sym(M):
    """Square root of a symmetric matrix by the rule of tf.contrib.gan's `_symmetric_matrix_square_root` (svd: s < 1e-10 stays, else sqrt(s)), stated
    on the eigendecomposition: U diag(sign(l) * (|l| < 1e-10 ? |l| : sqrt|l|)) U^T.  -> (root, its trace)."""
    M = np.asarray(M, np.float64)
    lam, U = np.linalg.eigh((M + M.T) * 0.5)
    a = np.abs(lam)
    f = np.sign(lam) * np.where(a < SQRT_EPS, a, np.sqrt(a))
    return (U * f) @ U.T, float(f.sum())


def frechet_distance(m1, c1, m2, c2):
    """tf.contrib.gan.eval.frechet_classifier_distance_from_activations from the two means and (n - 1)-normalised covariances, in float64:
    tr(C1 + C2) - 2 tr(sqrt(sqrt(C1) C2 sqrt(C1))) + |m1 - m2|^2."""
    m1, m2, c1, c2 = (np.asarray(a, np.float64) for a in (m1, m2, c1, c2))
    r1, _ = sqrtm_sym(c1)
    _, tr = sqrtm_sym(r1 @ c2 @ r1)
    d = m1 - m2
    return float(np.trace(c1) + np.trace(c2) - 2.0 * tr + d @ d)


def moments_from_state(state, D):
    """(n, mean [D], cov [D, D]) float64 from a host copy of the device state (include/ladder_hip.h, N17): mean = c + s/n,
    cov = (S - s s^T / n) / (n - 1), S mirrored from its entries on and above the diagonal.  The last step multiplies by the rounded reciprocal
    1 / (n - 1), as np.cov does, so that sums that are exact give np.cov's bits."""
    state = np.asarray(state, np.float64)
    if not np.isfinite(state[0]) or (state[0] > 0 and int(state[1]) != D):
        raise ValueError("the moments state was fed chunks of another feature width than D = %d" % D)
    n = int(state[0])
    c, s = state[2:2 + D], state[2 + D:2 + 2 * D]
    S = state[2 + 2 * D:2 + 2 * D + D * D].reshape(D, D)
    S = np.triu(S) + np.triu(S, 1).T
    if n < 1:
        raise ValueError("no rows accumulated")
    mean = c + s / n
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = (S - np.outer(s, s) / n) * np.true_divide(1, n - 1)
    return n, mean, cov


# ------------------------------------------------------------------------------------------------ device
class _stage:
    """Brackets the launches of one stage with HIP events and hands them to the installed profiler (layers.PROF, a profiler.KernelProfiler) under the
    stage's name; nothing without one.  The convolution launches inside a layer's bracket are also attributed to their kernel ids by layers._timed."""

    def __init__(self, name, flops=0.0):
        self.name, self.flops = name, flops

    def __enter__(self):
        from . import layers
        self.prof = layers.PROF
        if self.prof is not None:
            import torch
            self.s, self.e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.s.record()

    def __exit__(self, *exc):
        if self.prof is not None:
            self.e.record()
            self.prof.add(self.name, self.s, self.e, self.flops)
        return False


class _FrozenStore:
    """The parameter store a Conv2D reads (w / g / version), for frozen weights outside the model: it never enters arch.param_specs or the
    training ParamStore."""

    GROUP = "fid"

    def __init__(self):
        self.w, self.g, self.version = {}, {}, {self.GROUP: 0}

    @classmethod
    def group_of(cls, _name):
        return cls.GROUP


class VGG16Features:
    """The convolutional stack of tf.keras.applications.VGG16(include_top=False, pooling=pooling) on frozen weights (reference codes/utils.py:184-194).
    Every convolution goes through Conv2D.route with ReLU in the kernel epilogue, forward only, nothing kept."""

    def __init__(self, ctx, weights, pooling="avg", input_size=64, matmul_precision="f32"):
        import torch
        from . import layers
        self.pooling = check_pooling(pooling)
        self.hw = input_hw(input_size)
        values = load_vgg16_weights(weights)
        if matmul_precision not in layers.PRECISIONS:
            raise ValueError("matmul_precision must be one of %s" % sorted(layers.PRECISIONS))
        # a context of its own (precision, packed banks, workspace, forward-only flag); only the copy stream is the caller's
        c = self.ctx = ctx.fork(precision=layers.PRECISIONS[matmul_precision], forward_only=True)
        self.store = _FrozenStore()
        for k, v in values.items():
            self.store.w[k] = torch.as_tensor(v).to(c.device)
        self.blocks = [[layers.Conv2D(c, self.store, "block%d_conv%d" % (b, i), 3, cin if i == 1 else ch, ch, act="relu") for i in range(1, n + 1)]
                       for (b, n, ch), cin in zip(VGG16_BLOCKS, (3, 64, 128, 256, 512))]
        h, w = self.hw
        self.out_hw = (h >> 5, w >> 5)
        self.D = 512 if self.pooling else 512 * self.out_hw[0] * self.out_hw[1]

    def routes(self, n):
        """[(layer name, forward entry point, profiler kernel id)] for a chunk of n images: what each of the 13 layers runs on."""
        (h, w), out = self.hw, []
        for blk in self.blocks:
            for conv in blk:
                r = conv.route((n, h, w, conv.cin))
                out.append((conv.name, r.fwd.fn, r.fwd.kid))
            h, w = h // 2, w // 2
        return out

    def preprocess(self, images, mode):
        """[n, H, W, 3] uint8 / float (device or host) -> [n, h, w, 3] fp32 on the device: scale / clip / affine + legacy bilinear resize, one launch."""
        import torch
        from . import _lib as L
        if mode not in ("original", "generated"):
            raise ValueError("mode must be 'original' or 'generated' (got %r)" % (mode,))
        x = images if isinstance(images, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(images))
        if x.dtype != torch.uint8:
            x = x.to(torch.float32)
        x = x.to(self.ctx.device).contiguous()
        if x.dim() != 4 or int(x.shape[3]) != 3:
            raise ValueError("images must be [n, H, W, 3] (got %s)" % (tuple(x.shape),))
        n, H, W, _ = (int(v) for v in x.shape)
        y = self.ctx.empty(n, self.hw[0], self.hw[1], 3)
        if n:
            with _stage("preprocess"):
                L.call("ladder_fid_preprocess", x.data_ptr(), int(x.dtype == torch.uint8), y.data_ptr(), n, H, W, 3, self.hw[0], self.hw[1],
                       0 if mode == "original" else 1, self.ctx.stream)
        return y

    def stack(self, x):
        """The 13 convolutions, 5 pools and the final pooling on preprocessed [n, h, w, 3] -> [n, D]."""
        from . import _lib as L
        ctx, st = self.ctx, self.ctx.stream
        for blk in self.blocks:
            for conv in blk:
                r = conv.route(x.shape)
                with _stage("%s [%s, id %d]" % (conv.name, r.fwd.fn, r.fwd.kid), r.flops):
                    x = conv.forward(x)
                conv.kept = None
            n, h, w, ch = (int(v) for v in x.shape)
            y = ctx.empty(n, h // 2, w // 2, ch)
            with _stage("maxpool"):
                L.call("ladder_maxpool2x2_fwd", x.data_ptr(), y.data_ptr(), n, h, w, ch, st)
            x = y
        n, h, w, ch = (int(v) for v in x.shape)
        if self.pooling is None:
            return x.reshape(n, h * w * ch)
        y = ctx.empty(n, ch)
        with _stage("global_pool"):
            L.call("ladder_global_pool", x.data_ptr(), y.data_ptr(), n, h * w, ch, 0 if self.pooling == "avg" else 1, st)
        return y

    def __call__(self, images, mode):
        x = self.preprocess(images, mode)
        if int(x.shape[0]) == 0:
            return self.ctx.empty(0, self.D)
        return self.stack(x)


class FrechetStats:
    """Streaming float64 mean / covariance of feature chunks on the device (ladder_moments_accumulate)."""

    def __init__(self, ctx, D):
        import torch
        from . import _lib as L
        self.ctx, self.D = ctx, int(D)
        nd = L.query("ladder_moments_state_doubles", self.D)
        if nd == 0:
            raise ValueError("FrechetStats: D >= 1 (got %d)" % self.D)
        self.state = torch.zeros(nd, dtype=torch.float64, device=ctx.device)
        self._ws = None

    def update(self, features):
        """Adds the rows of `features` [n, D] (fp32, on the device): enqueued on the current stream, never synchronises."""
        import torch
        from . import _lib as L
        if features.dim() != 2 or int(features.shape[1]) != self.D or features.dtype != torch.float32:
            raise ValueError("FrechetStats.update: expected fp32 [n, %d] (got %s %s)" % (self.D, features.dtype, tuple(features.shape)))
        n = int(features.shape[0])
        if n == 0:
            return
        features = features.contiguous()
        nb = L.query("ladder_moments_workspace_bytes", n, self.D)
        if self._ws is None or self._ws.numel() < nb:
            self._ws = torch.empty(nb, dtype=torch.uint8, device=self.ctx.device)      # (stream-ordered: launches already enqueued keep the old buffer's memory)
        with _stage("moments"):
            L.call("ladder_moments_accumulate", features.data_ptr(), n, self.D, self.state.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                   self.ctx.stream)

    def moments(self):
        """One copy of the state to the host -> (n, mean [D], cov [D, D]) in float64."""
        return moments_from_state(self.state.cpu().numpy(), self.D)


def _device_chunks(arr, chunk, features):
    """Yields the chunks of a host array [n, H, W, 3] as device tensors.  Two pinned and two device buffers: the copy of chunk k+1 runs on the copy
    stream while the caller works on chunk k.  uint8 stays uint8 (the preprocess kernel reads bytes), anything else travels as fp32."""
    import torch
    ctx = features.ctx
    if isinstance(arr, torch.Tensor) and arr.is_cuda:
        for lo in range(0, int(arr.shape[0]), chunk):
            yield arr[lo:lo + chunk]
        return
    n = int(arr.shape[0])
    if n == 0:
        return
    cs, main = ctx.copy_stream, torch.cuda.current_stream(ctx.device)          # (the stream LadderEngine.generate copies on)
    dt = torch.uint8 if arr.dtype == np.uint8 else torch.float32
    shape = (min(chunk, n),) + tuple(int(v) for v in arr.shape[1:])
    pinned = [torch.empty(shape, dtype=dt, pin_memory=True) for _ in range(2)]
    dev = [torch.empty(shape, dtype=dt, device=ctx.device) for _ in range(2)]
    # The device buffers come from the main stream's allocator pool: their memory may be what a tensor of an earlier call occupied, with main-stream
    # kernels that use it still in flight.  The copy stream therefore starts behind everything enqueued on the main stream so far; from the second use
    # of a buffer on, `consumed` orders the copy behind the work on the chunk that last sat in it.
    born = torch.cuda.Event()
    born.record(main)
    copied, consumed = [None, None], [born, born]

    def start(k):
        lo, slot = k * chunk, k & 1
        b = min(chunk, n - lo)
        if copied[slot] is not None:
            copied[slot].synchronize()           # (host: the pinned buffer's previous copy has left it)
        pinned[slot][:b].numpy()[...] = arr[lo:lo + b]
        with torch.cuda.stream(cs):
            cs.wait_event(consumed[slot])        # (device: the work on the chunk that last sat in this buffer -- or in its memory -- is done)
            dev[slot][:b].copy_(pinned[slot][:b], non_blocking=True)
            copied[slot] = torch.cuda.Event()
            copied[slot].record(cs)
        return b

    nk = (n + chunk - 1) // chunk
    try:
        b_next = start(0)
        for k in range(nk):
            slot, b = k & 1, b_next
            if k + 1 < nk:
                b_next = start(k + 1)
            main.wait_event(copied[slot])
            yield dev[slot][:b]
            consumed[slot] = torch.cuda.Event()
            consumed[slot].record(main)
    finally:
        for e in copied:                         # nothing may outlive its copy
            if e is not None:
                e.synchronize()


def accumulate_array(arr, features, mode, chunk=256, stats=None):
    """All of `arr` through `features` into a FrechetStats (a new one unless given)."""
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk >= 1 (got %d)" % chunk)
    stats = stats or FrechetStats(features.ctx, features.D)
    for x in _device_chunks(arr, chunk, features):
        stats.update(features(x, mode))
    return stats


def fid_from_arrays(a, b, features, chunk=256, second_set="generated"):
    """The reference's score for two image sets [n, H, W, 3] (host arrays or device tensors): set 1 preprocessed as "original", set 2 as "generated"
    unless second_set says otherwise (codes/utils.py:141-153)."""
    s1 = accumulate_array(a, features, "original", chunk)
    s2 = accumulate_array(b, features, "generated" if second_set == "generated" else "original", chunk)
    (_, m1, c1), (_, m2, c2) = s1.moments(), s2.moments()
    return frechet_distance(m1, c1, m2, c2)


class MetricSets:
    """What the metrics named in `metrics` (two_sample.METRICS) need of the two feature sets (0: real, 1: generated): a FrechetStats each for "fid", a
    FeatureBank each for "kid" and "pr".  feed() never synchronises; results() copies to the host once per metric."""

    def __init__(self, features, metrics):
        from . import two_sample as T
        self.metrics = T.check_metrics(metrics)
        self.stats = [FrechetStats(features.ctx, features.D) for _ in range(2)] if "fid" in self.metrics else None
        self.banks = [T.FeatureBank(features.ctx, features.D) for _ in range(2)] if set(self.metrics) - {"fid"} else None

    def feed(self, which, f):
        if self.stats is not None:
            self.stats[which].update(f)
        if self.banks is not None:
            self.banks[which].add(f)

    def results(self, k=3, n_subsets=100, subset_size=1000, seed=0):
        """-> dict with  fid | kid_mean, kid_std, kid_per_subset | precision, recall, density, counts_gen, counts_real."""
        from . import two_sample as T
        out = {}
        if "fid" in self.metrics:
            (_, m1, c1), (_, m2, c2) = self.stats[0].moments(), self.stats[1].moments()
            out["fid"] = frechet_distance(m1, c1, m2, c2)
        if "kid" in self.metrics:
            out["kid_mean"], out["kid_std"], out["kid_per_subset"] = T.kid(*self.banks, n_subsets=n_subsets, subset_size=subset_size, seed=seed)
        if "pr" in self.metrics:
            out.update(T.precision_recall(*self.banks, k=k))
        return out


def metrics_from_arrays(a, b, features, metrics=("fid",), chunk=256, second_set="generated", k=3, n_subsets=100, subset_size=1000, seed=0):
    """The metrics named in `metrics` for two image sets, each sent through `features` ONCE (MetricSets).  "fid" is fid_from_arrays' value bit for bit
    (same chunks, same updates); `k` is the neighbour rank of the precision / recall balls, n_subsets / subset_size / seed are KID's (two_sample.kid)."""
    from . import two_sample as T
    metrics = T.check_metrics(metrics)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk >= 1 (got %d)" % chunk)
    n, m = int(a.shape[0]), int(b.shape[0])
    if "pr" in metrics:
        T.check_k(k, n, m)
    if "kid" in metrics and min(n, m, int(subset_size)) < 2:
        raise ValueError("KID needs subsets of at least 2 rows (subset_size %d, %d and %d images)" % (subset_size, n, m))
    sets = MetricSets(features, metrics)
    for which, (arr, mode) in enumerate(((a, "original"), (b, "generated" if second_set == "generated" else "original"))):
        for x in _device_chunks(arr, chunk, features):
            sets.feed(which, features(x, mode))
    return sets.results(k, n_subsets, subset_size, seed)


def load_images(path_or_array):
    """The `sampled_images` array of an archive (codes/utils.py:142-143, 147-148), or the array itself."""
    if isinstance(path_or_array, (str, bytes)) or hasattr(path_or_array, "__fspath__"):
        return np.load(path_or_array)["sampled_images"]
    return path_or_array


# ------------------------------------------------------------------------------------------------ command line
def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="fid.py", description="FID between two `sampled_images` archives on VGG16 features (MI355X HIP path)")
    ap.add_argument("--real", metavar="A.npz", required=True, help="first archive: always preprocessed as 'original' (x/255)")
    ap.add_argument("--generated", metavar="B.npz", required=True, help="second archive, e.g. written by generate.py")
    ap.add_argument("--weights", metavar="W.npz", required=True, help="VGG16 weights keyed by the Keras layer names (INTEGRATION.md, FID)")
    ap.add_argument("--pooling", choices=("avg", "max", "none"), default="avg")
    ap.add_argument("--chunk", type=int, default=256, help="images per batch")
    ap.add_argument("--second-set", choices=("generated", "original"), default=None,
                    help="preprocessing of the second archive (default: 'original' for uint8 bytes, 'generated' for floats)")
    ap.add_argument("--input-size", type=int, default=64)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--metrics", default="fid", help="comma-separated: fid, kid (kernel inception distance), pr (precision / recall / density)")
    ap.add_argument("--k", type=int, default=3, help="neighbour rank of the precision / recall balls")
    ap.add_argument("--kid-subsets", type=int, default=100)
    ap.add_argument("--kid-subset-size", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0, help="seed of the KID subsets")
    a = ap.parse_args(argv)
    if a.chunk < 1:
        ap.error("--chunk must be >= 1")
    from . import two_sample as T
    try:
        a.metrics = T.check_metrics(a.metrics)
    except ValueError as e:
        ap.error(str(e))
    return a


def sample_metrics_archives(data_file1, data_file2, FID_network, pooling_option, second_set, weights, chunk, input_size, device,
                            metrics=("fid", "kid", "pr"), k=3, n_subsets=100, subset_size=1000, seed=0):
    """compute_sample_metrics (codes/utils.py) behind its argument checks.  second_set None: decided from the second array's dtype (second_set_for).
    Each archive is opened once, the weights are validated once, both before the device is touched.  Prints the FID line of the reference, then one
    line per further metric.  -> the dict of metrics_from_arrays."""
    from . import two_sample as T
    metrics = T.check_metrics(metrics)
    check_network(FID_network)
    pooling = check_pooling(pooling_option)
    input_hw(input_size)
    values = load_vgg16_weights(weights)
    a, b = load_images(data_file1), load_images(data_file2)
    second_set, note = second_set_for(b, second_set)
    if note:
        print("fid.py: " + note)
    if "pr" in metrics:
        T.check_k(k, int(a.shape[0]), int(b.shape[0]))
    from .layers import Ctx
    features = VGG16Features(Ctx(device), values, pooling, input_size)
    out = metrics_from_arrays(a, b, features, metrics, chunk, second_set, k, n_subsets, subset_size, seed)
    if "fid" in metrics:
        print("FID score between {} and {} is:\n{}".format(data_file1, data_file2, out["fid"]))
    if "kid" in metrics:
        print("KID between {} and {} ({} subsets of {}) is:\n{} +- {}".format(data_file1, data_file2, len(out["kid_per_subset"]),
                                                                              min(subset_size, int(a.shape[0]), int(b.shape[0])), out["kid_mean"], out["kid_std"]))
    if "pr" in metrics:
        print("Precision / recall / density (k = {}) between {} and {} are:\n{} / {} / {}".format(k, data_file1, data_file2, out["precision"], out["recall"],
                                                                                                   out["density"]))
    return out


def score_archives(data_file1, data_file2, FID_network, pooling_option, second_set, weights, chunk, input_size, device):
    """compute_FID_score (codes/utils.py): sample_metrics_archives for "fid" alone -> the score."""
    return sample_metrics_archives(data_file1, data_file2, FID_network, pooling_option, second_set, weights, chunk, input_size, device, ("fid",))["fid"]


def main(argv=None):
    a = parse_args(argv)
    out = sample_metrics_archives(a.real, a.generated, "VGG", a.pooling, a.second_set, a.weights, a.chunk, a.input_size, a.device, a.metrics, a.k,
                                  a.kid_subsets, a.kid_subset_size, a.seed)
    return out["fid"] if a.metrics == ("fid",) else out


if __name__ == "__main__":
    main()
