"""Per-call times of the small-tile gather launches of the CelebA step under every variant of ladder_conv2d_fwd_variant / ladder_conv2d_bwd_data_variant /
ladder_dense_fwd_variant (csrc/igemm.hip), beside another build of the library where LADDER_PARENT_LIB names one (its plain entry points; every
output must be bit-equal to it).  Prints one JSON line per call: [median, min] us per launch of 7 x 30 back-to-back launches.

    [LADDER_PARENT_LIB=/path/to/other/libladder_hip.so] python profiles/gather_variants_percall.py [out.json]
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ladder_latent_data_distribution_modelling_amd import _lib as L  # noqa: E402
from ladder_latent_data_distribution_modelling_amd import arch  # noqa: E402

new = L.load()
old = C.CDLL(os.environ["LADDER_PARENT_LIB"]) if os.environ.get("LADDER_PARENT_LIB") else new
for name in ("ladder_conv2d_fwd", "ladder_conv2d_bwd_data", "ladder_dense_fwd"):
    res, args = L.PROTOTYPES[name]
    if old is not new:
        getattr(old, name).restype = res
        getattr(old, name).argtypes = args

st = torch.cuda.current_stream().cuda_stream
torch.manual_seed(0)


def timeit(fn, n=30, reps=7):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) * 1000.0 / n)
    return float(np.median(ts)), float(min(ts))


def p(t):
    return t.data_ptr()


rows = []


def conv_case(tag, N, H, W, Cin, Cout, k, s, pad, bwd):
    pt, Ho = arch.conv_out(H, k, s, pad)
    pl, Wo = arch.conv_out(W, k, s, pad)
    x = torch.randn(N, H, W, Cin, device="cuda")
    w = torch.randn(k, k, Cin, Cout, device="cuda") * 0.02
    b = torch.randn(Cout, device="cuda")
    y = torch.empty(N, Ho, Wo, Cout, device="cuda")
    dy = torch.randn(N, Ho, Wo, Cout, device="cuda")
    dx = torch.empty_like(x)
    geo = (N, H, W, Cin, Ho, Wo, Cout, k, k, s, pt, pl)
    if not bwd:
        nb = max(new.ladder_igemm_fwd_workspace_bytes(N * Ho * Wo, k * k * Cin, Cout), 16)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        f_old = lambda: old.ladder_conv2d_fwd(p(x), p(w), p(b), p(y), *geo, 1, p(ws), nb, st)
        f_new = lambda v: (lambda: new.ladder_conv2d_fwd_variant(p(x), p(w), p(b), p(y), *geo, 1, p(ws), nb, v, st))
        out = y
        flops = 2.0 * N * Ho * Wo * k * k * Cin * Cout
    else:
        nb = max(new.ladder_igemm_fwd_workspace_bytes(N * H * W, k * k * Cout, Cin), 16)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        f_old = lambda: old.ladder_conv2d_bwd_data(p(dy), p(w), p(dx), *geo, p(x), 1, p(ws), nb, st)
        f_new = lambda v: (lambda: new.ladder_conv2d_bwd_data_variant(p(dy), p(w), p(dx), *geo, p(x), 1, p(ws), nb, v, st))
        out = dx
        flops = 2.0 * N * H * W * k * k * Cin * Cout if s == 1 else 2.0 * N * Ho * Wo * k * k * Cin * Cout
    assert f_old() == 0
    torch.cuda.synchronize()
    ref = out.clone()
    rec = {"call": tag, "flops": flops, "parent_us": timeit(f_old)}
    for v in range(8):
        out.fill_(float("nan"))
        assert f_new(v)() == 0
        torch.cuda.synchronize()
        assert torch.equal(out, ref), (tag, v)
        rec["v%d_us" % v] = timeit(f_new(v))
    live = new.ladder_igemm_fwd_live_chunks(*geo, int(bwd), 1)
    full = new.ladder_igemm_fwd_live_chunks(*geo, int(bwd), 0)
    rec["live_fraction"] = live / full
    rows.append(rec)
    print(json.dumps(rec), flush=True)


def dense_case(tag, M, K, N):
    x = torch.randn(M, K, device="cuda")
    w = torch.randn(K, N, device="cuda") * 0.02
    b = torch.randn(N, device="cuda")
    y = torch.empty(M, N, device="cuda")
    nb = max(new.ladder_igemm_fwd_workspace_bytes(M, K, N), 16)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    f_old = lambda: old.ladder_dense_fwd(p(x), p(w), p(b), p(y), M, K, N, 1, p(ws), nb, st)
    f_new = lambda v: (lambda: new.ladder_dense_fwd_variant(p(x), p(w), p(b), p(y), M, K, N, 1, p(ws), nb, v, st))
    assert f_old() == 0
    torch.cuda.synchronize()
    ref = y.clone()
    rec = {"call": tag, "flops": 2.0 * M * K * N, "parent_us": timeit(f_old)}
    for v in (0, 2, 4, 6):
        y.fill_(float("nan"))
        assert f_new(v)() == 0
        torch.cuda.synchronize()
        assert torch.equal(y, ref), (tag, v)
        rec["v%d_us" % v] = timeit(f_new(v))
    rows.append(rec)
    print(json.dumps(rec), flush=True)


conv_case("conv2d_fwd 128 8 8 256 4 4 512 3 3 2", 128, 8, 8, 256, 512, 3, 2, "same", False)
conv_case("conv2d_fwd 128 4 4 512 2 2 512 3 3 1", 128, 4, 4, 512, 512, 3, 1, "valid", False)
conv_case("conv2d_fwd 128 2 2 512 2 2 512 3 3 1", 128, 2, 2, 512, 512, 3, 1, "same", False)
conv_case("conv2d_bwd_data 128 2 2 512 2 2 512 3 3 1", 128, 2, 2, 512, 512, 3, 1, "same", True)
conv_case("conv2d_bwd_data 128 4 4 512 2 2 512 3 3 1", 128, 4, 4, 512, 512, 3, 1, "valid", True)
conv_case("conv2d_bwd_data 128 8 8 256 4 4 512 3 3 2", 128, 8, 8, 256, 512, 3, 2, "same", True)
dense_case("dense_fwd 512 512 4608", 512, 512, 4608)
dense_case("dense_fwd 512 4608 512", 512, 4608, 512)
if len(sys.argv) > 1:
    json.dump(rows, open(sys.argv[1], "w"), indent=1)
