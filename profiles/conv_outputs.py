"""Every output of the implicit-GEMM convolution / dense entry points (csrc/igemm.hip, igemm_wgrad.hip, igemm_split.hip, convdirect.hip) on
fixed seeded inputs, written to one .npz -- for whichever library LADDER_HIP_LIB names.

    LADDER_HIP_LIB=/path/to/libladder_hip.so python profiles/conv_outputs.py out.npz
    python profiles/conv_outputs.py --compare a.npz b.npz        # table of bit equality per array (NaN positions must match, -0.0 != +0.0)

Run it once per library, each in a fresh process, and compare: two builds whose kernels and launch plans are the same give equal arrays bit
for bit, and the same return code for every call (the `rc` arrays; rejected calls included).  The cases are the smallest that reach each
route (CONV_CASES of tests/test_gpu_kernels.py): scalar gather, ragged, the 5x5 stride-2 parity classes, 1x1 stride 2 with empty classes,
split-K, halo forward, the halo filter gradient on each patch shape and at stride 2, strided split-K classes, conv_cout1, conv_smallcin,
conv1x1_smallcout; the dense shapes of test_dense_fwd_bwd; two GATHER_CASES of tests/test_gpu_split.py per precision for the split kernels;
ladder_conv2d_fwd_bnstats; ladder_reduce_splits at 1, 31 and 32 splits; the rejected calls of test_rejections_return_codes.  Every call
runs with its workspace and with ws = NULL, gated and ungated, with db and with db = NULL.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# N, H, W, Cin, Cout, k, stride, padding, act
CONV = [
    (2, 32, 32, 3, 128, 3, 2, "same", None), (1, 7, 9, 20, 36, 3, 1, "same", "relu"), (2, 10, 14, 16, 32, 5, 2, "same", None),
    (2, 8, 8, 16, 48, 1, 2, "same", None), (32, 2, 2, 256, 256, 3, 1, "same", None), (16, 64, 64, 32, 256, 3, 1, "same", "leaky_relu"),
    (32, 64, 64, 64, 128, 3, 1, "same", None), (32, 16, 16, 512, 160, 3, 1, "same", None), (64, 8, 8, 512, 512, 3, 1, "same", "leaky_relu"),
    (64, 64, 64, 128, 128, 3, 2, "same", None), (128, 8, 8, 256, 512, 3, 2, "same", "leaky_relu"), (4, 32, 32, 16, 1, 5, 1, "valid", "relu"),
    (9, 32, 32, 64, 1, 5, 1, "valid", "relu"), (2, 8, 8, 128, 3, 1, 1, "same", None),
    (5, 128, 128, 64, 1, 1, 1, "same", None),          # enough pixels for conv1x1_smallcout_kernel
]
DENSE = [(128, 2048, 64, None), (128, 4096, 64, "relu"), (128, 512, 512, "leaky_relu"), (7, 2, 32, "relu"), (256, 64, 4096, "leaky_relu"),
         (100, 33, 2, None), (4, 16, 1024, "tanh")]
GATHER = [(37, 3, 5, 128, 160, 3, 1, "same", None), (64, 16, 16, 256, 256, 3, 2, "same", "leaky_relu")]
PRECS = {"f16x3": 4, "bf16x6": 3, "bf16x3": 2}
BNSTATS = (80, 64, 64, 128, 128, 3, 2, "same", "leaky_relu")
E_SHAPE, E_ALIGN, E_WORKSPACE = -1, -2, -3


def compare(a, b):
    a, b = np.load(a), np.load(b)
    assert sorted(a.files) == sorted(b.files), (sorted(set(a.files) ^ set(b.files)))
    bad = 0
    print("| array | shape | NaNs | differing elements |\n|---|---|---|---|")
    for k in sorted(set(a.files) - {"library"}):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype:
            diff = "shape or type"
        elif x.dtype.kind == "f":                                           # bit for bit: -0.0 is not +0.0, NaN positions must match
            ne = (x.view(np.uint32) != y.view(np.uint32)) & ~(np.isnan(x) & np.isnan(y))
            diff = int(ne.sum())
            if diff:
                i = np.unravel_index(int(np.argmax(ne)), ne.shape) if ne.ndim else ()
                diff = "%d (first at %s: %r vs %r)" % (diff, list(map(int, i)), float(x[i]), float(y[i]))
        else:
            diff = int((x != y).sum())
        bad += diff != 0
        nans = int(np.isnan(x).sum()) if x.dtype.kind == "f" else 0
        print("| %s | %s | %d | %s |" % (k, "x".join(map(str, x.shape)) or "scalar", nans, diff))
    print("%d arrays, %d differ (%s vs %s)" % (len(a.files) - 1, bad, a["library"], b["library"]))
    return 1 if bad else 0


def main(out_path):
    import torch
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd import arch
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    out = {"library": np.array(os.environ.get("LADDER_HIP_LIB", L.LIB_PATH))}
    rcs = {}
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    nan = lambda *shape: torch.full(shape, float("nan"), device="cuda")       # an element a call leaves unwritten stays NaN in both builds

    def call(tag, name, *args):
        rcs[tag] = L.query(name, *args)
        return rcs[tag]

    def keep(tag, t):
        out[tag] = t.cpu().numpy()

    def wsbuf(nbytes):
        return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device="cuda")

    def geometry(case):
        N, H, W, Cin, Cout, k, s, pad, act = case
        pt, Ho = arch.conv_out(H, k, s, pad)
        pl, Wo = arch.conv_out(W, k, s, pad)
        return (N, H, W, Cin, Ho, Wo, Cout, k, k, s, pt, pl)

    def operands(case, seed, scale_dy=1.0):
        N, H, W, Cin, Cout, k, s, pad, act = case
        g = geometry(case)
        rng = np.random.default_rng(seed)
        x = rng.standard_normal((N, H, W, Cin))
        x[..., 0] = -0.0
        w = rng.standard_normal((k, k, Cin, Cout)) / np.sqrt(k * k * Cin)
        b = rng.standard_normal(Cout)
        dy = rng.standard_normal((N, g[4], g[5], Cout)) * scale_dy
        return dev(x), dev(w), dev(b), dev(dy)

    # ---- strict-fp32 convolutions
    for ci, case in enumerate(CONV):
        N, H, W, Cin, Cout, k, s, pad, act = case
        g = geometry(case)
        Ho, Wo = g[4], g[5]
        t = "conv_" + "x".join(str(v) for v in case[:7])
        x, w, b, dy = operands(case, 100 + ci)
        M, K = N * Ho * Wo, k * k * Cin
        fws = wsbuf(L.query("ladder_igemm_fwd_workspace_bytes", M, K, Cout))
        out[t + "_ids"] = np.array([L.query("ladder_conv2d_fwd_kernel_id", N, H, W, Cin, Ho, Wo, Cout, k, k, s, 1, g[10], g[11]),
                                    L.query("ladder_conv2d_bwd_filter_kernel_id", *g), L.query("ladder_igemm_fwd_splits", M, K, Cout)], dtype=np.int64)
        for tag, (wp, wn) in (("ws", (p(fws), fws.numel())), ("nows", (None, 0))):
            y = nan(N, Ho, Wo, Cout)
            call(t + "_fwd_" + tag, "ladder_conv2d_fwd", p(x), p(w), p(b), p(y), *g, L.ACT[act], wp, wn, st)
            keep(t + "_y_" + tag, y)
        y = nan(N, Ho, Wo, Cout)
        call(t + "_fwd_nobias", "ladder_conv2d_fwd", p(x), p(w), None, p(y), *g, L.ACT[act], p(fws), fws.numel(), st)
        keep(t + "_y_nobias", y)
        wws = wsbuf(L.query("ladder_conv2d_bwd_filter_workspace_bytes", *g[:9]))
        for tag, dbq in (("db", True), ("nodb", False)):
            dw, db = nan(k, k, Cin, Cout), nan(Cout)
            call(t + "_wgrad_" + tag, "ladder_conv2d_bwd_filter", p(x), p(dy), p(dw), p(db) if dbq else None, *g, p(wws), wws.numel(), st)
            keep(t + "_dw_" + tag, dw)
            keep(t + "_db_" + tag, db)
        dw = nan(k, k, Cin, Cout)
        call(t + "_wgrad_nows", "ladder_conv2d_bwd_filter", p(x), p(dy), p(dw), None, *g, None, 0, st)
        keep(t + "_dw_nows", dw)
        wT = nan(w.numel())
        call(t + "_flip", "ladder_filter_flip_transpose", p(w), p(wT), k, k, Cin, Cout, st)
        keep(t + "_wT", wT)
        bws = wsbuf(L.query("ladder_igemm_fwd_workspace_bytes", N * H * W, k * k * Cout, Cin))
        for tag, (wp, wn) in (("ws", (p(bws), bws.numel())), ("nows", (None, 0))):
            for gt, gate in (("ungated", None), ("gated", x)):
                dx = nan(N, H, W, Cin)
                call("%s_bwd_data_%s_%s" % (t, gt, tag), "ladder_conv2d_bwd_data", p(dy), p(wT), p(dx), *g, p(gate), 1 if gate is not None else 0, wp, wn, st)
                keep("%s_dx_%s_%s" % (t, gt, tag), dx)
        if L.query("ladder_conv1x1_smallcout_eligible", M, Cin, Cout) and k == 1:
            sws = wsbuf(L.query("ladder_conv1x1_smallcout_bwd_workspace_bytes", M, Cin, Cout))
            for tag, dbq in (("db", True), ("nodb", False)):
                dx, dw, db, rec = nan(N, H, W, Cin), nan(Cin, Cout), nan(Cout), torch.full((L.ABSMAX_FLOATS,), -7.0, device="cuda")
                call(t + "_smallcout_bwd_" + tag, "ladder_conv1x1_smallcout_bwd", p(x), p(dy), p(w), p(dx), p(dw), p(db) if dbq else None, M, Cin, Cout, 1,
                     p(sws), sws.numel(), st)
                keep(t + "_smallcout_dx_" + tag, dx); keep(t + "_smallcout_dw_" + tag, dw); keep(t + "_smallcout_db_" + tag, db)
                for rt, rps in (("tensor", 0), ("samples", H * W)):
                    dx2 = nan(N, H, W, Cin)
                    call("%s_smallcout_bwd_absmax_%s_%s" % (t, rt, tag), "ladder_conv1x1_smallcout_bwd_absmax", p(x), p(dy), p(w), p(dx2), p(dw), p(db) if dbq else None,
                         M, Cin, Cout, 1, p(sws), sws.numel(), p(rec), rps, st)
                    keep("%s_smallcout_dx_absmax_%s_%s" % (t, rt, tag), dx2); keep("%s_smallcout_rec_%s_%s" % (t, rt, tag), rec)
                    keep("%s_smallcout_dw_absmax_%s_%s" % (t, rt, tag), dw)
            call(t + "_smallcout_bwd_nows", "ladder_conv1x1_smallcout_bwd", p(x), p(dy), p(w), p(dx), p(dw), p(db), M, Cin, Cout, 1, None, 0, st)
        del x, w, b, dy
        torch.cuda.empty_cache()

    # ---- the forward that also emits the batch-norm statistics of its output
    g = geometry(BNSTATS)
    N, H, W, Cin, Ho, Wo, Cout, k = g[:8]
    x, w, b, _ = operands(BNSTATS, 300)
    snb = L.query("ladder_conv2d_fwd_bnstats_workspace_bytes", *g)
    assert snb > 0, "the bnstats geometry must be eligible"
    sws = wsbuf(snb)
    y, s4 = nan(N, Ho, Wo, Cout), nan(6 * Cout)
    call("bnstats_fwd", "ladder_conv2d_fwd_bnstats", p(x), p(w), p(b), p(y), *g, L.ACT[BNSTATS[8]], p(s4), p(sws), sws.numel(), st)
    keep("bnstats_y", y); keep("bnstats_sums", s4)
    call("bnstats_fwd_nows", "ladder_conv2d_fwd_bnstats", p(x), p(w), p(b), p(y), *g, L.ACT[BNSTATS[8]], p(s4), None, 0, st)
    call("bnstats_fwd_nosums", "ladder_conv2d_fwd_bnstats", p(x), p(w), p(b), p(y), *g, L.ACT[BNSTATS[8]], None, p(sws), sws.numel(), st)
    del x, w, b, y
    torch.cuda.empty_cache()

    # ---- dense layers
    for di, (M, K, N, act) in enumerate(DENSE):
        t = "dense_%dx%dx%d" % (M, K, N)
        rng = np.random.default_rng(400 + di)
        x, w, b, dy = dev(rng.standard_normal((M, K))), dev(rng.standard_normal((K, N)) / np.sqrt(K)), dev(rng.standard_normal(N)), dev(rng.standard_normal((M, N)))
        fws = wsbuf(L.query("ladder_igemm_fwd_workspace_bytes", M, K, N))
        for tag, (wp, wn) in (("ws", (p(fws), fws.numel())), ("nows", (None, 0))):
            y = nan(M, N)
            call(t + "_fwd_" + tag, "ladder_dense_fwd", p(x), p(w), p(b), p(y), M, K, N, L.ACT[act], wp, wn, st)
            keep(t + "_y_" + tag, y)
        wws = wsbuf(L.query("ladder_dense_bwd_weight_workspace_bytes", M, K, N))
        for tag, dbq in (("db", True), ("nodb", False)):
            dw, db = nan(K, N), nan(N)
            call(t + "_wgrad_" + tag, "ladder_dense_bwd_weight", p(x), p(dy), p(dw), p(db) if dbq else None, M, K, N, p(wws), wws.numel(), st)
            keep(t + "_dw_" + tag, dw); keep(t + "_db_" + tag, db)
        call(t + "_wgrad_nows", "ladder_dense_bwd_weight", p(x), p(dy), p(dw), p(db), M, K, N, None, 0, st)
        wT = nan(w.numel())
        call(t + "_flip", "ladder_filter_flip_transpose", p(w), p(wT), 1, 1, K, N, st)
        bws = wsbuf(L.query("ladder_igemm_fwd_workspace_bytes", M, N, K))
        for tag, (wp, wn) in (("ws", (p(bws), bws.numel())), ("nows", (None, 0))):
            for gt, gate in (("ungated", None), ("gated", x)):
                dx = nan(M, K)
                call("%s_bwd_data_%s_%s" % (t, gt, tag), "ladder_dense_bwd_data", p(dy), p(wT), p(dx), M, K, N, p(gate), 2 if gate is not None else 0, wp, wn, st)
                keep("%s_dx_%s_%s" % (t, gt, tag), dx)

    # ---- the split-precision gather kernels
    for pn, P in PRECS.items():
        for gi, case in enumerate(GATHER):
            N, H, W, Cin, Cout, k, s, pad, act = case
            g = geometry(case)
            Ho, Wo = g[4], g[5]
            t = "split_%s_%s" % (pn, "x".join(str(v) for v in case[:7]))
            x, w, b, dy = operands(case, 500 + gi, 1e-3)
            recs = []
            for a in (x, dy):
                r = torch.empty(L.ABSMAX_FLOATS, device="cuda")
                L.call("ladder_absmax", p(a), a.numel(), p(r), st)
                buf = torch.empty(L.query("ladder_presplit_bytes", a.numel(), P), dtype=torch.uint8, device="cuda")
                L.call("ladder_presplit", p(a), p(r), p(buf), a.numel(), 0, P, st)
                recs += [r, buf]
            xa, xpl, da, dypl = recs
            keep(t + "_xplanes", xpl)
            out[t + "_eligible"] = np.array([L.query("ladder_conv2d_fwd_split_eligible", *g), L.query("ladder_conv2d_bwd_data_split_eligible", *g, 0),
                                            L.query("ladder_conv2d_bwd_data_split_eligible", *g, 1), L.query("ladder_conv2d_bwd_filter_split_eligible", *g)], dtype=np.int64)
            pk = torch.empty(L.query("ladder_filter_pack_split_bytes", k * k, Cin, Cout, P), dtype=torch.uint8, device="cuda")
            L.call("ladder_filter_pack_split", p(w), p(pk), k * k, Cin, Cout, 0, P, st)
            keep(t + "_pack", pk)
            fws = wsbuf(L.query("ladder_conv2d_fwd_split_workspace_bytes", *g))
            for tag, (wp, wn) in (("ws", (p(fws), fws.numel())), ("nows", (None, 0))):
                y = nan(N, Ho, Wo, Cout)
                call(t + "_fwd_" + tag, "ladder_conv2d_fwd_split", p(xpl), p(xa), p(pk), p(b), p(y), *g, L.ACT[act], P, wp, wn, st)
                keep(t + "_y_" + tag, y)
            snb = L.query("ladder_conv2d_fwd_split_bnstats_workspace_bytes", *g)
            sws, y, s4 = wsbuf(snb), nan(N, Ho, Wo, Cout), nan(6 * Cout)
            call(t + "_fwd_bnstats", "ladder_conv2d_fwd_split_bnstats", p(xpl), p(xa), p(pk), p(b), p(y), *g, L.ACT[act], P, p(s4), p(sws), sws.numel() if snb else 0, st)
            keep(t + "_y_bnstats", y); keep(t + "_sums_bnstats", s4)
            pkT = torch.empty(L.query("ladder_filter_pack_split_bytes", k * k, Cout, Cin, P), dtype=torch.uint8, device="cuda")
            L.call("ladder_filter_pack_split", p(w), p(pkT), k * k, Cout, Cin, 1, P, st)
            bws = wsbuf(L.query("ladder_conv2d_bwd_data_split_workspace_bytes", *g))
            for tag, (wp, wn) in (("ws", (p(bws), bws.numel())), ("nows", (None, 0))):
                for gt, gate in (("ungated", None), ("gated", x)):
                    dx = nan(N, H, W, Cin)
                    call("%s_bwd_data_%s_%s" % (t, gt, tag), "ladder_conv2d_bwd_data_split", p(dypl), p(da), p(pkT), p(dx), *g, p(gate), 1 if gate is not None else 0, P,
                         wp, wn, st)
                    keep("%s_dx_%s_%s" % (t, gt, tag), dx)
            wws = wsbuf(L.query("ladder_conv2d_bwd_filter_split_workspace_bytes", *g[:9]))
            for tag, dbq in (("db", True), ("nodb", False)):
                dw, db = nan(k, k, Cin, Cout), nan(Cout)
                call(t + "_wgrad_" + tag, "ladder_conv2d_bwd_filter_split", p(xpl), p(xa), p(dypl), p(da), p(dw), p(db) if dbq else None, *g, P, p(wws), wws.numel(), st)
                keep(t + "_dw_" + tag, dw); keep(t + "_db_" + tag, db)
            call(t + "_wgrad_nows", "ladder_conv2d_bwd_filter_split", p(xpl), p(xa), p(dypl), p(da), p(dw), p(db), *g, P, None, 0, st)
            call(t + "_fwd_noscale", "ladder_conv2d_fwd_split", p(xpl), None, p(pk), p(b), p(y), *g, L.ACT[act], P, p(fws), fws.numel(), st)
            del x, w, b, dy, xpl, dypl
            torch.cuda.empty_cache()

    # ---- the second stage alone
    for S in (1, 31, 32):
        n = 1000
        part = np.random.default_rng(600 + S).standard_normal((S, n))
        part[:, 1] = -0.0
        part, o = dev(part), nan(n)
        call("reduce_%d" % S, "ladder_reduce_splits", p(part), p(o), S, n, st)
        keep("reduce_%d_out" % S, o)
    call("reduce_0_splits", "ladder_reduce_splits", p(o), p(o), 0, 1000, st)
    call("reduce_0_n", "ladder_reduce_splits", p(o), p(o), 4, 0, st)

    # ---- rejected calls (tests/test_gpu_abi_errors.py::test_rejections_return_codes)
    x, w, b = torch.zeros(2, 8, 8, 16, device="cuda"), torch.zeros(3, 3, 16, 32, device="cuda"), torch.zeros(32, device="cuda")
    y, ws = torch.full((2, 8, 8, 32), 7.0, device="cuda"), wsbuf(1 << 20)
    conv = lambda tag, N, xp: call(tag, "ladder_conv2d_fwd", xp, p(w), p(b), p(y), N, 8, 8, 16, 8, 8, 32, 3, 3, 1, 1, 1, 0, p(ws), ws.numel(), st)
    assert conv("reject_conv_n0", 0, p(x)) == E_SHAPE and conv("reject_conv_negative", -3, p(x)) == E_SHAPE
    assert conv("reject_conv_misaligned", 2, p(x) + 4) == E_ALIGN
    keep("reject_conv_y_untouched", y)
    dw, db, dy = torch.empty_like(w), torch.empty_like(b), torch.zeros_like(y)
    assert call("reject_wgrad_nows", "ladder_conv2d_bwd_filter", p(x), p(dy), p(dw), p(db), 2, 8, 8, 16, 8, 8, 32, 3, 3, 1, 1, 1, None, 0, st) == E_WORKSPACE
    assert call("reject_dense_m0", "ladder_dense_fwd", p(x), p(w), p(b), p(y), 0, 16, 32, 0, None, 0, st) == E_SHAPE
    call("reject_dense_nt_small", "ladder_dense_fwd_nt", p(x), p(w), None, p(y), 128, 16, 32, 0, st)
    call("reject_dense_nt_noout", "ladder_dense_fwd_nt", p(x), p(w), None, None, 8192, 128, 1152, 0, st)
    call("reject_dense_noout", "ladder_dense_fwd", p(x), p(w), None, None, 8192, 128, 1152, 0, None, 0, st)
    for tag, a in (("4096", (4096, 128, 1152)), ("8192", (8192, 128, 1152)), ("1100", (8192, 128, 1100))):
        call("query_dense_fwd_is_persistent_" + tag, "ladder_dense_fwd_is_persistent", *a)
    call("query_dense_bwd_weight_is_persistent", "ladder_dense_bwd_weight_is_persistent", 8192, 96, 1152)

    torch.cuda.synchronize()
    names = sorted(rcs)
    out["rc_names"] = np.array(names)
    out["rc"] = np.array([rcs[k] for k in names], dtype=np.int64)
    np.savez(out_path, **out)
    print("wrote %d arrays to %s (library: %s); %d calls, %d rejected" % (len(out) - 1, out_path, out["library"], len(names), int((out["rc"] != 0).sum())))


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    main(sys.argv[1])
