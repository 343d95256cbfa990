"""Records tests/golden/conv_host_queries.json: the return value of every pure-host export of the implicit-GEMM convolution files (tile, split-K
and workspace planning, kernel ids, eligibility) over a fixed list of geometries, with and without LADDER_DISABLE_HALO=1.  No device is needed.
tests/test_conv_host_queries_cpu.py holds the library to it, so the file pins the planning: record it from the commit BEFORE a change to that
planning, `python tests/golden/make_conv_host_queries.py [OUT.json]`, and let the test compare the commit after it.

The geometries: CONV_CASES of tests/test_gpu_kernels.py, GATHER_CASES of tests/test_gpu_split.py, every layer of tests/golden/conv_routes.json
at its recorded input shape, and degenerate ones (a zero or negative extent, more than 28 taps, odd maps under stride 2)."""
import ast
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l
DEGENERATE = [
    (0, 8, 8, 16, 8, 8, 32, 3, 3, 1, 1, 1), (2, -1, 8, 16, 8, 8, 32, 3, 3, 1, 1, 1), (2, 8, 8, 16, 0, 8, 32, 3, 3, 1, 1, 1),
    (2, 8, 8, 16, 8, 8, 32, 3, 0, 1, 1, 1), (2, 8, 8, 16, 8, 8, 32, 3, 3, 0, 1, 1), (2, 8, 8, -16, 8, 8, 32, 3, 3, 1, 1, 1),
    (4, 16, 16, 32, 16, 16, 128, 6, 6, 1, 2, 2), (64, 16, 16, 128, 8, 8, 128, 6, 6, 2, 2, 2), (128, 16, 16, 128, 16, 16, 256, 5, 6, 1, 2, 2),
    (32, 9, 7, 128, 5, 4, 128, 3, 3, 2, 1, 1), (256, 1, 5, 128, 1, 3, 128, 3, 3, 2, 1, 1), (512, 1, 1, 128, 1, 1, 128, 3, 3, 2, 1, 1),
    (128, 5, 1, 128, 3, 1, 256, 3, 3, 2, 1, 1), (64, 15, 15, 256, 8, 8, 256, 3, 3, 2, 1, 1), (96, 7, 7, 128, 4, 4, 128, 1, 1, 2, 0, 0),
]


def _literal(path, name):
    """the list a test module assigns to `name`, without importing the module (it needs a device)"""
    for node in ast.parse(open(path).read()).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == name:
            return ast.literal_eval(node.value)
    raise KeyError(name)


def _geo(N, H, W, Cin, Cout, k, s, pad):
    from ladder_latent_data_distribution_modelling_amd import arch
    pt, Ho = arch.conv_out(H, k, s, pad)
    pl, Wo = arch.conv_out(W, k, s, pad)
    return (N, H, W, Cin, Ho, Wo, Cout, k, k, s, pt, pl)


def geometries():
    from ladder_latent_data_distribution_modelling_amd import engine, layers
    geos = [_geo(*c[:8]) for c in _literal(os.path.join(ROOT, "tests", "test_gpu_kernels.py"), "CONV_CASES")]
    geos += [_geo(*c[:8]) for c in _literal(os.path.join(ROOT, "tests", "test_gpu_split.py"), "GATHER_CASES")]
    routes = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_routes.json")))
    for key in sorted(routes):
        name = key.split("/")[0]
        cfg = json.load(open(os.path.join(ROOT, "codes", "%s_config.json" % name)))
        ctx = types.SimpleNamespace(ns=layers.PRECISIONS["f32"], up2=4, keep_activations=True)
        enc = engine.Encoder(ctx, None, cfg)
        dec = (engine.CelebADecoder if name == "celeba" else engine.MnistDecoder)(ctx, None, cfg)
        convs = enc.convs + ([dec.conv0] + [b[0] for b in dec.blocks] + [dec.conv_out] if name == "celeba" else dec.convs)
        convs = {c.name: c for c in convs}
        for rec in routes[key]["records"]:
            c, (N, H, W, Cin) = convs[rec["layer"]], rec["in_shape"]
            assert Cin == c.cin, rec
            geos.append(_geo(N, H, W, Cin, c.cout, c.k, c.stride, c.padding))
    return sorted(set(geos)) + DEGENERATE


def queries(L, g):
    """[(label, value)] of every host query for one geometry"""
    N, H, W, Cin, Ho, Wo, Cout, KH, KW, s, pt, pl = g
    out = []

    def q(name, *a, tag=""):
        out.append((name[len("ladder_"):] + tag, int(L.query(name, *a))))

    q("ladder_conv2d_fwd_kernel_id", N, H, W, Cin, Ho, Wo, Cout, KH, KW, s, 1, pt, pl)
    q("ladder_conv2d_fwd_kernel_id", N, Ho, Wo, Cout, H, W, Cin, KH, KW, 1, s, KH - 1 - pt, KW - 1 - pl, tag=":bwd_data")
    q("ladder_conv2d_fwd_bnstats_workspace_bytes", *g)
    q("ladder_conv2d_fwd_split_eligible", *g)
    q("ladder_conv2d_fwd_split_workspace_bytes", *g)
    q("ladder_conv2d_fwd_split_bnstats_workspace_bytes", *g)
    q("ladder_conv2d_bwd_data_split_eligible", *g, 0, tag=":ungated")
    q("ladder_conv2d_bwd_data_split_eligible", *g, 1, tag=":gated")
    q("ladder_conv2d_bwd_data_split_workspace_bytes", *g)
    q("ladder_conv2d_bwd_filter_split_eligible", *g)
    if min(N, H, W, Cin, Ho, Wo, Cout, KH, KW, s) <= 0:          # the unguarded planners divide by these extents
        return out
    M, K, Mb, Kb = N * Ho * Wo, KH * KW * Cin, N * H * W, KH * KW * Cout
    for tag, (m, k, ci, co) in (("", (M, K, Cin, Cout)), (":bwd_data", (Mb, Kb, Cout, Cin))):
        q("ladder_igemm_fwd_tile", m, ci, co, tag=tag)
        q("ladder_igemm_fwd_splits", m, k, co, tag=tag)
        q("ladder_igemm_fwd_workspace_bytes", m, k, co, tag=tag)
        q("ladder_dense_fwd_is_persistent", m, k, co, tag=tag)
    q("ladder_conv2d_bwd_filter_kernel_id", *g)
    q("ladder_conv2d_bwd_filter_workspace_bytes", *g[:9])
    q("ladder_conv2d_bwd_filter_split_workspace_bytes", *g[:9])
    q("ladder_dense_bwd_weight_is_persistent", M, K, Cout)
    q("ladder_dense_bwd_weight_workspace_bytes", M, K, Cout)
    q("ladder_conv1x1_smallcout_eligible", M, Cin, Cout)
    if Cin >= 4:
        q("ladder_conv1x1_smallcout_bwd_workspace_bytes", M, Cin, Cout)
    return out


def record(lib_path=None):
    """{"queries": [labels], "answers": {geometry: [answers, answers under LADDER_DISABLE_HALO=1 or None where they are the same]}} from the library at
    lib_path (default: the tree's own build).  A geometry's answers follow the order of the labels; a degenerate geometry has only the first ones."""
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    L.load(lib_path)
    saved = os.environ.pop("LADDER_DISABLE_HALO", None)
    try:
        geos, labels, legs = geometries(), [], []
        for leg in ("halo", "nohalo"):
            if leg == "nohalo":
                os.environ["LADDER_DISABLE_HALO"] = "1"
            got = [queries(L, g) for g in geos]
            for one in got:
                names = [n for n, _ in one]
                assert names == labels[:len(names)] or labels == names[:len(labels)], (names, labels)
                labels = max(labels, names, key=len)
            legs.append([[v for _, v in one] for one in got])
        result = dict(queries=labels, answers={",".join(map(str, g)): [a, None if a == b else b] for g, a, b in zip(geos, *legs)})
    finally:
        os.environ.pop("LADDER_DISABLE_HALO", None)
        if saved is not None:
            os.environ["LADDER_DISABLE_HALO"] = saved
    return result


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "conv_host_queries.json")
    with open(out, "w") as f:
        json.dump(record(os.environ.get("LADDER_HIP_LIB")), f, separators=(",", ":"), sort_keys=True, indent=None)
        f.write("\n")
    print("wrote", out)
