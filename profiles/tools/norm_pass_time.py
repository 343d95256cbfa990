"""Device time of the batch-norm and instance-norm entry points (csrc/norm.hip) on the CelebA shapes of configs[2] at batch 128 (the shapes
of profiles/r06_f32_percall.md), strict fp32 (no absmax record): batch-norm forward statistics, forward apply, backward statistics, backward
apply; instance-norm forward with the factor-2 resize (the normalised tensor kept) and backward.

    python profiles/tools/norm_pass_time.py [--out profiles/norm_pass_time.json] [--lib [label=]other/libladder_hip.so ...] [--rounds 2] [--reps 100]

Every launch is timed by a pair of device events; after `--warmup` launches, the median of `--reps` launches (min and max are kept).  A
process loads one library, so every library is measured in a child process of its own; `--rounds 2` with one `--lib` runs other, tree,
other, tree -- the spread between a library's own runs is the noise floor of the session, against which a difference between two
libraries is to be read.  One JSON document; no GPU, no result.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if not any(os.path.isdir(os.path.join(p, "ladder_latent_data_distribution_modelling_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)

BN = [(524288, 128), (131072, 128), (32768, 256), (8192, 256), (2048, 512), (512, 512)]            # (rows, C)
IN = [(128, 64, 64, 128), (128, 16, 16, 256), (128, 2, 2, 512)]                                    # (N, H, W, C)
ACT = 1                                                                                            # leaky_relu


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        us.append(1e3 * a.elapsed_time(b))
    us.sort()
    return dict(us_median=round(statistics.median(us), 2), us_min=round(us[0], 2), us_max=round(us[-1], 2))


def child(reps, warmup):
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    g = torch.Generator(device="cuda").manual_seed(5)
    rand = lambda *s: torch.randn(*s, device="cuda", generator=g)
    entries = []

    def entry(name, shape, fn):
        fn()                                                                   # (L.call raises on a rejected call)
        entries.append(dict(entry=name, shape=list(shape), **timed(fn, reps, warmup)))
        print(json.dumps(entries[-1]), file=sys.stderr, flush=True)

    for rows, C in BN:
        x, dy, gm, be = rand(rows, C) * 1.7 + 0.6, rand(rows, C), 1 + 0.3 * rand(C), 0.2 * rand(C)
        y, dx, sums, mr, ds, dg, db = torch.empty_like(x), torch.empty_like(x), torch.empty(4 * C, device="cuda"), torch.empty(2 * C, device="cuda"), \
            torch.empty(2 * C, device="cuda"), torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        ws = torch.empty(L.query("ladder_bn_workspace_bytes", rows, C), dtype=torch.uint8, device="cuda")
        entry("bn_fwd_stats", (rows, C), lambda: L.call("ladder_bn_fwd_stats", p(x), p(sums), rows, C, p(ws), ws.numel(), st))
        entry("bn_fwd_apply", (rows, C), lambda: L.call("ladder_bn_fwd_apply", p(x), p(sums), float(rows), p(gm), p(be), p(y), p(mr), rows, C, 1e-3, ACT, st))
        entry("bn_bwd_stats", (rows, C), lambda: L.call("ladder_bn_bwd_stats", p(dy), p(x), p(mr), p(gm), p(be), p(ds), rows, C, ACT, p(ws), ws.numel(), st))
        entry("bn_bwd_apply", (rows, C), lambda: L.call("ladder_bn_bwd_apply", p(dy), p(x), p(mr), p(gm), p(be), p(ds), float(rows), p(dx), p(dg), p(db), rows, C, ACT, st))
        del x, dy, y, dx
    for N, H, W, C in IN:
        HW = H * W
        x, dy, sty = rand(N, HW, C) * 2 + 0.5, rand(N, HW, C), 0.5 * rand(N, 2 * C)
        up, lo, dx, mr, dst = torch.empty(N, 4 * HW, C, device="cuda"), torch.empty_like(x), torch.empty_like(x), torch.empty(N, 2 * C, device="cuda"), \
            torch.empty(N, 2 * C, device="cuda")
        ws = torch.empty(max(L.query("ladder_in_style_workspace_bytes", N, HW, C), 16), dtype=torch.uint8, device="cuda")
        entry("in_style_fwd_resize2x_keep", (N, H, W, C), lambda: L.call("ladder_in_style_fwd_resize2x_keep", p(x), p(sty), p(up), p(lo), p(mr), N, H, W, C, 1e-6, ACT,
                                                                        p(ws), ws.numel(), None, st))
        entry("in_style_bwd", (N, H, W, C), lambda: L.call("ladder_in_style_bwd", p(dy), p(x), p(sty), p(mr), p(dx), p(dst), N, HW, C, ACT, p(ws), ws.numel(), st))
        del x, dy, up, lo, dx
    print(json.dumps(dict(device_name=torch.cuda.get_device_name(0), entries=entries)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "norm_pass_time.json"))
    ap.add_argument("--lib", nargs="*", default=[], help="[label=]path of further libladder_hip.so files to time, each in a child process")
    ap.add_argument("--rounds", type=int, default=2, help="how often the list of libraries is gone through")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        if not torch.cuda.is_available():
            sys.exit("norm_pass_time.py measures on the GPU: none found")
        child(a.reps, a.warmup)
        return
    libs = [tuple(s.split("=", 1)) if "=" in s else (s, s) for s in a.lib] + [("this tree", None)]
    runs = []
    for rnd in range(a.rounds):
        for label, path in libs:
            env = dict(os.environ) if path is None else dict(os.environ, LADDER_HIP_LIB=os.path.abspath(path))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--reps", str(a.reps), "--warmup", str(a.warmup)], env=env,
                               stdout=subprocess.PIPE, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit("the measurement of %s failed (exit %d): nothing further is run" % (label, r.returncode))
            runs.append(dict(library=label, round=rnd, **json.loads(r.stdout.strip().splitlines()[-1])))
    # per entry and library: the worse (larger) of its medians, and the spread of its medians
    summary = []
    for i, e in enumerate(runs[0]["entries"]):
        row = dict(entry=e["entry"], shape=e["shape"])
        for label, _ in libs:
            med = [r["entries"][i]["us_median"] for r in runs if r["library"] == label]
            row[label] = dict(us_median_worse=max(med), us_median_spread=round(max(med) - min(med), 2))
        summary.append(row)
        print(json.dumps(row), flush=True)
    doc = dict(what="batch-norm / instance-norm entry points: device-event time per call in microseconds, median of %d launches after %d warm-up launches, "
                    "%d alternating rounds per library" % (a.reps, a.warmup, a.rounds), act="leaky_relu", reps=a.reps, warmup=a.warmup, summary=summary, runs=runs)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
