"""Time of batched shortest-likely-path interpolation on a wide representation ("Batched SLP interpolation": wide representations):
SLPInterpolator.optimise_batch (csrc/slp_wide.hip, one launch runs the whole loop) against what the code offered before it for R > 8, the
host loop SLPInterpolator.optimise, one path at a time.

    python profiles/tools/slp_wide_time.py [--out profiles/slp_wide_time.json] [--reps 5] [--host-paths 2]

batch: (K, R, n_step) = (30, 16, 5) and (30, 64, 5), P = 1, 64, 1024 pairs, 500 iterations, record=True; HIP events around optimise_batch
(the upload of the end points, the launch, the one copy back), one warm-up, median of `reps`.
host loop: the same mixture and the first `host-paths` pairs, 500 iterations each, WALL time per path (the loop synchronises every iteration),
median over the paths after one warm-up path; the P-path figure is that time SCALED by P and labelled so -- the loop has no batched form.
one workgroup: P = 1 at (30, 64, 5) and (30, 64, 32), microseconds per iteration, beside the two bounds the design implies -- reading
2 K R^2 floats once per iteration at the rate one CU draws from its XCD's L2, and 4 n_pad K R^2 fp32 MFMA flops on one CU's four SIMDs.
One JSON document.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if not any(os.path.isdir(os.path.join(p, "ladder_latent_data_distribution_modelling_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)

K, N_ITER = 30, 500
L2_GBPS_PER_CU = 70.0            # one CU reading rows every workgroup shares from its XCD's L2 (measured 66-73 GB/s)
MFMA_FLOP_PER_CLK_CU, CLOCK_GHZ = 256.0, 2.4    # v_mfma_f32_16x16x4_f32: 64 flop / clk / SIMD, four SIMDs


def _events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def _med(secs):
    return dict(seconds_median=round(statistics.median(secs), 6), seconds_min=round(min(secs), 6), seconds_max=round(max(secs), 6))


def _case(R, P, n_step, seed=3):
    rng = np.random.default_rng(seed)
    starts, ends = rng.normal(0, 1.5, (P, R)), rng.normal(0, 1.5, (P, R))
    return starts.astype(np.float32).astype(np.float64), ends.astype(np.float32).astype(np.float64)


def batch_time(slp, R, P, n_step, reps):
    starts, ends = _case(R, P, n_step)
    secs = []
    for r in range(1 + reps):
        s = _events(lambda: slp.optimise_batch(starts, ends, n_step=n_step, n_iter=N_ITER, record=True))
        if r:
            secs.append(s)
    return _med(secs)


def host_time(slp, R, n_step, paths):
    starts, ends = _case(R, 1 + paths, n_step)
    secs = []
    for i in range(1 + paths):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        slp.optimise(starts[i], ends[i], n_step=n_step, n_iter=N_ITER)
        if i:
            secs.append(time.perf_counter() - t0)
    return _med(secs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slp_wide_time.json"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-paths", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("slp_wide_time.py measures on the GPU: none found")
    from oracle import ladder_oracle as O
    from ladder_latent_data_distribution_modelling_amd.codes.interpolation import SLPInterpolator
    from ladder_latent_data_distribution_modelling_amd.engine import Ctx
    ctx = Ctx("cuda:0")
    rows, single = [], []
    for R in (16, 64):
        gm = O.synthetic_gm(dict(n_mixtures=K, representation_size=R), np.random.default_rng(K * 7 + R))
        slp = SLPInterpolator(types.SimpleNamespace(ctx=ctx), *(gm[k].astype(np.float32) for k in ("weights", "means", "covs")))
        host = host_time(slp, R, 5, a.host_paths) if a.host_paths else None
        for P in (1, 64, 1024):
            row = dict(K=K, R=R, n_step=5, P=P, n_iter=N_ITER, batch=batch_time(slp, R, P, 5, a.reps))
            if host is not None:
                row["host_loop_one_path_wall"] = host
                row["host_loop_scaled_to_P_seconds"] = round(host["seconds_median"] * P, 4)
                row["scaled_host_over_batch"] = round(host["seconds_median"] * P / row["batch"]["seconds_median"], 1)
            rows.append(row)
            print(json.dumps(row), flush=True)
        if R == 64:
            for n_step in (5, 32):
                t = batch_time(slp, R, 1, n_step, a.reps)
                n_pad = 16 * ((n_step + 15) // 16)
                single.append(dict(K=K, R=R, n_step=n_step, P=1, us_per_iteration=round(1e6 * t["seconds_median"] / N_ITER, 2),
                                   bound_l2_read_us=round(2 * K * R * R * 4 / (L2_GBPS_PER_CU * 1e3), 2),
                                   bound_mfma_us=round(4 * n_pad * K * R * R / (MFMA_FLOP_PER_CLK_CU * CLOCK_GHZ * 1e3), 2)))
                print(json.dumps(single[-1]), flush=True)
    doc = dict(what="batched SLP interpolation on a wide representation: optimise_batch (HIP events, one warm-up, median of %d) against the host loop "
                    "optimise (wall time per path, scaled to P), %d iterations, record=True" % (a.reps, N_ITER),
               K=K, n_iter=N_ITER, reps=a.reps, host_paths=a.host_paths, device_name=torch.cuda.get_device_name(0),
               bounds=dict(l2_gbps_per_cu=L2_GBPS_PER_CU, mfma_flop_per_clk_cu=MFMA_FLOP_PER_CLK_CU, clock_ghz=CLOCK_GHZ),
               rows=rows, one_workgroup=single)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
