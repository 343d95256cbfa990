"""Throughput of the FID evaluation ("FID evaluation on the device"): images per second of fid_from_arrays on two synthetic
10 000-image 128x128x3 sets (one uint8, one float), and where the device time goes.

    python profiles/fid_throughput.py --mode rate   [--n 10000] [--chunk 128] [--reps 3]     # images per second, end to end (host arrays in, score out)
    python profiles/fid_throughput.py --mode stages [--n 2048]  [--chunk 128]                # per-stage device time (HIP events around every stage)

The conventions are those of profiles/generate_throughput.py: one warm-up pass, then `reps` timed passes, one JSON line per process; the rows of
profiles/fid_throughput.json come from two processes per cell.  The weights are seeded random numbers (He-normal): the arithmetic does not depend on them.
`--mode stages` installs the existing profiler (profiler.KernelProfiler as layers.PROF): every stage is bracketed with HIP events under its name and the
convolution launches are attributed to their kernel ids as in bench.py; its total is the device time of the stages, not the wall time.
The fp32 MFMA peak the convolution rate is compared with is the measured v_mfma_f32_32x32x2_f32 rate of profiles/mfma_rate.hip.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(p, "ladder_latent_data_distribution_modelling_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("rate", "stages"), required=True)
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--pooling", default="avg")
    a = ap.parse_args()
    from ladder_latent_data_distribution_modelling_amd import fid as F
    from ladder_latent_data_distribution_modelling_amd.layers import Ctx
    rng = np.random.default_rng(1)
    real = rng.integers(0, 256, (a.n, 128, 128, 3), dtype=np.uint8)
    gen = rng.random((a.n, 128, 128, 3), dtype=np.float32) * 1.5 - 0.2
    feats = F.VGG16Features(Ctx("cuda:0"), F.random_weights(), F.check_pooling(a.pooling))
    F.fid_from_arrays(real[:2 * a.chunk], gen[:2 * a.chunk], feats, chunk=a.chunk)          # warm-up: allocator, workspace, pinned buffers
    torch.cuda.synchronize()
    if a.mode == "rate":
        secs = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            score = F.fid_from_arrays(real, gen, feats, chunk=a.chunk)
            torch.cuda.synchronize()
            secs.append(time.perf_counter() - t0)
        rate = sorted(2 * a.n / s for s in secs)
        print(json.dumps(dict(mode="rate", n_per_set=a.n, chunk=a.chunk, pooling=a.pooling, reps=a.reps, score=score, images_per_s_median=round(statistics.median(rate), 1),
                              images_per_s_min=round(rate[0], 1), images_per_s_max=round(rate[-1], 1), seconds=[round(s, 4) for s in secs])))
        return
    from ladder_latent_data_distribution_modelling_amd import layers
    from ladder_latent_data_distribution_modelling_amd.profiler import KernelProfiler
    layers.PROF = prof = KernelProfiler()                    # stages under their names (fid._stage), convolution launches under their kernel ids (layers._timed)
    F.fid_from_arrays(real, gen, feats, chunk=a.chunk)
    summ = prof.summary()
    layers.PROF = None
    stages = {k: dict(launches=v["launches"], total_ms=round(v["total_ms"], 3), tflops=round(v["tflops"], 2) if v["flops_per_launch"] else None)
              for k, v in summ.items() if isinstance(k, str)}
    kernels = {str(k): dict(kernel=v["kernel"][:60], launches=v["launches"], total_ms=round(v["total_ms"], 3), tflops=round(v["tflops"], 2))
               for k, v in summ.items() if not isinstance(k, str)}
    total = sum(r["total_ms"] for r in stages.values())
    conv_ms = sum(r["total_ms"] for k, r in stages.items() if k.startswith("block"))
    conv_fl = sum(v["flops_per_launch"] * v["launches"] for k, v in summ.items() if isinstance(k, str) and k.startswith("block"))
    small = total - conv_ms
    print(json.dumps(dict(mode="stages", n_per_set=a.n, chunk=a.chunk, pooling=a.pooling, device_ms_total=round(total, 2), conv_ms=round(conv_ms, 2),
                          conv_tflops=round(conv_fl / (conv_ms * 1e-3) / 1e12, 2), small_kernels_ms=round(small, 3),
                          small_kernels_share=round(small / total, 4), images_per_s_device=round(2 * a.n / (total * 1e-3), 1), stages=stages, kernels=kernels)))


if __name__ == "__main__":
    main()
