"""Throughput of bulk generation: images per second of LadderEngine.generate against the loop a user had to write
before it existed, and the achieved bandwidth of ladder_images_to_u8 beside a device-to-device copy of the same byte count.

    python profiles/generate_throughput.py --mode new      [--n 8192] [--chunk 128] [--uint8] [--reps 5] [--method ours]
    python profiles/generate_throughput.py --mode baseline ...      # host-numpy sampling + eng.decode(code).cpu().numpy() per chunk
    python profiles/generate_throughput.py --mode u8bw

`--mode baseline` uses nothing newer than LadderEngine.decode / decode_representation, so the SAME script measures an older checkout when
PYTHONPATH points at it: the baseline rows of profiles/generate_throughput.json were taken that way on a checkout of the commit before
generation existed, alternating with the new path in one session on one box (3 timed passes per process, two processes per cell).
`--method standard_gaussian` (new path only) leaves the inner decoder out; profiles/generate_breakdown.py uses a kernel trace of it to tell the inner decoder's launches from the decoder's.
Workload: codes/celeba_config.json, prior "ours", the reference's fitted mixture (tests/golden/GM_prior_info.npz, *_full).
One warm-up pass, then `reps` timed passes; prints one JSON line with the median and the spread.
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
    ap.add_argument("--mode", choices=("new", "baseline", "u8bw"), required=True)
    ap.add_argument("--n", type=int, default=8192)
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--uint8", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--method", choices=("ours", "standard_gaussian"), default="ours")
    a = ap.parse_args()
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.engine import LadderEngine
    if a.mode == "u8bw":
        return u8_bandwidth(L, a.reps)
    cfg = json.load(open(os.path.join(ROOT, "codes", "celeba_config.json")))
    eng = LadderEngine(cfg, "cuda:0", seed=1)
    fix = np.load(os.path.join(ROOT, "tests", "golden", "GM_prior_info.npz"))
    w, m, K = (np.asarray(fix[k], np.float64) for k in ("w_full", "m_full", "K_full"))
    shape = (int(cfg["dim_input_x"]), int(cfg["dim_input_y"]), int(cfg["dim_input_channel"]))

    if a.mode == "new":
        sampler = eng.prior_sampler(a.method, (w, m, K) if a.method == "ours" else None, seed=1)

        def run():
            return eng.generate(a.n, sampler, chunk=a.chunk, as_uint8=a.uint8)
    else:
        chol, p = np.linalg.cholesky(K), np.clip(w, 0, None) / np.clip(w, 0, None).sum()

        def run():
            rng = np.random.default_rng(1)
            out = np.empty((a.n,) + shape, np.uint8 if a.uint8 else np.float32)
            for lo in range(0, a.n, a.chunk):
                b = min(a.chunk, a.n - lo)
                comp = rng.choice(len(p), size=b, p=p)
                t = m[comp] + np.einsum("nij,nj->ni", chol[comp], rng.standard_normal((b, m.shape[1])))
                img = eng.decode(eng.decode_representation(t)).cpu().numpy()
                out[lo:lo + b] = np.rint(np.clip(img, 0, 1) * np.float32(255)).astype(np.uint8) if a.uint8 else img
            return out

    run()                                                    # warm-up: allocator, workspace, filter banks, pinned buffers
    torch.cuda.synchronize()
    secs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        imgs = run()
        torch.cuda.synchronize()
        secs.append(time.perf_counter() - t0)
    assert imgs.shape == (a.n,) + shape and np.isfinite(imgs.astype(np.float32)).all()
    rate = sorted(a.n / s for s in secs)
    print(json.dumps(dict(mode=a.mode, method=a.method, n=a.n, chunk=a.chunk, dtype=str(imgs.dtype), reps=a.reps, images_per_s_median=round(statistics.median(rate), 1),
                          images_per_s_min=round(rate[0], 1), images_per_s_max=round(rate[-1], 1), seconds=[round(s, 4) for s in secs],
                          lib=L.LIB_PATH if "LADDER_HIP_LIB" not in os.environ else os.environ["LADDER_HIP_LIB"])))


def u8_bandwidth(L, reps):
    n = 1024 * 128 * 128 * 3                                  # 1024 CelebA images: 201 MB read + 50 MB written
    x = torch.rand(n, device="cuda") * 1.2 - 0.1
    out = torch.empty(n, dtype=torch.uint8, device="cuda")
    nbytes = 5 * n
    src, dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")   # copy: same bytes moved
    st = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        for _ in range(3):
            fn()
        ms = []
        for _ in range(max(reps, 5) * 4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return sorted(ms)

    pack = timed(lambda: L.call("ladder_images_to_u8", x.data_ptr(), out.data_ptr(), n, st))
    copy = timed(lambda: dst.copy_(src))
    gbs = lambda ms: round(nbytes / (ms * 1e-3) / 1e9, 1)
    print(json.dumps(dict(mode="u8bw", pixels=n, bytes_moved=nbytes, pack_us_median=round(statistics.median(pack) * 1e3, 1),
                          pack_GBps_median=gbs(statistics.median(pack)), pack_GBps_min=gbs(pack[-1]), pack_GBps_max=gbs(pack[0]),
                          copy_us_median=round(statistics.median(copy) * 1e3, 1), copy_GBps_median=gbs(statistics.median(copy)),
                          copy_GBps_min=gbs(copy[-1]), copy_GBps_max=gbs(copy[0]))))


if __name__ == "__main__":
    main()
