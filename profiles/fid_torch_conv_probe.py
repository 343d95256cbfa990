"""Comparison probe, not a product path: the 13-layer VGG16 stack (3x3 / SAME / bias / ReLU, 2x2 max pools, global average) through
torch.nn.functional.conv2d in fp32 on the same GPU, at the shapes profiles/fid_throughput.py runs (64x64 inputs, chunk 128 / 512).

    python profiles/fid_torch_conv_probe.py [--chunk 128] [--iters 20]

Prints one JSON line: images per second of the stack alone (device time between two events, median over `iters` after warm-up), for the
channels-last memory format and the default one.  DESIGN.md quotes the ratio to the `stages` figure of fid_throughput.py.
"""
import argparse
import json
import statistics

import torch
import torch.nn.functional as F

BLOCKS = ((2, 64), (2, 128), (3, 256), (3, 512), (3, 512))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    g = torch.Generator(device="cuda").manual_seed(0)
    out = {}
    for fmt_name, fmt in (("channels_last", torch.channels_last), ("contiguous", torch.contiguous_format)):
        ws, cin = [], 3
        for n, c in BLOCKS:
            for _ in range(n):
                w = (torch.randn(c, cin, 3, 3, device="cuda", generator=g) * (2.0 / (9 * cin)) ** 0.5).contiguous(memory_format=fmt)
                ws.append((w, 0.05 * torch.randn(c, device="cuda", generator=g)))
                cin = c
        x = (torch.rand(a.chunk, 3, 64, 64, device="cuda", generator=g) * 2 - 1).contiguous(memory_format=fmt)

        def run():
            t, k = x, 0
            for n, _ in BLOCKS:
                for _ in range(n):
                    t = F.relu(F.conv2d(t, ws[k][0], ws[k][1], padding=1))
                    k += 1
                t = F.max_pool2d(t, 2, 2)
            return t.mean((2, 3))

        with torch.no_grad():
            for _ in range(3):
                run()
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.iters):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                run()
                e.record()
                e.synchronize()
                ms.append(s.elapsed_time(e))
        out[fmt_name] = dict(ms_median=round(statistics.median(ms), 3), ms_min=round(min(ms), 3), images_per_s=round(a.chunk / (statistics.median(ms) * 1e-3), 1))
    print(json.dumps(dict(probe="torch.nn.functional.conv2d fp32", chunk=a.chunk, iters=a.iters, **out)))


if __name__ == "__main__":
    main()
