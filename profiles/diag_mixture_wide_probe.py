"""Time of the VampPrior term on a wide code ("The VampPrior term on a wide code"; csrc/diag_mixture.hip).

    python profiles/diag_mixture_wide_probe.py [--out profiles/diag_mixture_wide_probe.json] [--reps 30] [--kernel-db results.db]
    rocprofv3 --kernel-trace --stats -d DIR -- python profiles/diag_mixture_wide_probe.py --trace       (a run of its own: only leg (a), 30 calls)

One process, HIP events around single calls, 5 warm-up calls per leg, then `reps` rounds that alternate the legs, all at L = 100, B = 128, K = 50:
  (a) ladder_diag_mixture_wide_fwd_bwd at Z = 256                              -- the new entry
  (b) ladder_diag_mixture_fwd_bwd at Z = 64                                    -- the narrow entry: the per-element yardstick
  (c) ladder_gmm_wide_logprob_fwd_bwd at Z = 256 with diagonal covariances     -- the only way to this term at this width before (a), without
                                                                                  component gradients
Per leg: min and median, and the leg's spread against itself = |median of the even rounds - median of the odd rounds| / median.
Conditions: median (a) <= 4 x median (b) x (1 + spread of (b)), 4 being the ratio of the widths; median (a) < median (c).  The exit status is 1 if
one fails.  With --kernel-db (the rocpd database of a --trace run) the per-launch times are folded in: the bytes and operations each launch needs,
computed from the shapes below, over its kernel time, beside the time its bound allows (157.3 TFLOP/s fp32 vector, 6.3 TB/s achievable HBM).
"""
import argparse
import json
import os
import sqlite3
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if not any(os.path.isdir(os.path.join(p, "ladder_latent_data_distribution_modelling_amd")) for p in sys.path if p):
    sys.path.insert(0, ROOT)

L_, B, K = 100, 128, 50
PEAK_FLOPS, PEAK_BYTES = 157.3e12, 6.3e12


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a, np.float32)).cuda()


def p(t):
    return None if t is None else t.data_ptr()


def inputs(Z):
    """the clustered set of tests/test_gpu_diag_mixture_wide.py: every responsibility is non-zero, nothing a kernel could skip"""
    rng = np.random.default_rng(K + Z)
    base = rng.standard_normal(Z)
    cm = base + 0.05 * rng.standard_normal((K, Z))
    cs = 0.8 * (1 + 0.02 * rng.standard_normal((K, Z)))
    mu = base + 0.3 * rng.standard_normal((B, Z))
    sd = 0.1 + rng.random((B, Z))
    eps = rng.standard_normal((L_, B, Z))
    return mu, sd, eps, cm, cs


def launch_model(Z):
    """bytes and floating-point operations each launch of (a) needs, from the shapes (csrc/diag_mixture.hip: DW_KC = 16, 256 slices)"""
    S, Kp, nkc, slices = L_ * B, (K + 15) // 16 * 16, (K + 15) // 16, 256
    lsplit = slices // B
    return {
        # sub, mul, fma per (sample, component, dimension); reads eps, writes r (its re-reads stay in cache)
        "dw_resp_kernel": dict(flop=4.0 * S * K * Z, bytes=4.0 * (S * Z + S * Kp + 2 * K * Z)),
        # sub, 2 mul, add, 3 fma; reads eps (once per chunk of components from L2 / Infinity Cache: counted once) and r, writes the partials
        "dw_accum_kernel": dict(flop=10.0 * S * K * Z, bytes=4.0 * (S * Z + S * Kp + 2 * slices * K * Z + 2 * nkc * lsplit * B * Z)),
        # both reduce launches: [slices, 2, K, Z] -> dcomp_*, [chunks * l-ranges, 2, B, Z] -> dmu, dsd
        "dw_reduce_kernel": dict(flop=2.0 * (slices * K * Z + nkc * lsplit * B * Z), bytes=4.0 * (2 * (slices + 1) * K * Z + 2 * (nkc * lsplit + 1) * B * Z),
                                 launches=2),
        "dw_prepare_kernel": dict(flop=3.0 * K * Z, bytes=16.0 * K * Z),
        "sum_doubles_kernel": dict(flop=S / 16.0, bytes=8.0 * S / 16),
    }


def kernel_times(db_path):
    """-> {kernel: (calls, average microseconds)} of the dw_* kernels in a rocprofv3 (rocpd SQLite) kernel trace"""
    db = sqlite3.connect(db_path)
    out = {}
    for name, calls, avg in db.execute("select name, count(*), avg(duration) from kernels group by name"):
        for short in ("dw_resp_kernel", "dw_accum_kernel", "dw_reduce_kernel", "dw_prepare_kernel", "sum_doubles_kernel"):
            if short in name:
                out[short] = (calls, avg / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diag_mixture_wide_probe.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--trace", action="store_true", help="only 30 calls of leg (a): the run to put under rocprofv3 --kernel-trace")
    ap.add_argument("--kernel-db", default="", help="rocpd database of a --trace run: per-launch times, achieved rates and bounds go into the document")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("diag_mixture_wide_probe.py measures on the GPU: none found")
    if a.reps < 20:
        sys.exit("at least 20 repeats per leg")
    from ladder_latent_data_distribution_modelling_amd import _lib as L
    from ladder_latent_data_distribution_modelling_amd.engine import Ctx
    st = Ctx("cuda:0").stream

    def diag_leg(Z, query, entry, wide):
        arrs = [dev(v) for v in inputs(Z)]
        out, dmu, dsd, dcm, dcs = (torch.empty(n, device="cuda") for n in (1, B * Z, B * Z, K * Z, K * Z))
        ws = torch.empty(L.query(query, L_, B, Z, K) if wide else L.query(query, B, Z, K), dtype=torch.uint8, device="cuda")
        call = lambda: L.call(entry, *(p(t) for t in arrs), L_, B, Z, K, p(out), p(dmu), p(dsd), p(dcm), p(dcs), p(ws), ws.numel(), st)
        return call, out, (arrs, dmu, dsd, dcm, dcs, ws)

    leg_a, out_a, keep_a = diag_leg(256, "ladder_diag_mixture_wide_workspace_bytes", "ladder_diag_mixture_wide_fwd_bwd", True)
    if a.trace:
        for _ in range(30):
            leg_a()
        torch.cuda.synchronize()
        print("sum_logp", out_a.item())
        return
    leg_b, out_b, keep_b = diag_leg(64, "ladder_diag_mixture_workspace_bytes", "ladder_diag_mixture_fwd_bwd", False)
    Z = 256
    mu, sd, eps, cm, cs = inputs(Z)
    covs = np.zeros((K, Z, Z), np.float32)
    covs[:, np.arange(Z), np.arange(Z)] = cs.astype(np.float32) ** 2
    params = torch.zeros(L.query("ladder_gmm_wide_param_bytes", K, Z), dtype=torch.uint8, device="cuda")
    pws = torch.empty(L.query("ladder_gmm_wide_prepare_workspace_bytes", K, Z), dtype=torch.uint8, device="cuda")
    wd, md, cd = dev(np.full(K, 1.0 / K)), dev(cm), dev(covs)
    L.call("ladder_gmm_wide_prepare", p(wd), p(md), p(cd), K, Z, p(params), p(pws), pws.numel(), st)
    assert int(params[:4].view(torch.int32).item()) == -1
    mud, sdd, epsd = dev(mu), dev(sd), dev(eps)
    out_c, dmu_c, dsd_c = torch.empty(1, device="cuda"), torch.empty(B, Z, device="cuda"), torch.empty(B, Z, device="cuda")
    ws_c = torch.empty(L.query("ladder_gmm_wide_workspace_bytes", L_, B, Z, K), dtype=torch.uint8, device="cuda")
    leg_c = lambda: L.call("ladder_gmm_wide_logprob_fwd_bwd", p(mud), p(sdd), p(epsd), p(params), L_, B, Z, K, p(out_c), p(dmu_c), p(dsd_c), p(ws_c),
                           ws_c.numel(), st)
    legs = {"a": leg_a, "b": leg_b, "c": leg_c}
    for fn in legs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(a.reps):
        for k, fn in legs.items():                   # a, b, c, a, b, c, ...
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            us[k].append(e0.elapsed_time(e1) * 1e3)
    assert abs(out_a.item() - out_c.item()) < 6e-5 * abs(out_c.item()) + 2e-3, (out_a.item(), out_c.item())   # (a) and (c) compute the same term

    def stats(v):
        med = statistics.median(v)
        return dict(us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                    self_spread=round(abs(statistics.median(v[0::2]) - statistics.median(v[1::2])) / med, 4))

    res = {k: stats(v) for k, v in us.items()}
    ma, mb, mc = (res[k]["us_median"] for k in "abc")
    allowed = 4.0 * mb * (1.0 + res["b"]["self_spread"])
    doc = dict(what="the VampPrior term at L = %d, B = %d, K = %d: (a) ladder_diag_mixture_wide_fwd_bwd at Z = 256, (b) ladder_diag_mixture_fwd_bwd at Z = 64, "
                    "(c) ladder_gmm_wide_logprob_fwd_bwd at Z = 256 with diagonal covariances; HIP events around single calls, 5 warm-up calls per leg, "
                    "%d rounds alternating a, b, c; self_spread = |median of the even rounds - median of the odd rounds| / median" % (L_, B, K, a.reps),
               device_name=torch.cuda.get_device_name(0), reps=a.reps, legs=res, sum_logp=dict(a=out_a.item(), c=out_c.item()),
               a_over_b=round(ma / mb, 3), a_over_c=round(ma / mc, 4), allowed_a_us=round(allowed, 1),
               conditions={"a <= 4 b (1 + spread of b)": bool(ma <= allowed), "a < c": bool(ma < mc)},
               workspace_bytes_a=keep_a[-1].numel(), an_S_K_Z_array_would_be_bytes=4 * L_ * B * K * 256)
    if a.kernel_db:
        times, launches = kernel_times(a.kernel_db), {}
        for name, m in launch_model(256).items():
            if name not in times:
                continue
            n = m.get("launches", 1)
            t = times[name][1] * n                                  # microseconds of this kernel per call of the entry
            bound = max(m["flop"] / PEAK_FLOPS, m["bytes"] / PEAK_BYTES) * 1e6
            launches[name] = dict(us_per_call=round(t, 2), launches_per_call=n, gflop=round(m["flop"] * 1e-9, 4), mbytes=round(m["bytes"] * 1e-6, 3),
                                  achieved_tflops=round(m["flop"] / t * 1e-6, 3), achieved_gbytes_per_s=round(m["bytes"] / t * 1e-3, 1),
                                  bound="fp32 vector" if m["flop"] / PEAK_FLOPS > m["bytes"] / PEAK_BYTES else "HBM", bound_us=round(bound, 2),
                                  share_of_bound=round(bound / t, 4))
        doc["launches_of_a"] = launches
        doc["kernel_us_of_a"] = round(sum(v["us_per_call"] for v in launches.values()), 1)
    print(json.dumps(doc, indent=1))
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    sys.exit(0 if all(doc["conditions"].values()) else 1)


if __name__ == "__main__":
    main()
