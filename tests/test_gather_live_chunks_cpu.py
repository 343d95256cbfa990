"""ladder_igemm_fwd_live_chunks (host arithmetic of csrc/igemm.hip) against a numpy brute force: per row tile of each launch, the (tap, 16-channel
slab) pairs with at least one row whose tap lies inside the gathered image, over the geometries of tests/test_gpu_gather_small_maps.py; and the
closed forms at batch 128 (4 / 9 for 2x2 SAME, 2.25 / 9 for the backward-data of 4x4 -> 2x2 VALID, 121 / 144 for 8x8 -> 4x4 stride 2)."""
import numpy as np
import pytest

from ladder_latent_data_distribution_modelling_amd import _lib as L
from ladder_latent_data_distribution_modelling_amd import arch

CASES = [
    (64, 2, 2, 16, 64, 3, 1, "same"), (128, 2, 2, 16, 64, 3, 1, "same"), (96, 2, 2, 16, 64, 3, 1, "same"), (3, 2, 2, 16, 64, 3, 1, "same"),
    (64, 4, 4, 16, 16, 3, 1, "valid"), (64, 8, 8, 16, 32, 3, 2, "same"), (64, 2, 2, 16, 16, 5, 1, "same"), (2, 8, 8, 16, 48, 1, 2, "same"),
    (128, 2, 2, 256, 256, 3, 1, "same"), (32, 1, 1, 16, 128, 3, 1, "same"), (8, 4, 4, 32, 160, 3, 1, "same"), (4, 8, 8, 20, 64, 3, 1, "same"),
    (128, 4, 4, 512, 512, 3, 1, "valid"), (128, 8, 8, 256, 512, 3, 2, "same"), (128, 2, 2, 512, 512, 3, 1, "same"),
    (64, 4, 4, 64, 64, 3, 1, "valid"), (64, 8, 8, 64, 64, 3, 2, "same"), (64, 2, 2, 64, 64, 5, 1, "same"),
]


def _launch_chunks(N, src_hw, rows_hw, taps, Cg, Cout_g, skipping):
    """One launch: GEMM rows = N x rows_hw output pixels, each tap = a function (ho, wo) -> source pixel (h, w) of a src_hw map; Cg gathered
    channels, Cout_g GEMM columns.  Returns (live chunks, all chunks) over all tiles."""
    (Hs, Ws), (Ho, Wo) = src_hw, rows_hw
    M = N * Ho * Wo
    t = abs(L.query("ladder_igemm_fwd_tile", M, Cg, Cout_g))
    bm, bn = t // 1000, t % 1000
    tiles_m, tiles_n = -(-M // bm), -(-Cout_g // bn)
    nchunks = -(-(len(taps) * Cg) // 16)
    full = tiles_m * tiles_n * nchunks
    small_tile = (bm, bn) in ((64, 64), (32, 128))
    if not (skipping and small_tile and Cg % 16 == 0 and len(taps) > 1 and Ho * Wo <= 16):
        return full, full
    posmajor = N >= bm
    live = 0
    for tm in range(tiles_m):
        alive = set()
        for m in range(tm * bm, min((tm + 1) * bm, M)):
            pos = m // N if posmajor else m % (Ho * Wo)
            ho, wo = divmod(pos, Wo)
            for ti, tap in enumerate(taps):
                h, w = tap(ho, wo)
                if 0 <= h < Hs and 0 <= w < Ws:
                    alive.add(ti)
        live += len(alive) * (Cg // 16)
    return live * tiles_n, full


def brute_force(case, bwd, skipping=True):
    N, H, W, Cin, Cout, k, s, pad = case
    pt, Ho = arch.conv_out(H, k, s, pad)
    pl, Wo = arch.conv_out(W, k, s, pad)
    if not bwd:
        taps = [(lambda ho, wo, r=r, c=c: (ho * s + r - pt, wo * s + c - pl)) for r in range(k) for c in range(k)]
        return _launch_chunks(N, (H, W), (Ho, Wo), taps, Cin, Cout, skipping)
    if s == 1:     # dx[hi] gathers dy[hi + pad_t - r]
        taps = [(lambda hi, wi, r=r, c=c: (hi + pt - r, wi + pl - c)) for r in range(k) for c in range(k)]
        return _launch_chunks(N, (Ho, Wo), (H, W), taps, Cout, Cin, skipping)
    assert s == 2 and Cout % 16 == 0
    live = full = 0
    classes = []
    for ch in range(2):          # output pixels of parity (ch, cw) see the taps with (hi + pad_t - r) even: one dense launch each
        for cw in range(2):
            hh, ww = (H - ch + 1) // 2, (W - cw + 1) // 2
            taps = [(lambda a, b, r=r, c=c, ch=ch, cw=cw: ((2 * a + ch + pt - r) // 2, (2 * b + cw + pl - c) // 2))
                    for r in range(k) if (ch + pt - r) % 2 == 0 for c in range(k) if (cw + pl - c) % 2 == 0]
            if hh * ww > 0:
                classes.append(((hh, ww), taps))
    if any(not taps for _, taps in classes):   # a class without a tap: one generic launch over all taps writes the zeros
        M = N * H * W
        t = abs(L.query("ladder_igemm_fwd_tile", M, Cout, Cin))
        full = -(-M // (t // 1000)) * -(-Cin // (t % 1000)) * -(-(k * k * Cout) // 16)
        return full, full
    for hw, taps in classes:
        a, b = _launch_chunks(N, (Ho, Wo), hw, taps, Cout, Cin, skipping)
        live, full = live + a, full + b
    return live, full


def _query(case, bwd, variant):
    N, H, W, Cin, Cout, k, s, pad = case
    pt, Ho = arch.conv_out(H, k, s, pad)
    pl, Wo = arch.conv_out(W, k, s, pad)
    return L.query("ladder_igemm_fwd_live_chunks", N, H, W, Cin, Ho, Wo, Cout, k, k, s, pt, pl, int(bwd), variant)


@pytest.mark.parametrize("bwd", [False, True], ids=["fwd", "bwd_data"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_live_chunks_match_brute_force(case, bwd):
    live, full = brute_force(case, bwd)
    assert 0 < live <= full
    for variant in (0, 2, 4, 6):                       # no skipping at any depth: the full tap walk
        assert _query(case, bwd, variant) == full
    for variant in (1, 3, 5, 7):
        assert _query(case, bwd, variant) == live
    assert _query(case, bwd, -1) in (live, full)       # the default (or LADDER_IGEMM_VARIANT) is one of the two
    assert _query(case, bwd, 8) == -1


def test_closed_forms_at_batch_128():
    for C in (64, 512):     # (a GEMM of at most 32 columns runs the 128x32 tile, which walks every tap)
        assert np.isclose(_query((128, 2, 2, C, C, 3, 1, "same"), False, 1) / _query((128, 2, 2, C, C, 3, 1, "same"), False, 0), 4 / 9)
        assert np.isclose(_query((128, 2, 2, C, C, 3, 1, "same"), True, 1) / _query((128, 2, 2, C, C, 3, 1, "same"), True, 0), 4 / 9)
        assert np.isclose(_query((128, 4, 4, C, C, 3, 1, "valid"), True, 1) / _query((128, 4, 4, C, C, 3, 1, "valid"), True, 0), 2.25 / 9)
        assert np.isclose(_query((128, 8, 8, C, 2 * C, 3, 2, "same"), False, 1) / _query((128, 8, 8, C, 2 * C, 3, 2, "same"), False, 0), 121 / 144)


def test_other_kernels_are_reported():
    # 3x3 / stride 1 / SAME on a large map runs the halo kernel, not the gather kernel
    assert L.query("ladder_igemm_fwd_live_chunks", 16, 64, 64, 32, 64, 64, 256, 3, 3, 1, 1, 1, 0, 1) == -1
