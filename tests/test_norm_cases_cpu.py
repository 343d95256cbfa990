"""The case table of the norm and element-wise passes (tests/norm_cases.py, run on the device by tests/test_gpu_norm_matrix.py) reaches what it claims to
reach.  `features` is held against the library where the library can be asked on the host (ladder_bn_workspace_bytes: stats_nblk;
ladder_in_style_workspace_bytes: in_split), the rows of every family are the ones the table is specified with (a dropped or reshaped row fails here), and
the union of the rows covers every kernel of csrc/norm.hip the table is about, every loop of them on both sides of its boundary and every route decision.
No device is needed."""
import itertools
import os
import re

import pytest

import norm_cases as R

FEATS = [(r, R.features(r)) for r in R.CASES]


def _of(entry):
    return [(r, f) for r, f in FEATS if r[0] == entry]


@pytest.fixture(scope="module")
def L():
    from ladder_latent_data_distribution_modelling_amd import _lib
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    _lib.load(build.build(verbose=False))
    return _lib


def test_the_table_holds_exactly_the_specified_rows():
    assert len(set(R.CASES)) == len(R.CASES)
    rows = lambda e: [r[1:] for r in R.CASES if r[0] == e]  # noqa: E731
    two_sweep = [(33000, 96), (30000, 100), (40000, 64), (60000, 10)]
    assert sorted(rows("bn"), key=str) == sorted(
        [(r, c, a, "plain") for r, c in two_sweep for a in ("leaky_relu", None)]
        + [(40000, 64, "leaky_relu", "absmax"), (40000, 64, "leaky_relu", "pgrad_only"), (9000, 64, "leaky_relu", "shift_x"), (9000, 64, None, "shift_y"),
           (33000, 96, "leaky_relu", "planes"), (100, 96, "leaky_relu", "plain"), (77, 10, None, "plain")], key=str)
    assert sorted(rows("refuse")) == [("minmax_misaligned_x",), ("minmax_planes_c_not_4",), ("planes_n_not_8",), ("record_on_scalar_route",)]
    assert sorted(rows("colstats")) == sorted([(r, 8, 0) for r in (1, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 2049)]
                                              + [(r, 3, 0) for r in (1, 3, 4, 5, 31, 32, 33, 1025)] + [(525288, 4, 0), (525288, 3, 0), (129, 8, 1)])
    assert sorted(rows("stage2")) == sorted(itertools.product((0, 1), (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023), (1, 3, 16, 100)))
    assert sorted(rows("in")) == sorted([(2, 16, 16, 32, "off"), (2, 16, 16, 32, "off_corner"), (2, 3, 5, 8, "off"), (1, 17, 241, 4, "off"), (1, 65, 63, 4, "off"),
                                         (1024, 16, 16, 4, "off"), (3, 16, 16, 72, "absmax"), (2, 5, 5, 10, "off")])
    assert sorted(rows("resize")) == sorted([(2, 3, 5, 8, 6, 20, 0), (1, 4, 2, 3, 12, 2, 0), (1, 2, 8, 160, 4, 16, 0), (1, 2, 90, 3, 4, 180, 0), (2, 3, 5, 8, 6, 10, 1),
                                             (1, 2, 90, 3, 6, 180, 0)])
    assert sorted(rows("d2s")) == [(1, 2, 40, 64, 2, 0), (1, 2, 40, 64, 2, 1), (2, 3, 5, 4, 2, 0)]
    assert sorted(rows("pad")) == [(2, 5, 7, 3, 0), (2, 5, 7, 3, 1), (2, 5, 7, 3, 5), (8, 126, 126, 5, 1), (8, 128, 130, 5, 2)]
    assert sorted(rows("act_bwd"), key=str) == sorted(itertools.product((1, 2, 3, 4, 5, 7, 1024, 2097152 + 7), (None, "leaky_relu", "relu", "tanh")), key=str)
    assert {r[0] for r in R.CASES} == set(R.RUNNERS)
    assert all(f["elems"] <= R.MAX_ELEMS for _, f in FEATS)                          # cheap float64 references, a few seconds per row on the device


def test_the_library_sizes_its_workspaces_as_features_says(L):
    for r, f in _of("bn") + _of("colstats"):
        assert L.query("ladder_bn_workspace_bytes", r[1], r[2]) == f["nblk"] * 2 * r[2] * 8, r
    for r, f in _of("in"):
        _, N, H, W, C, _ = r
        assert L.query("ladder_in_style_workspace_bytes", N, H * W, C) == N * f["split"] * 2 * C * 4 == f["ws_bytes"], r
    for rows in (1, 1024, 1025, 524288, 524289, 525288, 1 << 22):
        assert L.query("ladder_bn_workspace_bytes", rows, 1) == R.stats_nblk(rows) * 16
    for N, HW, C in ((1, 1, 4), (1, 64, 4), (1, 65, 4), (32, 4096, 64), (33, 4096, 65), (2048, 1 << 16, 4), (4096, 100, 8)):
        assert L.query("ladder_in_style_workspace_bytes", N, HW, C) == N * R.in_split(N, HW, C) * 2 * C * 4


def test_every_kernel_the_table_is_about_is_launched():
    src = open(os.path.join(R.ROOT, "ladder_latent_data_distribution_modelling_amd", "csrc", "norm.hip")).read()
    in_file = set(re.findall(r"__global__[^\n;{]*?void (\w+)\(", src))
    out_of_scope = {"gather_rows_u8_kernel", "gather_rows_scalar_kernel", "axpy_kernel"}   # minibatch assembly and ladder_axpy: not this table's
    assert out_of_scope <= in_file
    reached = set().union(*(f["kernels"] for _, f in FEATS))
    assert {k.split("<")[0] for k in reached} == in_file - out_of_scope
    assert reached >= {"colstats_stage1<%s,%d>" % (row, v) for row in ("MomentsRow<false>", "BnBwdRow") for v in (4, 1)} | {"colstats_stage1<MomentsRow<true>,4>"}
    assert reached >= {"colstats_stage2<64,16,1>", "colstats_stage2<16,16,1>", "colstats_stage2<16,64,4>"}
    assert reached >= {"%s<%d>" % (k, v) for k in ("resize_fwd_kernel", "resize_bwd_kernel", "resize_bwd_x2_kernel", "d2s_kernel") for v in (4, 1)}


def test_batch_norm_sweeps_and_routes():
    bn = _of("bn")
    for v4 in (True, False):                          # one and two sweeps of the float4 and of the scalar apply, forward and backward
        assert {f["sweeps_fwd"] for _, f in bn if f["v4_fwd"] == v4} == {1, 2}
        assert {f["sweeps_bwd"] for _, f in bn if f["has_dx"] and f["v4_bwd"] == v4} == {1, 2}
    two = [(r, f) for r, f in bn if f["v4_fwd"] and f["sweeps_fwd"] == 2 and f["sweeps_bwd"] == 2]
    assert {f["fixed"] for _, f in two} == {True, False}
    assert 2 ** 21 % 96 == 32 and 2 ** 21 % 100 == 52 and 2 ** 21 % 64 == 0
    for r, f in two:                                  # the conditions those rows rely on
        assert r[1] * r[2] // 4 > 2048 * 256 and f["fixed"] == ((2 ** 21) % r[2] == 0), r
    for r, f in bn:
        if not f["v4_fwd"] and r[1] > 1000:
            assert r[1] * r[2] > 2048 * 256 and f["sweeps_fwd"] == 2, r
    # !fixed on ONE sweep too (there (i * 4) % C and (i0 * 4) % C are the same number), and every kernel with the !fixed branch on two
    assert any(not f["fixed"] and f["sweeps_fwd"] == 1 and f["v4_fwd"] for _, f in bn)
    for k in ("bn_apply_kernel", "bn_apply_planes_kernel", "bn_bwd_apply_v4_kernel"):
        assert any(k in f["kernels"] and not f["fixed"] and f["sweeps_fwd"] == 2 for _, f in bn), k
    assert any("bn_apply_kernel" in f["kernels"] and f["fixed"] and f["sweeps_fwd"] == 2 and f["record"] for _, f in bn)      # the _absmax entries: no fold
    assert {f["fold"] for _, f in bn if f["v4_fwd"]} == {True, False} and any(f["fold"] and f["sweeps_fwd"] == 2 for _, f in bn)
    assert {f["pgrad_rides"] for _, f in bn} == {True, False} and any(f["pgrad_rides"] and f["sweeps_bwd"] == 2 for _, f in bn)
    assert any(not f["has_dx"] for _, f in bn)
    assert any(f["idle_lanes"] and f["v4_fwd"] and f["sweeps_fwd"] == 2 for _, f in bn)
    shifted = [(r, f) for r, f in bn if f["shifted"]]                                    # a C % 4 == 0 tensor on the scalar kernels, two sweeps
    assert {r[4] for r, _ in shifted} == {"shift_x", "shift_y"}
    assert all(f["c4"] and not f["v4_fwd"] and not f["v4_bwd"] and f["sweeps_fwd"] == 2 and f["sweeps_bwd"] == 2 for _, f in shifted)
    assert {r[3] for r, f in bn if f["sweeps_fwd"] == 2 and r[4] == "plain" and r[1:3] == (33000, 96)} == {"leaky_relu", None}


def test_column_statistics_loops():
    cs = _of("colstats")
    for V, RL in ((4, 16), (1, 4)):
        mine = [(r, f) for r, f in cs if f["V"] == V and not f["shifted"]]
        assert any(f["tail_only"] and not f["batch"] for _, f in mine) and any(f["batch"] and not f["tail"] for _, f in mine), V
        assert any(f["both"] for _, f in mine) and any(f["idle_lane"] for _, f in mine), V
        at = 8 * RL                                   # the batched loop's boundary: one row short of it, on it, one past it
        assert {at - 1, at, at + 1} <= {r[1] for r, _ in mine}
        assert R.stage1_loops(at, V)["batch"] and not R.stage1_loops(at, V)["tail"] and not R.stage1_loops(at - 7 * RL, V)["batch"]
        capped = [f for r, f in mine if r[1] > 512 * 1024]
        assert len(capped) == 1 and (capped[0]["nblk"], capped[0]["per"], capped[0]["last"]) == (512, 1026, 1002), V
        assert {f["nblk"] for _, f in mine} >= {1, 2, 512}
    assert any(f["minmax"] and f["nblk"] == 512 for _, f in cs)
    sh = [(r, f) for r, f in cs if f["shifted"]]
    assert len(sh) == 1 and sh[0][1]["c4"] and sh[0][1]["V"] == 1 and not sh[0][1]["minmax"]


def test_second_stage_instantiations_on_both_sides_of_their_lane_count():
    by = {}
    for r, f in FEATS:
        if "stage2" in f:
            name = [k for k in f["kernels"] if k.startswith("colstats_stage2")][0]
            by.setdefault(name, []).append(f["stage2"])
    for _, f in _of("bn"):
        by["colstats_stage2<64,16,1>"].append(R.stage2_loops(16, 1, f["nblk"]))
    assert set(by) == {"colstats_stage2<64,16,1>", "colstats_stage2<16,16,1>", "colstats_stage2<16,64,4>"}
    for name, loops in by.items():
        assert {s["side"] for s in loops} >= {-1, 1}, name
    for name in ("colstats_stage2<16,16,1>", "colstats_stage2<16,64,4>"):
        assert {s["side"] for s in by[name]} == {-1, 0, 1}, name
    four = by["colstats_stage2<16,64,4>"]
    assert set().union(*(s["left"] for s in four)) >= {0, 1, 2, 3}
    assert any(s["main"] == {1} and s["left"] == {0} for s in four)                      # 256 partials: the four-accumulator loop alone
    assert any(0 in s["main"] and 1 in s["main"] and 3 in s["left"] for s in four)       # 255: its last lane is three strides of remainder
    assert any(s["main"] == {1} and s["left"] == {0, 1} for s in four)                   # 257
    assert any(max(s["main"]) == 4 for s in four)
    st = _of("stage2")
    assert {r[3] % 16 for r, _ in st} >= {0, 1, 3, 4} and any(f["dead_columns"] for _, f in st) and any(not f["dead_columns"] for _, f in st)
    assert any(r[2] == 1 for r, _ in st)


def test_instance_norm_splits_and_pivots():
    rows = _of("in")
    assert any(f["vec"] and f["last_split"] == 1 and f["split"] == 65 for _, f in rows)
    assert any(f["vec"] and f["last_split"] == f["per"] - 1 and f["split"] > 1 for _, f in rows)
    lim = [f for _, f in rows if f["vec"] and f["split_limit"] == "groups"]
    assert len(lim) == 1 and (lim[0]["split"], lim[0]["per"]) == (2, 128)
    assert any(f["pivots"] < 16 and not f["square"] and f["vec"] for _, f in rows) and all(f["HW"] >= 15 for _, f in rows)
    assert any(f["idle_quads"] and f["record"] for _, f in rows) and any(not f["vec"] for _, f in rows)
    assert {r[5] for r, _ in rows} == {"off", "off_corner", "absmax"}
    assert all(f["ws_bytes"] > 0 for _, f in rows)


def test_resize_depth_to_space_pad_and_act_bwd_edges():
    rz = _of("resize")
    assert any(f["fy"] != f["fx"] and f["fy"] > 1 and f["fx"] > 1 for _, f in rz) and any(f["fx"] == 1 and f["fy"] == 3 and f["V"] == 1 for _, f in rz)
    assert all(r[2] != r[3] for r, _ in rz)                                               # no square map: a swap of H / W shows
    for V in (4, 1):
        assert any(f["bpr"] == 2 and f["x2"] and f["V"] == V and f["ragged"] for _, f in rz), V   # forward and the factor-2 transpose
    assert any(f["bpr"] >= 2 and not f["x2"] for _, f in rz)                              # the general transpose
    assert any(f["shifted"] and f["c4"] and f["V"] == 1 and f["gated"] for _, f in rz)
    d2 = _of("d2s")
    assert any(not f["seg4"] and f["V"] == 1 for _, f in d2) and any(f["bpr"] == 2 and f["V"] == 4 for _, f in d2)
    assert any(f["shifted"] and f["seg4"] and f["V"] == 1 and f["bpr"] >= 2 for _, f in d2)
    pd = _of("pad")
    assert {f["p"] for _, f in pd} >= {0, 1, 2, 5} and any(f["p"] == f["H"] for _, f in pd) and all(r[4] > 1 for r, _ in pd)
    assert any(f["sweeps_fwd"] == 2 for _, f in pd) and any(f["sweeps_bwd"] == 2 for _, f in pd) and any(f["sweeps_fwd"] == 1 and f["sweeps_bwd"] == 1 for _, f in pd)
    ab = _of("act_bwd")
    assert any(f["sweeps4"] == 2 and f["tail"] == 3 for _, f in ab) and any(f["sweeps4"] == 0 and f["tail"] for _, f in ab)
    assert {f["tail"] for _, f in ab} == {0, 1, 2, 3} and {r[2] for r, _ in ab} == set(R.ACT) and R.ACT == {None: 0, "leaky_relu": 1, "relu": 2, "tanh": 3}


def test_a_shifted_row_in_every_entry_family():
    for entry in ("bn", "colstats", "in", "resize", "d2s"):
        assert any(f.get("shifted") for _, f in _of(entry)), entry
    assert ("refuse", "minmax_misaligned_x") in R.CASES


def test_the_restatement_stays_inside_the_stated_bars():
    """The data are chosen so that the fp32 restatement of the formulas (mean and 1 / sd rounded to fp32) stays within a quarter of every stated bar: then
    the stated bars hold unchanged on the device (which prints the figure of every row).  Largest restatement errors: batch norm y 2.6e-7, dx 1.8e-7,
    dgamma 1.8e-7, dbeta 1.9e-7; instance norm (means 50 sd off zero) y 1.9e-6, dx 8.7e-7, dstyle 2.4e-6."""
    for r in R.BN_ROWS:
        d = R.bn_reference(*r[1:4])
        assert R.bn_bars(d["rest"]) == dict(y=R.BAR_Y, dx=R.BAR_DX_BN, dgamma=R.BAR_PARAM, dbeta=R.BAR_PARAM), (r, d["rest"])
    for r in R.IN_ROWS:
        d = R.in_reference(*r[1:5], "off" if r[5] == "absmax" else r[5])
        assert R.in_bars(d["rest"]) == dict(y=R.BAR_Y, up=R.BAR_Y, dx=R.BAR_DX_IN, dstyle=R.BAR_PARAM), (r, d["rest"])
