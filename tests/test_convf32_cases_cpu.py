"""The case table of the strict-fp32 halo convolutions (tests/convf32_cases.py, run on the device by tests/test_gpu_convf32_matrix.py) reaches what it
claims to reach: the library's own pure-host plan query (ladder_conv3x3_f32_plan: the functions conv3x3_f32_launch calls) and every entry point's
eligibility query agree with `features` for every row, and the union of the rows covers all 21 instantiations of conv3x3_halo_f32s_kernel, every
ragged tail its guards exist for and both route boundaries.  Dropping or reshaping a row so that a form or a guard is no longer run fails here.
No device is needed."""
import pytest

import convf32_cases as R


@pytest.fixture(scope="module")
def L():
    from ladder_latent_data_distribution_modelling_amd import _lib
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    _lib.load(build.build(verbose=False))
    return _lib


ALL = R.CASES + R.REFUSED_ROWS + [row for row, _ in R.CLASS_LOOP]
FEATS = [(r, R.features(r)) for r in R.CASES]
SMALL = [(r, f) for r, f in FEATS if f["family"] == 2]


def _of(entry, rows=SMALL):
    return [(r, f) for r, f in rows if r[0] == entry]


def test_the_library_plans_every_row_as_the_table_says(L):
    assert len(set(R.CASES)) == len(R.CASES) and set(r[0] for r in R.CASES) == set(R.ENTRIES)
    for row in ALL:
        f = R.features(row)
        rc, plan = R.plan_query(L, row)
        assert rc == f["family"] and plan == R.expected_plan(f), (row, plan, R.expected_plan(f))
        assert R.eligible_query(L, row) == f["eligible"], row
    assert all(f["eligible"] == 1 for _, f in FEATS)
    # the query needs no plan buffer
    assert L.query("ladder_conv3x3_f32_plan", *R.internal(R.CASES[0]), None) == 2


def test_every_row_keeps_the_contraction_depth_of_the_stated_bar():
    for row in ALL:
        assert R.features(row)["k"] <= R.K_MAX == 2304, row


@pytest.mark.parametrize("entry", ["plain", "s2bwd", "up2fwd", "up2bwd", "s2fwd"])
def test_every_tiling_in_every_entry(entry):
    """Seven tilings x five entries: all 21 instantiations (UPM 0: plain, s2bwd; 1: up2fwd; 2: up2bwd, s2fwd), each halo mode through every entry that uses it."""
    assert {(f["geo"], f["ni"], f["fks"]) for _, f in _of(entry)} == set(R.FORMS)
    assert [(f["geo"], f["ni"], f["fks"]) for r, f in FEATS if r in R.FORM_ROWS and r[0] == entry] == list(R.FORMS)


def test_the_upsampled_source_runs_every_geometry():
    assert {f["geo"] for _, f in _of("up2fwd_ups")} == {0, 1, 2, 3}


def test_ragged_last_workgroups():
    live = lambda geo, rows=SMALL: {f["live"] for _, f in rows if f["geo"] == geo}  # noqa: E731
    assert live(2) == {1, 2, 3, 4} and live(3) == {1, 2}
    for entry in ("up2fwd", "s2bwd", "up2bwd", "s2fwd"):                            # one ragged row per non-plain entry
        assert any(f["geo"] in (2, 3) and f["live"] < (4 if f["geo"] == 2 else 2) for _, f in _of(entry)), entry
    # the live counts are images: those rows are 8x8 maps (one sub-patch per image)
    assert all(r[2:4] == (8, 8) for r, f in SMALL if f["geo"] in (2, 3) and f["live"] < (4 if f["geo"] == 2 else 2))


def test_ragged_channel_tiles():
    rag = [(r, f) for r, f in SMALL if f["cout_rem"]]
    assert any(f["ni"] == 1 for _, f in rag) and any(f["ni"] == 2 for _, f in rag)
    assert any(R.internal(r)[4] < 64 for r, _ in rag)
    assert any(f["cout_rem"] % 32 for _, f in rag if f["ni"] == 2) and any(f["cout_rem"] == 4 for _, f in rag)      # inside a wave's 32 channels; one float4
    assert all(r[0] in ("plain", "up2bwd", "s2fwd") for r, _ in rag)                # (class launches need whole channel tiles per class)


def test_more_than_one_sub_patch_per_image():
    for sub_w in (16, 8):
        assert any(f["th_n"] > 1 for _, f in SMALL if f["sub_w"] == sub_w), sub_w
        assert any(f["tw_n"] > 1 for _, f in SMALL if f["sub_w"] == sub_w), sub_w
    assert any(f["tw_n"] == 3 and f["geo"] in (2, 3) for _, f in SMALL) and any(f["th_n"] == 3 and f["geo"] in (2, 3) for _, f in SMALL)


def test_route_pairs_sit_on_their_thresholds():
    lo, hi = (R.features(r) for r in R.ROUTE_ROWS)
    assert (lo["grid8x32"], lo["family"]) == (511, 2) and (hi["grid8x32"], hi["family"], hi["grid"]) == (512, 1, 512)
    assert R.ROUTE_ROWS[0][2:] == R.ROUTE_ROWS[1][2:] and R.ROUTE_ROWS[0][1] + 1 == R.ROUTE_ROWS[1][1]
    refused = R.features(R.REFUSED_ROWS[0])
    taken = [f for r, f in FEATS if r[0] == "plain" and r[1] == R.REFUSED_ROWS[0][1] + 1 and r[2:6] == R.REFUSED_ROWS[0][2:6]]
    assert (refused["family"], refused["grid_small"], refused["eligible"]) == (0, 255, 0)
    assert len(taken) == 1 and (taken[0]["family"], taken[0]["grid"]) == (2, 256)


def test_bias_and_activation_are_spread():
    with_epi = [(r, f) for r, f in FEATS if r[0] in R.HAS_EPILOGUE]
    for entry in R.HAS_EPILOGUE:
        rows = [r for r, _ in with_epi if r[0] == entry]
        assert any(r[6] == 0 for r in rows) and any(r[7] == 0 for r in rows) and any(r[6] == 1 and r[7] == 1 for r in rows), entry
    for geo in (0, 1, 2, 3):
        rows = [r for r, f in with_epi if f["family"] == 2 and f["geo"] == geo]
        assert any(r[6] == 0 for r in rows) and any(r[7] == 0 for r in rows) and any(r[6] == 1 and r[7] == 1 for r in rows), geo
    assert all(r[6:] == (0, 0) for r in R.CASES if r[0] not in R.HAS_EPILOGUE)     # (the backward entries take neither)
    for entry in R.ENTRIES:                                                        # NULL bias and act = 0 in every entry
        assert any(r[6] == 0 for r in R.CASES if r[0] == entry) and any(r[7] == 0 for r in R.CASES if r[0] == entry)


def test_class_loop_group_is_the_8x32_kernels_class_launches():
    """Every row of the child-process group is a class launch of the 8x32-pixel kernel below the 512-patch threshold: LADDER_CLASS_LOOP decides its mapping."""
    rows = R.CLASS_LOOP
    for row, proj in rows:
        f = R.features(row)
        assert f["family"] == 1 and f["flag"] == 0 and f["tiles_m"] < 512 and f["internal"][4] == 512 and 1 <= f["internal"][5] <= 3, row
    for entry in ("up2fwd", "up2fwd_ups"):
        assert {p for r, p in rows if r[0] == entry} == {None, (3, 0), (3, 1)}
    assert any(r[0] == "s2bwd" and r[4] == 128 for r, _ in rows)
