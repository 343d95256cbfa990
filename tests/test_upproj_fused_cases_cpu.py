"""The case table of the fused pair forward (tests/upproj_fused_ref.py, run on the device by tests/test_gpu_upproj_fused_matrix.py) reaches what it
claims to reach: the library's own host queries (csrc/upproj.hip: eligibility, the 128-pixel kernel's routing, the projection workspace) agree with
`features` for every case, and the union of the cases' features covers every ring remainder, width, workgroup mapping and projection form listed
below.  Dropping or reshaping a case so that a loop tail or an epilogue form is no longer run fails here.  No device is needed."""
import pytest

import upproj_fused_ref as R


@pytest.fixture(scope="module")
def L():
    from ladder_latent_data_distribution_modelling_amd import _lib
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    _lib.load(build.build(verbose=False))
    return _lib


FEATS = [(c, R.features(c)) for c in R.CASES]
PX_RES = [(c, f) for c, f in FEATS if f["kernel"] == "px64" and f["resident"]]
PX_STR = [(c, f) for c, f in FEATS if f["kernel"] == "px64" and not f["resident"]]
WIDE = [(c, f) for c, f in FEATS if f["kernel"] == "wide"]


def _set(rows, key):
    return {f[key] for _, f in rows}


def test_the_library_routes_every_case_as_the_table_says(L):
    assert len(set(R.CASES)) == len(R.CASES) == sum(len(g) for g in R.GROUPS.values())
    for case, f in FEATS:
        N, H, W, cin, cout, pco = case[:6]
        assert L.query("ladder_up2proj_fused_eligible", N, H, W, cin, cout) == 1, case
        assert L.query("ladder_up2proj_fused_wide_tile", N, H, W, cin, cout) == (1 if f["kernel"] == "wide" else 0), case
        assert L.query("ladder_up2proj_fused_workspace_bytes", N, H, W, cout, pco) == f["nslab"] * 4 * N * H * W * pco * 4, case
        assert f["total"] == H * cin // 32 and cin % 32 == 0 and f["nslab"] * 16 == cout
    # the groups are what their names say (the child-process runs of the GPU test pick them by name)
    assert [c for c, _ in PX_RES] == R.GROUPS["resident"] and [c for c, _ in PX_STR] == R.GROUPS["streamed"] and [c for c, _ in WIDE] == R.GROUPS["wide"]


def test_px64_resident_slab_coverage():
    assert _set(PX_RES, "stage_mod") == set(range(8))                       # x staging unrolled by 8, 7 loads ahead
    assert _set(PX_RES, "mod3") == {0, 1, 2}                                # MFMA loop unrolled by 3
    assert {4, 6} <= _set(PX_RES, "total")                                  # fewer chunks than the staging pipeline is deep
    assert _set(PX_RES, "W") == {8, 16, 32, 64}
    assert _set(PX_RES, "xcd") == {True, False}
    assert max(_set(PX_RES, "nslab")) >= 3


def test_px64_streamed_slab_coverage():
    assert _set(PX_STR, "stage_mod") == set(range(4))                       # staging unrolled by 4, 3 loads ahead
    assert _set(PX_STR, "mod3") == {0, 1, 2}
    assert _set(PX_STR, "W") == {8, 16, 32, 64}
    assert _set(PX_STR, "xcd") == {True, False}


def test_wide_kernel_coverage():
    assert _set(WIDE, "mod2") == {0, 1}                                     # MFMA loop unrolled by 2
    assert _set(WIDE, "mod3") == {0, 1, 2}                                  # staging unrolled by 3
    assert _set(WIDE, "W") == {16, 32}
    assert _set(WIDE, "xcd") == {True, False}
    assert 2 in {c[1] for c, _ in WIDE}
    assert all(c[5] == 0 and c[6] == 1 for c, _ in WIDE)                    # (the kernel has no projection and always writes y)


def test_projection_and_argument_coverage():
    for rows in (PX_RES, PX_STR):
        assert {(c[5], c[6]) for c, _ in rows if c[5]} == {(pco, keep) for pco in (1, 2, 3, 4) for keep in (0, 1)}
        # every shape of the 64-pixel kernel once with and once without the projection
        assert {c[:5] for c, _ in rows if c[5]} == {c[:5] for c, _ in rows if not c[5]} == {c[:5] for c, _ in rows}
    assert any(c[5] and c[7] == 0 for c in R.CASES)                         # projection of an un-activated map
    for rows in (PX_RES, PX_STR, WIDE):
        assert any(c[8] == 0 for c, _ in rows)                              # bias == NULL
    assert any(c[5] and c[9] == 0 for c in R.CASES)                         # proj_b == NULL
    assert {c[5] for c in R.CASES if c[10]} >= {1, 3}                       # the scalar reduction (proj_out 4-byte aligned only)
    assert all(c[6] == 1 and c[9] == 0 and c[10] == 0 for c in R.CASES if not c[5])
    assert all(c[3] <= 256 for c in R.CASES)                                # TOL32 is derived for K = Cin <= 512


def test_reference_is_sensitive_to_a_single_dropped_chunk():
    """The comparison the GPU test makes would see one missing 32-deep chunk of one row: removing it from the float64 reference of the smallest case
    moves the map by far more than TOL32 of its scale."""
    import numpy as np
    import torch
    from oracle import ladder_oracle as O
    case = R.GROUPS["streamed"][0]
    (x, w, b, _, _), ref, _ = R.reference(case)
    N, H, W = case[:3]
    x2 = x.copy()
    x2[:, H - 1, :, -32:] = 0.0                                             # the last chunk of the last row
    up = O.resize_bilinear_legacy(torch.as_tensor(x2, dtype=torch.float64), 2 * H, 2 * W)
    y2 = O.conv2d_tf(up, torch.as_tensor(w, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64), 1, "same").numpy()
    y2 = np.where(y2 > 0, y2, 0.2 * y2) if case[7] else y2
    assert R._rel(y2, ref) > 1e3 * R.TOL32
