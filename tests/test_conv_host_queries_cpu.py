"""The host planning of the implicit-GEMM convolution files (csrc/igemm.hip, igemm_wgrad.hip, igemm_split.hip, convdirect.hip) answers every
pure-host query as tests/golden/conv_host_queries.json recorded it (tests/golden/make_conv_host_queries.py: tile, split-K and workspace
planning, kernel ids and eligibility over the geometries of the GPU tests, of the shipped configs and degenerate ones, with and without
LADDER_DISABLE_HALO=1).  No device is needed."""
import importlib.util
import json
import os

import pytest


@pytest.fixture(scope="module")
def lib_path():
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    return build.build(verbose=False)


def test_host_queries_match_recorded_planning(lib_path, golden_dir):
    spec = importlib.util.spec_from_file_location("make_conv_host_queries", os.path.join(golden_dir, "make_conv_host_queries.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    want = json.load(open(os.path.join(golden_dir, "conv_host_queries.json")))
    got = rec.record(lib_path)
    assert got["queries"] == want["queries"] and len(want["queries"]) == 25
    assert sorted(got["answers"]) == sorted(want["answers"])                 # the same geometries
    diff = {g: (got["answers"][g], v) for g, v in want["answers"].items() if got["answers"][g] != v}
    assert not diff, dict(list(diff.items())[:5])
    # the recording exercises both answers of the switchable queries: the halo routes exist and LADDER_DISABLE_HALO=1 removes them
    kid = want["queries"].index("conv2d_fwd_kernel_id")
    assert 256128 in {v[0][kid] for v in want["answers"].values()}
    assert 256128 not in {(v[1] or v[0])[kid] for v in want["answers"].values()} and any(v[1] for v in want["answers"].values())
    assert len(want["answers"]) >= 80
