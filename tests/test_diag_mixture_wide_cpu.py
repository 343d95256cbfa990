"""The wide VampPrior term (csrc/diag_mixture.hip) without a GPU: its workspace query answers non-zero exactly for the shapes the entry takes, and
the family table's lookup names the narrow pair, the wide pair, or -- for the widths neither takes -- the pair whose refusal is today's failure."""
import pytest

E_SHAPE = -1
NARROW = ("ladder_diag_mixture_workspace_bytes", "ladder_diag_mixture_fwd_bwd", False)
WIDE = ("ladder_diag_mixture_wide_workspace_bytes", "ladder_diag_mixture_wide_fwd_bwd", True)


@pytest.fixture(scope="module")
def lib():
    from ladder_latent_data_distribution_modelling_amd import _lib
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    return _lib.load(build.build(verbose=False))


def test_workspace_query_is_nonzero_exactly_for_the_shapes_taken(lib):
    for Z in range(0, 273):
        for K in (0, 1, 50, 1024, 1025):
            for Lmc in (0, 1, 100):
                for B in (0, 1, 100):
                    takes = 80 <= Z <= 256 and Z % 16 == 0 and 1 <= K <= 1024 and Lmc >= 1 and B >= 1
                    assert (lib.ladder_diag_mixture_wide_workspace_bytes(Lmc, B, Z, K) != 0) == takes, (Lmc, B, Z, K)


def test_workspace_grows_with_samples_and_components_never_with_their_product_by_width(lib):
    """r [S, K] and the per-slice [K, Z] partials: at the shipped shape (L 100, B 128, K 50, Z 256) an [S, K, Z] array alone would be 655 MB."""
    q = lib.ladder_diag_mixture_wide_workspace_bytes
    assert q(100, 128, 256, 50) < 64 << 20
    assert q(1, 1, 80, 1) < 1 << 16
    assert q(100, 128, 256, 1024) < 512 << 20            # the slices' partials are capped, whatever K


def test_engine_names_the_entry_pair_by_width(lib):
    from ladder_latent_data_distribution_modelling_amd.mixture_forms import family

    def pair(Z):
        row = family("diag_term", 4, Z)
        return row.workspace_bytes, row.fwd_bwd, row.query_takes_L
    for Z in range(1, 65):
        assert pair(Z) == NARROW, Z
    for Z in range(80, 257, 16):
        assert pair(Z) == WIDE, Z
    # neither tier takes these: the lookup still names the narrow pair, and its refusal (before any launch) is what such a model met before
    for Z in list(range(65, 80)) + [72, 88, 250, 272]:
        assert pair(Z) == NARROW, Z
        assert lib.ladder_diag_mixture_fwd_bwd(*([None] * 5), 3, 2, Z, 4, *([None] * 5), None, 0, None) == E_SHAPE, Z
        assert lib.ladder_diag_mixture_wide_fwd_bwd(*([None] * 5), 3, 2, Z, 4, *([None] * 5), None, 0, None) == E_SHAPE, Z
