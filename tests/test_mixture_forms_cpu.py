"""The family table of the mixture operations (mixture_forms.py) without a GPU: over every width 0 .. 272 and a spread of component counts the
lookup gives the family, or the refusal, that each owner's own rule gave before there was a table (written out below as literal ranges, not read from
the table); where a family's size query answers 0 outside its shapes the row's rule and the query agree; and the table and the ctypes prototypes
name the same mixture entry points, each once."""
import os
import re

import pytest

WIDTHS = range(0, 273)
COUNTS = (0, 1, 50, 64, 65, 1024, 1025)
WIDE_WIDTHS = range(80, 257, 16)                 # 80, 96, ..., 256

# operation -> (role whose entry name tells the families apart, f(K, R) -> that name, or (exception type, regex of its message))
EM_REFUSAL = (ValueError, r"the device EM fit takes samples of 1 \.\. 64 dimensions, or 80 \.\. 256 in steps of 16, got \d+$")
KMEANS_REFUSAL = (NotImplementedError, r"the HIP k-means covers 1 <= n_clusters <= 64 and 1 <= n_features <= 64 or 80 <= n_features <= 256 in steps of 16, "
                                       r"got \d+ and \d+$")
VB_REFUSAL = (ValueError, r"the HIP mixture fit takes a representation of at most 64 dimensions, got \d+$")
SLP_REFUSAL = (ValueError, r"SLPInterpolator: the wide mixture \(R > 8\) needs R % 4 == 0 and R <= 64 \(got R = \d+\)$")
EXPECTED = {
    "term": ("fwd_bwd", lambda K, R: "ladder_gmm_logprob_fwd_bwd" if R <= 8 else "ladder_gmm_dense_logprob_fwd_bwd" if R <= 64
             else "ladder_gmm_wide_logprob_fwd_bwd"),
    "sampler": ("sample", lambda K, R: "ladder_mixture_sample" if R <= 64 else "ladder_mixture_sample_wide"),
    "em": ("mstep", lambda K, R: "ladder_emgmm_mstep" if 1 <= R <= 64 else "ladder_emgmm_wide_mstep" if R in WIDE_WIDTHS else EM_REFUSAL),
    "kmeans": ("assign", lambda K, R: KMEANS_REFUSAL if not 1 <= K <= 64 else "ladder_kmeans_assign" if 1 <= R <= 64
               else "ladder_kmeans_wide_assign" if R in WIDE_WIDTHS else KMEANS_REFUSAL),
    "vb": ("estep", lambda K, R: "ladder_vbgmm_shard_estep" if R <= 8 else "ladder_vbgmm_wide_estep" if R <= 64 else VB_REFUSAL),
    "slp": ("optimise", lambda K, R: "ladder_slp_optimise" if R <= 8 else "ladder_slp_wide_optimise" if (R <= 64 and R % 4 == 0) else SLP_REFUSAL),
    # the VampPrior term: the wide pair exactly where it takes the width, the narrow pair (whose entry refuses before any launch) everywhere else; K has no say
    "diag_term": ("fwd_bwd", lambda K, R: "ladder_diag_mixture_wide_fwd_bwd" if R in WIDE_WIDTHS else "ladder_diag_mixture_fwd_bwd"),
}
MIXTURE_PREFIXES = ("ladder_gmm_", "ladder_mixture_sample", "ladder_emgmm_", "ladder_kmeans_", "ladder_vbgmm_", "ladder_slp_", "ladder_diag_mixture_")
# the one mixture export that is deliberately NOT on the table: the per-row log-density of the diagonal mixture has one form, so nothing selects it
OFF_THE_TABLE = ("ladder_diag_mixture_logprob_rows", "ladder_diag_mixture_logprob_rows_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from ladder_latent_data_distribution_modelling_amd import _lib
    from ladder_latent_data_distribution_modelling_amd.csrc import build
    return _lib.load(build.build(verbose=False))


@pytest.fixture(scope="module")
def F():
    from ladder_latent_data_distribution_modelling_amd import mixture_forms
    return mixture_forms


@pytest.mark.parametrize("op", sorted(EXPECTED))
def test_lookup_gives_the_family_or_the_refusal_of_the_owners_rule(F, op):
    role, rule = EXPECTED[op]
    for R in WIDTHS:
        for K in COUNTS:
            want = rule(K, R)
            if isinstance(want, str):
                assert getattr(F.family(op, K, R), role) == want, (op, K, R)
            else:
                with pytest.raises(want[0]) as e:
                    F.family(op, K, R)
                assert type(e.value) is want[0] and re.match(want[1], str(e.value)), (op, K, R, str(e.value))
    assert sorted(EXPECTED) == sorted(F.FAMILIES)


def test_rows_of_an_operation_share_their_role_names_and_say_their_tiers(F):
    tiers = lambda R: F.family("term", 3, R).tiers
    assert tiers(8) == tiers(0) == ("packed",) and tiers(9) == tiers(64) == ("dense",) and tiers(65) == tiers(256) == tiers(272) == ("wide",)
    for op, rows in F.FAMILIES.items():
        assert all(row.op == op and set(row.tiers) <= {"packed", "dense", "wide"} for row in rows)
        assert all(sorted(vars(row)) == sorted(vars(rows[0])) for row in rows), op     # the same attributes on every row: no owner probes for one
        must = set.intersection(*(set(row.entries) for row in rows))
        assert {"term": {"param_size", "prepare", "workspace_bytes", "fwd_bwd", "logprob_rows"}, "sampler": {"param_bytes", "prepare", "prepare_diag", "sample"},
                "em": {"state_doubles", "stats_doubles", "shift_doubles", "workspace_bytes", "shift", "estep", "mstep", "prepare"},
                "kmeans": {"state_doubles", "draws_doubles", "workspace_bytes", "seed", "set_centres", "assign", "update"},
                "vb": {"state_doubles", "stats_doubles", "workspace_bytes", "moments_doubles", "moments", "estep", "mstep"},
                "slp": {"state_bytes", "optimise"}, "diag_term": {"workspace_bytes", "fwd_bwd"}}[op] == must, op


def test_what_differs_in_calling_convention_is_on_the_row(F):
    packed, dense, wide = F.FAMILIES["term"]
    assert (packed.rows_workspace, dense.rows_workspace, wide.rows_workspace) == (False, True, True)
    assert (packed.prepare_workspace_bytes, dense.prepare_workspace_bytes, wide.prepare_workspace_bytes) == (None, None, "ladder_gmm_wide_prepare_workspace_bytes")
    assert [r.prepare_workspace_bytes for r in F.FAMILIES["sampler"]] == [None, "ladder_mixture_sample_wide_prepare_workspace_bytes"]
    assert [r.factor_workspace_bytes for r in F.FAMILIES["em"]] == [None, "ladder_emgmm_wide_mstep_workspace_bytes"]
    assert [(r.moments_by_pass, r.estep_takes_moments, r.fit) for r in F.FAMILIES["vb"]] == [(False, False, "ladder_vbgmm_fit"), (True, True, None)]
    assert [r.state_doubles for r in F.FAMILIES["vb"]] == ["ladder_vbgmm_state_doubles", "ladder_vbgmm_wide_state_doubles"]
    assert [r.max_points for r in F.FAMILIES["slp"]] == [None, 2048]
    assert all(r.draws_doubles == "ladder_kmeans_draws_doubles" for r in F.FAMILIES["kmeans"])
    assert [(r.workspace_bytes, r.query_takes_L) for r in F.FAMILIES["diag_term"]] == [("ladder_diag_mixture_workspace_bytes", False),
                                                                                     ("ladder_diag_mixture_wide_workspace_bytes", True)]


def test_size_queries_that_answer_zero_agree_with_the_rows(F, lib):
    wide_ok = lambda R: R in WIDE_WIDTHS
    term_wide, (samp, samp_wide), (_, em_wide), (km, km_wide), slp_dense = (F.FAMILIES["term"][2], F.FAMILIES["sampler"], F.FAMILIES["em"], F.FAMILIES["kmeans"],
                                                                             F.FAMILIES["slp"][1])
    for R in WIDTHS:
        assert term_wide.takes(R) == samp_wide.takes(R) == em_wide.takes(R) == km_wide.takes(R) == wide_ok(R), R
        assert samp.takes(R) == km.takes(R) == (1 <= R <= 64), R
        assert slp_dense.takes(R) == (8 < R <= 64 and R % 4 == 0), R
        assert (lib.ladder_emgmm_wide_shift_doubles(R) != 0) == wide_ok(R), R
        assert (lib.ladder_slp_wide_state_bytes(2, 4, R) != 0) == slp_dense.takes(R), R
        for K in COUNTS:
            at = (K, R)
            assert term_wide.takes(R, K) == (wide_ok(R) and 1 <= K <= 1024), at
            for q in (lib.ladder_gmm_wide_param_bytes(K, R), lib.ladder_gmm_wide_prepare_workspace_bytes(K, R), lib.ladder_gmm_wide_workspace_bytes(1, 8, R, K)):
                assert (q != 0) == term_wide.takes(R, K), at
            assert (lib.ladder_mixture_sample_param_bytes(K, R) != 0) == (K >= 1 and samp.takes(R)), at
            assert (lib.ladder_mixture_sample_wide_param_bytes(K, R) != 0) == (K >= 1 and samp_wide.takes(R)), at
            assert (lib.ladder_mixture_sample_wide_prepare_workspace_bytes(K, R) != 0) == (K >= 1 and samp_wide.takes(R)), at
            assert km.takes(R, K) == (1 <= K <= 64 and 1 <= R <= 64) and km_wide.takes(R, K) == (1 <= K <= 64 and wide_ok(R)), at
            assert (lib.ladder_kmeans_state_doubles(K, R) != 0) == km.takes(R, K), at
            assert (lib.ladder_kmeans_wide_state_doubles(K, R) != 0) == km_wide.takes(R, K), at
            assert (lib.ladder_kmeans_wide_workspace_bytes(256, K, R) != 0) == km_wide.takes(R, K), at
            # (the EM rows draw no component limit on this side: the library's is 1 <= K <= 64)
            for q in (lib.ladder_emgmm_wide_state_doubles(K, R), lib.ladder_emgmm_wide_stats_doubles(K, R), lib.ladder_emgmm_wide_workspace_bytes(256, K, R),
                      lib.ladder_emgmm_wide_mstep_workspace_bytes(K, R)):
                assert (q != 0) == (1 <= K <= 64 and em_wide.takes(R)), at
    # Not in the sweep, because they do not answer 0 outside their family's shapes (they refuse K < 1 or R < 1 alone; the launches refuse the rest):
    # the ladder_vbgmm_wide_* size queries (C "wide" = the dense tier: they answer for R = 80 as for R = 16).  That this is so:
    assert lib.ladder_vbgmm_wide_state_doubles(3, 80) != 0 and lib.ladder_vbgmm_wide_stats_doubles(3, 80) != 0 and lib.ladder_vbgmm_wide_moments_doubles(80) != 0
    assert lib.ladder_vbgmm_wide_workspace_bytes(256, 3, 80) != 0
    for R in (12, 36, 64):                                                      # the dense SLP row's bound on n_step * R is the query's
        for n_step in range(1, 65):
            assert (lib.ladder_slp_wide_state_bytes(1, n_step, R) != 0) == (n_step * R <= slp_dense.max_points), (n_step, R)


def test_table_and_prototypes_name_the_same_mixture_entries_each_once(F):
    from ladder_latent_data_distribution_modelling_amd import _lib
    in_table = [name for rows in F.FAMILIES.values() for row in rows for name in row.entries.values()]
    assert sorted(set(in_table)) == F.ENTRY_NAMES and all(name in _lib.PROTOTYPES for name in in_table)
    mixture_exports = sorted(n for n in _lib.PROTOTYPES if n.startswith(MIXTURE_PREFIXES) and n not in OFF_THE_TABLE)
    assert mixture_exports == F.ENTRY_NAMES
    assert all(n in _lib.PROTOTYPES for n in OFF_THE_TABLE) and not any(n in in_table for n in OFF_THE_TABLE)
    assert sorted(n for n in in_table if n.startswith("ladder_diag_mixture_")) == sorted(
        ["ladder_diag_mixture_workspace_bytes", "ladder_diag_mixture_fwd_bwd", "ladder_diag_mixture_wide_workspace_bytes", "ladder_diag_mixture_wide_fwd_bwd"])
    assert len(in_table) == len(set(in_table)) + 1 and in_table.count("ladder_kmeans_draws_doubles") == 2      # the one export two rows share
    with open(F.__file__) as f:
        src = f.read()
    assert [n for n in F.ENTRY_NAMES if src.count('"%s"' % n) != 1] == []       # a plain search finds each name, once
    # ... and nowhere else in the package is one spelt out or put together from pieces
    pkg = os.path.dirname(F.__file__)
    for d, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(".py") and fn not in ("mixture_forms.py", "_lib.py"):
                with open(os.path.join(d, fn)) as f:
                    text = f.read()
                assert not re.search(r'"ladder_[a-z0-9_]*_"|replace\("ladder_', text), fn
                assert [n for n in F.ENTRY_NAMES if '"%s"' % n in text] == [], fn


def test_entry_names_by_width_and_the_limits_derived_from_the_rows(F):
    """What tests/test_emgmm_wide_cpu.py and tests/test_gpu_kmeans_wide.py asserted of `family_prefix`, on the entries the lookup returns."""
    from ladder_latent_data_distribution_modelling_amd.codes import interpolation as I
    from ladder_latent_data_distribution_modelling_amd.codes.vbgmm import NARROW_MAX_R
    em = lambda R: F.family("em", 6, R)
    assert em(64).estep == em(1).estep == "ladder_emgmm_estep" and em(64).prepare == "ladder_emgmm_prepare"
    assert em(80).estep == em(256).estep == "ladder_emgmm_wide_estep" and em(80).prepare == "ladder_emgmm_wide_prepare"
    assert em(64) is em(1) and em(80) is em(256) and em(64) is not em(80)
    for R in (72, 272, 0):
        with pytest.raises(ValueError, match=r"80 \.\. 256 in steps of 16"):
            em(R)
    assert F.family("kmeans", 3, 64).assign == "ladder_kmeans_assign" and F.family("kmeans", 3, 80).assign == "ladder_kmeans_wide_assign"
    assert F.family("kmeans", 3, 64).seed == "ladder_kmeans_seed" and F.family("kmeans", 3, 80).seed == "ladder_kmeans_wide_seed"
    for K, R in ((3, 72), (3, 272), (65, 80)):
        with pytest.raises(NotImplementedError, match=r"n_features <= 64 or 80 <= n_features <= 256"):
            F.family("kmeans", K, R)
    assert F.EM_WIDTH_RULE == "1 .. 64 dimensions, or 80 .. 256 in steps of 16"
    assert NARROW_MAX_R == 8 and I.MAX_POINTS_WIDE == 2048
