"""Which kernel family serves a mixture operation at a given width: the one table the Python side selects from, and `family`, its one lookup.

Tiers, by the width R of the mixture (the words of the Python code): packed R <= 8, dense 8 < R <= 64, wide 64 < R <= 256.  The C names do not
follow them: "wide" in `ladder_vbgmm_wide_*` and `ladder_slp_wide_*` is the dense tier, "wide" in `ladder_gmm_wide_*`, `ladder_mixture_sample_wide_*`,
`ladder_emgmm_wide_*` and `ladder_kmeans_wide_*` the wide tier, and the un-suffixed sampler, EM and k-means entries serve packed and dense alike.
A row names its operation, its tiers, the shapes its family takes (lo <= R <= hi, R % step == 0, 1 <= K <= max_k; None: no bound drawn on this side),
every entry point under a role name shared by the operation's rows, and what differs in how the families are called.  The table selects by tier;
the operations in REFUSALS also hold the shape against the row, the others (the dense term at R = 10, say) are refused by the library, as ever.
"diag_term", the VampPrior's diagonal mixture (mixture.py: DiagMixture), is the one operation that does not select by tier: its wide row serves exactly
the widths that row takes, whatever K, and its narrow row every other width -- 70 too, which the tier rule would call wide -- so that such a model
meets the narrow entry's refusal before any launch, as it always has.
"""
import torch

from . import _lib as L


class Form:
    def __init__(self, op, tiers, lo, hi, step=1, max_k=None, **roles):
        self.op, self.tiers, self.lo, self.hi, self.step, self.max_k = op, tiers, lo, hi, step, max_k
        self.entries = {role: name for role, name in roles.items() if isinstance(name, str)}      # role -> exported name
        self.__dict__.update(roles)

    def takes(self, R, K=1):
        return (self.lo is None or self.lo <= R) and (self.hi is None or R <= self.hi) and R % self.step == 0 and (self.max_k is None or 1 <= K <= self.max_k)


NARROW, WIDE, _KMEANS_DRAWS = ("packed", "dense"), ("wide",), "ladder_kmeans_draws_doubles"       # (the draws are sized by K alone: one export, both families)
FAMILIES = {
    # the ELBO term, log_prob_rows and what SLP reads (mixture.py).  prepare_workspace_bytes: sizes the workspace `prepare` takes (None: takes none);
    # rows_workspace: whether logprob_rows takes one, sized by workspace_bytes
    "term": (
        Form("term", ("packed",), 1, 8, param_size="ladder_gmm_packed_stride", prepare="ladder_gmm_prepare", workspace_bytes="ladder_gmm_workspace_bytes",
             fwd_bwd="ladder_gmm_logprob_fwd_bwd", logprob_rows="ladder_gmm_logprob_rows", prepare_workspace_bytes=None, rows_workspace=False),
        Form("term", ("dense",), 9, 64, 4, param_size="ladder_gmm_dense_param_floats", prepare="ladder_gmm_prepare_dense", workspace_bytes="ladder_gmm_dense_workspace_bytes",
             fwd_bwd="ladder_gmm_dense_logprob_fwd_bwd", logprob_rows="ladder_gmm_dense_logprob_rows", prepare_workspace_bytes=None, rows_workspace=True),
        Form("term", WIDE, 80, 256, 16, 1024, param_size="ladder_gmm_wide_param_bytes", prepare="ladder_gmm_wide_prepare", workspace_bytes="ladder_gmm_wide_workspace_bytes",
             fwd_bwd="ladder_gmm_wide_logprob_fwd_bwd", logprob_rows="ladder_gmm_wide_logprob_rows",
             prepare_workspace_bytes="ladder_gmm_wide_prepare_workspace_bytes", rows_workspace=True)),
    # the VampPrior term (mixture.py: DiagMixture; csrc/diag_mixture.hip).  query_takes_L: the workspace query takes (L, B, Z, K), not (B, Z, K)
    "diag_term": (
        Form("diag_term", NARROW, 1, 64, workspace_bytes="ladder_diag_mixture_workspace_bytes", fwd_bwd="ladder_diag_mixture_fwd_bwd", query_takes_L=False),
        Form("diag_term", WIDE, 80, 256, 16, 1024, workspace_bytes="ladder_diag_mixture_wide_workspace_bytes", fwd_bwd="ladder_diag_mixture_wide_fwd_bwd",
             query_takes_L=True)),
    "sampler": (                                 # ancestral sampling (engine.py: prior_sampler)
        Form("sampler", NARROW, 1, 64, param_bytes="ladder_mixture_sample_param_bytes", prepare="ladder_mixture_sample_prepare",
             prepare_diag="ladder_mixture_sample_prepare_diag", sample="ladder_mixture_sample", prepare_workspace_bytes=None),
        Form("sampler", WIDE, 80, 256, 16, param_bytes="ladder_mixture_sample_wide_param_bytes", prepare="ladder_mixture_sample_wide_prepare",
             prepare_diag="ladder_mixture_sample_wide_prepare_diag", sample="ladder_mixture_sample_wide",
             prepare_workspace_bytes="ladder_mixture_sample_wide_prepare_workspace_bytes")),
    "em": (                                      # the EM fit of prior "GMM" (codes/emgmm.py).  factor_workspace_bytes: sizes what `mstep` and `prepare` take
        Form("em", NARROW, 1, 64, state_doubles="ladder_emgmm_state_doubles", stats_doubles="ladder_emgmm_stats_doubles", shift_doubles="ladder_emgmm_shift_doubles",
             workspace_bytes="ladder_emgmm_workspace_bytes", shift="ladder_emgmm_shift", estep="ladder_emgmm_estep", mstep="ladder_emgmm_mstep",
             prepare="ladder_emgmm_prepare", factor_workspace_bytes=None),
        Form("em", WIDE, 80, 256, 16, state_doubles="ladder_emgmm_wide_state_doubles", stats_doubles="ladder_emgmm_wide_stats_doubles",
             shift_doubles="ladder_emgmm_wide_shift_doubles", workspace_bytes="ladder_emgmm_wide_workspace_bytes", shift="ladder_emgmm_wide_shift",
             estep="ladder_emgmm_wide_estep", mstep="ladder_emgmm_wide_mstep", prepare="ladder_emgmm_wide_prepare",
             factor_workspace_bytes="ladder_emgmm_wide_mstep_workspace_bytes")),
    "kmeans": (                                  # the labels of a cold fit (codes/kmeans.py)
        Form("kmeans", NARROW, 1, 64, 1, 64, state_doubles="ladder_kmeans_state_doubles", draws_doubles=_KMEANS_DRAWS, workspace_bytes="ladder_kmeans_workspace_bytes",
             seed="ladder_kmeans_seed", set_centres="ladder_kmeans_set_centres", assign="ladder_kmeans_assign", update="ladder_kmeans_update"),
        Form("kmeans", WIDE, 80, 256, 16, 64, state_doubles="ladder_kmeans_wide_state_doubles", draws_doubles=_KMEANS_DRAWS,
             workspace_bytes="ladder_kmeans_wide_workspace_bytes", seed="ladder_kmeans_wide_seed", set_centres="ladder_kmeans_wide_set_centres",
             assign="ladder_kmeans_wide_assign", update="ladder_kmeans_wide_update")),
    # the variational fit of prior "ours" (codes/vbgmm.py).  fit: the persistent one-workgroup launch for few samples; moments_by_pass: `moments` takes a
    # pass argument and runs once for pass 0, once for pass 1; estep_takes_moments: `estep` takes the moments pointer
    "vb": (
        Form("vb", ("packed",), None, 8, fit="ladder_vbgmm_fit", fit_workspace_bytes="ladder_vbgmm_workspace_bytes", state_doubles="ladder_vbgmm_state_doubles",
             stats_doubles="ladder_vbgmm_shard_stats_doubles", workspace_bytes="ladder_vbgmm_shard_workspace_bytes",
             moments_doubles="ladder_vbgmm_shard_moments_doubles", moments="ladder_vbgmm_shard_moments", estep="ladder_vbgmm_shard_estep",
             mstep="ladder_vbgmm_shard_mstep", moments_by_pass=False, estep_takes_moments=False),
        Form("vb", ("dense",), 9, 64, fit=None, fit_workspace_bytes=None, state_doubles="ladder_vbgmm_wide_state_doubles",
             stats_doubles="ladder_vbgmm_wide_stats_doubles", workspace_bytes="ladder_vbgmm_wide_workspace_bytes",
             moments_doubles="ladder_vbgmm_wide_moments_doubles", moments="ladder_vbgmm_wide_moments", estep="ladder_vbgmm_wide_estep",
             mstep="ladder_vbgmm_wide_mstep", moments_by_pass=True, estep_takes_moments=True)),
    "slp": (                                     # shortest-likely-path interpolation on the term's buffer (codes/interpolation.py).  max_points: bounds n_step * R
        Form("slp", ("packed",), None, 8, state_bytes="ladder_slp_state_bytes", optimise="ladder_slp_optimise", max_points=None),
        Form("slp", ("dense",), 9, 64, 4, state_bytes="ladder_slp_wide_state_bytes", optimise="ladder_slp_wide_optimise", max_points=2048)),
}
ENTRY_NAMES = sorted({name for rows in FAMILIES.values() for row in rows for name in row.entries.values()})
assert all(name in L.PROTOTYPES for name in ENTRY_NAMES), [name for name in ENTRY_NAMES if name not in L.PROTOTYPES]
(EM_NARROW, EM_WIDE), (KM_NARROW, KM_WIDE), (VB_PACKED, VB_DENSE), (SLP_PACKED, SLP_DENSE) = (FAMILIES[op] for op in ("em", "kmeans", "vb", "slp"))
EM_WIDTH_RULE = "1 .. %d dimensions, or %d .. %d in steps of %d" % (EM_NARROW.hi, EM_WIDE.lo, EM_WIDE.hi, EM_WIDE.step)
# The operations whose lookup refuses a shape no row takes ("term" and "sampler": their owners raise when the selected family's size query answers 0)
REFUSALS = {
    "em": lambda K, R: ValueError("the device EM fit takes samples of %s, got %d" % (EM_WIDTH_RULE, R)),
    "kmeans": lambda K, R: NotImplementedError(
        "the HIP k-means covers 1 <= n_clusters <= %d and 1 <= n_features <= %d or %d <= n_features <= %d in steps of %d, got %d and %d"
        % (KM_NARROW.max_k, KM_NARROW.hi, KM_WIDE.lo, KM_WIDE.hi, KM_WIDE.step, K, R)),
    "vb": lambda K, R: ValueError("the HIP mixture fit takes a representation of at most %d dimensions, got %d" % (VB_DENSE.hi, R)),
    "slp": lambda K, R: ValueError("SLPInterpolator: the wide mixture (R > 8) needs R %% 4 == 0 and R <= 64 (got R = %d)" % R),
}


def family(op, K, R):
    """The row of `op` that serves K components on R dimensions; raises what the owner of `op` has always raised where there is none."""
    if op == "diag_term":                                    # by the wide row's width rule alone (module docstring)
        narrow, wide = FAMILIES[op]
        return wide if wide.takes(R) else narrow
    tier = "packed" if R <= 8 else "dense" if R <= 64 else "wide"
    row = next((r for r in FAMILIES[op] if tier in r.tiers), None)
    if op in REFUSALS and (row is None or not row.takes(R, K)):
        raise REFUSALS[op](K, R)
    return row


def sized_workspace(query, device, *shape):
    """-> (byte tensor sized by the export `query` for `shape`, its (pointer, bytes) as a launch takes them); (None, ()) for a row that names no query."""
    if query is None:
        return None, ()
    ws = torch.empty(L.query(query, *shape), dtype=torch.uint8, device=device)
    return ws, (ws.data_ptr(), ws.numel())


def check_status_word(buf, noun, cause):
    """Reads (and so waits for) the status `prepare` left in the first word of `buf`: -1 usable, k >= 0 no Cholesky factor of component k, else bad weights."""
    status = int(buf[:4].view(torch.int32).item())
    if status >= 0:
        raise ValueError("component %d of the %s has no Cholesky factor (%s not positive definite)" % (status, noun, cause))
    if status != -1:
        raise ValueError("the weights of the %s have no positive finite sum" % noun)
