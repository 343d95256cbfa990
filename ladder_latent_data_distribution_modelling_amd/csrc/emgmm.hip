// EM fit of the baseline "GMM" prior on the device (reference codes/base.py:101-106, 699-710, 749-767):
// sklearn.mixture.GaussianMixture(covariance_type="full", init_params="kmeans") restated in float64 for 1 <= R <= 64, 1 <= K <= 64 -- the functions
// _estimate_gaussian_parameters, _compute_precision_cholesky, _estimate_log_gaussian_prob, _m_step and the loop of BaseMixture.fit_predict.
//
// One EM iteration `it` (0 = the M-step on the hard k-means labels, then 1 .. max_iter) is
//   emgmm_estep_kernel     fit_estep_slice under the policy EmEstep: a workgroup owns 64 samples; per component k it stages the upper-triangular P_k = precisions_cholesky_[k] in LDS, forms
//                          y = (x - mu_k) P_k on v_mfma_f64_16x16x4_f64 (the all-zero 16 x 16 blocks below the diagonal are skipped) and reduces |y|^2 per
//                          row; after the last k: logsumexp per row, responsibilities [N, K] float64, the slice's sum of log_prob_norm.
//                          it = 0: the responsibilities are the one-hot labels.
//   fit_stats_kernel       grid (component, row split): n_k, sum r x~ and the 16 x 16 blocks on and above the diagonal of sum r x~ x~^T on the same MFMA,
//                          x~ = x - c with ONE shift vector c for all components (the fp32-rounded global mean: x - c is exact in float64 and the raw
//                          second moments carry no uncentred cancellation); partials go to the workspace
//   fit_reduce_kernel      adds the partials in the order split 0, 1, ... (and the slices' log_prob_norm sums in slice order) into
//                          stats = [ sum log_prob_norm | n_k [K] | sum r x~ [K,R] | sum r x~ x~^T [K,R,R] ]; the lower triangle mirrors the upper one
//   (all-reduce of stats over the data-parallel ranks, by the caller: the lower bound is a GLOBAL mean, so its sum travels with the rest)
//   emgmm_mstep_kernel     one workgroup per component: weight, mean, covariance centred from the shifted raw moments + reg_covar
//                          (fit_centre_mean / fit_centred_cov), Cholesky factor,
//                          its triangular inverse (precisions_cholesky_), log-determinant, fp32 copies for the engine's feed
//   emgmm_finish_kernel    fit_end_iteration with lower_bound = sum log_prob_norm / N of THIS iteration's E-step: |change| < tol, n_iter_,
//                          converged_ and the `done` flag
// Every kernel returns at once when `done` is set, so the host may enqueue iterations ahead and read the flag every few iterations (the contract of
// ladder_vbgmm_shard_*).  No atomics: every sum has one fixed order, so a fit gives the same bits on every run and for every `check_every`.
//
// The state layout (EmState) and emgmm_finish_kernel are csrc/em_state.h's, shared with the fit for 80 <= R <= 256 (csrc/emgmm_wide.hip).
//
// All but the policy, the M-step's own arithmetic and the state layout is shared with the wide variational fit of csrc/vbgmm.hip: the E-step body,
// the column-sum / statistics / reduce kernels, the host side of the E-step, the centring and the factorisation in csrc/fit_mfma.h, the `done`
// test and the end of an iteration in csrc/fit_util.h.
#include "em_state.h"
#include "fit_mfma.h"

namespace {

// ------------------------------------------------------------------------------------------------ E-step
// _estimate_weighted_log_prob and _estimate_log_prob_resp as the policy of fit_estep_slice: constants log|P_k| and log w_k, the slice scalar is
// the sum of log_prob_norm.
struct EmEstep {
  static constexpr int NCONST = 2;
  const double *logdet, *w;
  int R;
  __device__ void load(double* s_c, int k) const {
    s_c[k] = logdet[k];
    s_c[FIT_MAXK + k] = log(w[k]);
  }
  __device__ double log_term(const double* s_c, int k, double q) const { return (-0.5 * (R * kLog2Pi + q) + s_c[k]) + s_c[FIT_MAXK + k]; }
  __device__ double finish_row(double* wr, int K, double lpn) const {
    for (int k = 0; k < K; ++k) wr[k] = exp(wr[k] - lpn);
    return lpn;
  }
};

__global__ __launch_bounds__(256) void emgmm_estep_kernel(const float* __restrict__ X, const int* __restrict__ labels, const double* state, int N, int K,
                                                          int R, double* resp, double* __restrict__ lpn_part) {
  EmState S(const_cast<double*>(state), K, R);
  if (fit_done(S.tail)) return;
  fit_estep_slice(EmEstep{S.logdet, S.w, R}, X, labels, S.pchol, S.means, N, K, R, resp, lpn_part);
}

// ------------------------------------------------------------------------------------------------ M-step
// _compute_precision_cholesky for one component, by ONE wavefront (64 threads): A [R][FIT_LDC] in LDS holds the covariance on entry (fit_chol_inverse).
// Writes precisions_cholesky_[k] (upper triangular), its log-determinant and the component status (-1: a non-positive pivot).
__device__ void em_prepare_component(double* A, int R, int k, EmState& S, int tid) {
  const bool bad = fit_chol_inverse(A, R, S.pchol + (size_t)k * R * R, tid);
  if (tid == 0) {
    double ld = 0.0;
    for (int j = 0; j < R; ++j) ld += log(1.0 / A[j * FIT_LDC + j]);
    S.logdet[k] = ld;
    S.cstat[k] = bad ? -1.0 : 0.0;
  }
}

__global__ __launch_bounds__(64) void emgmm_mstep_kernel(const double* __restrict__ stats, const double* __restrict__ mom, double* state, int K, int R,
                                                         double reg_covar, int it, float* __restrict__ w_out, float* __restrict__ m_out,
                                                         float* __restrict__ c_out) {
  EmState S(state, K, R);
  if (fit_done(S.tail)) return;
  const int k = blockIdx.x, tid = threadIdx.x;
  __shared__ double s_A[FIT_MAXR * FIT_LDC], s_s1[FIT_MAXR], s_dm[FIT_MAXR];
  const FitStats<const double> st(stats, K, R, k);
  const double nk_raw = st.nk[k], nk = nk_raw + kEps10;            // nk = resp.sum(axis=0) + 10 * eps
  if (tid == 0) {
    double w;
    if (it == 0) {
      w = nk / mom[R];                                             // _initialize: weights = nk / n_samples
    } else {
      double tot = 0.0;                                            // _m_step: weights_ = nk; weights_ /= weights_.sum()
      for (int j = 0; j < K; ++j) tot += st.nk[j] + kEps10;
      w = nk / tot;
    }
    S.w[k] = w;
    w_out[k] = (float)w;
  }
  if (tid < R) {
    const double mean = fit_centre_mean(mom, R, tid, st.x[tid], nk_raw, nk, s_s1, s_dm);
    S.means[k * R + tid] = mean;
    m_out[k * R + tid] = (float)mean;
  }
  __syncthreads();
  double* C = S.cov + (size_t)k * R * R;                           // [i][j] for i <= j, mirrored
  float* Cf = c_out + (size_t)k * R * R;
  for (int e = tid; e < R * R; e += 64) {
    const int i = e / R, j = e - i * R;
    if (j < i) continue;
    const double v = fit_centred_cov(st.xx[e], s_s1, s_dm, i, j, nk_raw, nk, reg_covar);
    s_A[i * FIT_LDC + j] = v;
    s_A[j * FIT_LDC + i] = v;
    C[i * R + j] = v;
    C[j * R + i] = v;
    Cf[i * R + j] = (float)v;
    Cf[j * R + i] = (float)v;
  }
  __syncthreads();
  em_prepare_component(s_A, R, k, S, tid);
}

// precisions_cholesky_ / log-determinant / status of the covariances already IN the state (parameters set from outside)
__global__ __launch_bounds__(64) void emgmm_prepare_kernel(double* state, int K, int R) {
  EmState S(state, K, R);
  const int k = blockIdx.x, tid = threadIdx.x;
  __shared__ double s_A[FIT_MAXR * FIT_LDC];
  const double* C = S.cov + (size_t)k * R * R;
  for (int e = tid; e < R * R; e += 64) s_A[(e / R) * FIT_LDC + (e % R)] = C[e];
  __syncthreads();
  em_prepare_component(s_A, R, k, S, tid);
}

}  // namespace

extern "C" {

size_t ladder_emgmm_state_doubles(int K, int R) { return (K < 1 || R < 1) ? 0 : em_state_doubles(K, R); }
size_t ladder_emgmm_stats_doubles(int K, int R) { return (K < 1 || R < 1) ? 0 : fit_stats_doubles(K, R); }
size_t ladder_emgmm_shift_doubles(int R) { return R < 1 ? 0 : (size_t)R + 1; }

size_t ladder_emgmm_workspace_bytes(int N, int K, int R) { return fit_sliced_workspace_bytes(N, K, R); }

int ladder_emgmm_shift(const float* X, int N, int R, double* moments, ladder_stream_t stream) {
  if (X == nullptr || moments == nullptr || N < 1 || R < 1 || R > FIT_MAXR) return LADDER_E_SHAPE;
  if (fit_misaligned(moments)) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(fit_colsum_kernel, dim3(R), dim3(256), 0, stream, X, N, R, moments);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_emgmm_estep(const float* X, int N, int K, int R, const int* labels, const double* state, const double* moments, double* stats, void* ws,
                       size_t ws_bytes, ladder_stream_t stream) {
  return fit_sliced_estep(emgmm_estep_kernel, false, X, N, K, R, labels, state, em_state_doubles(K, R), moments, stats, ws, ws_bytes,
                          stream);
}

int ladder_emgmm_mstep(const double* stats, const double* moments, int K, int R, double* state, double reg_covar, double tol, int max_iter, int it,
                       float* weights, float* means, float* covs, ladder_stream_t stream) {
  if (stats == nullptr || moments == nullptr || state == nullptr || weights == nullptr || means == nullptr || covs == nullptr || K < 1 || K > FIT_MAXK ||
      R < 1 || R > FIT_MAXR || max_iter < 0 || it < 0)
    return LADDER_E_SHAPE;
  if (fit_misaligned(stats) || fit_misaligned(moments) || fit_misaligned(state)) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(emgmm_mstep_kernel, dim3(K), dim3(64), 0, stream, stats, moments, state, K, R, reg_covar, it, weights, means, covs);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(emgmm_finish_kernel, dim3(1), dim3(64), 0, stream, stats, moments, state, K, R, tol, max_iter, it);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_emgmm_prepare(double* state, int K, int R, ladder_stream_t stream) {
  if (state == nullptr || K < 1 || K > FIT_MAXK || R < 1 || R > FIT_MAXR) return LADDER_E_SHAPE;
  if (fit_misaligned(state)) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(emgmm_prepare_kernel, dim3(K), dim3(64), 0, stream, state, K, R);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(emgmm_finish_kernel, dim3(1), dim3(64), 0, stream, (const double*)nullptr, (const double*)nullptr, state, K, R, 0.0, 0, -1);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
