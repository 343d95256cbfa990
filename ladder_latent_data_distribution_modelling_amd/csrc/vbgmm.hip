// Variational Bayesian Gaussian mixture fit on the device: the producer of the hyper-prior feed
// (prior_weight, prior_mean, prior_cov), i.e. what the reference gets from sklearn.mixture.BayesianGaussianMixture(
// n_components=K, covariance_type='full', weight_concentration_prior_type='dirichlet_distribution' | 'dirichlet_process',
// weight_concentration_prior=0.1, warm_start=True).fit(t_samples)  (codes/base.py:93-99, 681-789).
//
// The problem is tiny and strictly sequential (N ~ 2e3..2e4 samples of R <= 8 dims, K <= 64 components, 10..1000 dependent E/M
// iterations; a representation of 9 .. 64 dims takes the vbwide_* kernels at the end of this file, on the float64 MFMA).  Arithmetic is float64 like sklearn's; every reduction has one fixed order, so a fit gives the same bits on every run
// and on every rank.  Two paths call the SAME device functions (vb_*) for all that sklearn defines -- the E-step, the
// Dirichlet / Wishart update with its Cholesky and inverse, the lower bound, _set_parameters (the wide fit calls vb_digamma, vb_estep_constant,
// vb_log_wishart_term, vb_lower_bound and vb_write_feed too, and takes its E-step body, statistics, centring and factorisation from
// csrc/fit_mfma.h); the one-hot start, the `done` test and the end of an iteration (fit_end_iteration) are those of csrc/fit_util.h, which the EM
// fit of csrc/emgmm.hip follows too:
//   vbgmm_fit_kernel                   below 1 024 samples: ONE persistent workgroup of 16 wavefronts keeps the whole VB loop in one launch
//   vbgmm_shard_{estep,mstep}_kernel   every other fit: an E-step launch over 256-sample slices + an M-step launch per iteration, the samples
//                                      possibly sharded over the data-parallel ranks
// They differ in ONE thing, the statistics pass: the persistent kernel centres the second moments before summing, as sklearn does; the
// sharded path sums raw moments (additive over slices and ranks) and centres them in the M-step (the two forms agree to ~1e-13).
// The functions are forced-inline and restate sklearn 1.7's _bayesian_mixture.py / _gaussian_mixture.py (BSD-3) in sklearn's evaluation
// order -- do not reorder a sum or merge (x - mu) P: -ffp-contract=fast fuses by what surrounds a statement.  tests/test_gpu_vbgmm.py
// compares against sklearn itself through its public API.
#include "fit_mfma.h"

namespace {

constexpr int VB_THREADS = 1024, VB_WAVES = VB_THREADS / 64, VB_MAXK = 64, VB_MAXR = 8;

struct VbCfg {
  int N, K, R, prior_type, max_iter, init_from_labels;
  double wc_prior, mean_prec_prior, reg_covar, tol;
};

__device__ double vb_digamma(double x) {
  double r = 0.0;
  while (x < 10.0) {
    r -= 1.0 / x;
    x += 1.0;
  }
  const double f = 1.0 / (x * x);
  // asymptotic series: ln x - 1/(2x) - sum B_2n / (2n x^2n)
  const double t = f * (-1.0 / 12.0 + f * (1.0 / 120.0 + f * (-1.0 / 252.0 + f * (1.0 / 240.0 + f * (-1.0 / 132.0 +
                   f * (691.0 / 32760.0 + f * (-1.0 / 12.0)))))));
  return r + log(x) - 0.5 / x + t;
}

// state layout (doubles): wa[K] wb[K] mean_prec[K] dof[K] means[K*R] cov[K*R*R] prec_chol[K*R*R] | the four tail doubles of fit_util.h
// The wide fit (R > 8, below) keeps `extra` = 2 more doubles per component before the tail: the E-step constants ck[K] and the
// factorisation status cstat[K].
struct VbState {
  double *wa, *wb, *mprec, *dof, *means, *cov, *pchol, *ck, *cstat, *tail;
  __device__ VbState(double* s, int K, int R, int extra = 0) {
    wa = s; wb = wa + K; mprec = wb + K; dof = mprec + K; means = dof + K; cov = means + (size_t)K * R;
    pchol = cov + (size_t)K * R * R; ck = pchol + (size_t)K * R * R; cstat = ck + K; tail = ck + (size_t)extra * K;
  }
};

// ---------------------------------------------------------------------------------------------------------------- shared by both paths
// What _estimate_log_prob + _estimate_log_weights give per component, all but the quadratic form: Pk = precisions_cholesky_[k] (global memory or an
// LDS copy), dig_sum = digamma(sum_k wa) (dirichlet_distribution only).  s_stick, if given, holds digamma(wb_j) - digamma(wa_j + wb_j) per component:
// the stick-breaking prefix adds the same terms in the same order either way.
__device__ __forceinline__ double vb_estep_constant(int k, const double* Pk, const VbState& S, const VbCfg& c, double dig_sum,
                                                    const double* s_stick = nullptr) {
  const int R = c.R;
  double log_det = 0.0, log_lambda = R * log(2.0);
  for (int j = 0; j < R; ++j) {
    log_det += log(Pk[j * R + j]);
    log_lambda += vb_digamma(0.5 * (S.dof[k] - j));
  }
  double lw;
  if (c.prior_type == 0) {
    lw = vb_digamma(S.wa[k]) - dig_sum;
  } else {            // stick breaking: digamma(a) - digamma(a+b) + sum_{j<k} (digamma(b_j) - digamma(a_j+b_j))
    lw = vb_digamma(S.wa[k]) - vb_digamma(S.wa[k] + S.wb[k]);
    if (s_stick != nullptr)
      for (int j = 0; j < k; ++j) lw += s_stick[j];
    else
      for (int j = 0; j < k; ++j) lw += vb_digamma(S.wb[j]) - vb_digamma(S.wa[j] + S.wb[j]);
  }
  return -0.5 * R * log(2.0 * M_PI) + log_det - 0.5 * R * log(S.dof[k]) + 0.5 * (log_lambda - R / S.mprec[k]) + lw;
}

// The E-step on the N rows of X (_estimate_log_prob_resp): resp <- responsibilities; returns sum r log r in thread 0 (0 elsewhere).
// EVERY thread of the VB_THREADS must call it (three barriers); s_scal: 1, s_red: VB_WAVES doubles of LDS.
__device__ __forceinline__ double vb_estep(const float* __restrict__ X, int N, const VbState& S, const VbCfg& c, double* s_mu, double* s_pc,
                                           double* s_ck, double* s_scal, double* s_red, double* __restrict__ resp, int tid) {
  const int K = c.K, R = c.R;
  if (tid == 0 && c.prior_type == 0) {
    double sw = 0.0;
    for (int k = 0; k < K; ++k) sw += S.wa[k];
    s_scal[0] = vb_digamma(sw);
  }
  for (int i = tid; i < K * R; i += VB_THREADS) s_mu[i] = S.means[i];
  for (int i = tid; i < K * R * R; i += VB_THREADS) s_pc[i] = S.pchol[i];
  __syncthreads();
  if (tid < K) s_ck[tid] = vb_estep_constant(tid, s_pc + (size_t)tid * R * R, S, c, s_scal[0]);
  __syncthreads();
  double ent = 0.0;
  for (int n = tid; n < N; n += VB_THREADS) {
    double x[VB_MAXR];
    for (int i = 0; i < R; ++i) x[i] = (double)X[(size_t)n * R + i];
    double* wr = resp + (size_t)n * K;
    double mx = -INFINITY;
    for (int k = 0; k < K; ++k) {
      const double* P = s_pc + (size_t)k * R * R;
      const double* mu = s_mu + k * R;
      double q = 0.0;
      for (int j = 0; j < R; ++j) {
        double xy = 0.0, my = 0.0;                    // y = X @ prec_chol - mu @ prec_chol, as sklearn evaluates it
        for (int i = 0; i <= j; ++i) {
          xy += x[i] * P[i * R + j];
          my += mu[i] * P[i * R + j];
        }
        const double y = xy - my;
        q += y * y;
      }
      const double w = s_ck[k] - 0.5 * q;
      wr[k] = w;
      mx = fmax(mx, w);
    }
    double se = 0.0;
    for (int k = 0; k < K; ++k) se += exp(wr[k] - mx);
    const double lse = mx + log(se);
    for (int k = 0; k < K; ++k) {
      const double lr = wr[k] - lse, r = exp(lr);
      wr[k] = r;
      ent += r * lr;
    }
  }
  ent = wave_sum_d(ent);                                          // the shuffle tree, then the wavefronts in the order 0, 1, ...
  if ((tid & 63) == 0) s_red[tid >> 6] = ent;
  __syncthreads();
  double entropy = 0.0;
  if (tid == 0)
    for (int w = 0; w < VB_WAVES; ++w) entropy += s_red[w];
  return entropy;
}

// _m_step for component k from nk, xk and the CENTRED empirical covariance sk (+ reg_covar): _estimate_weights, _estimate_means,
// _estimate_wishart_full, _compute_precision_cholesky.  One thread per component; s_sk[k] is reused as scratch for the Cholesky factor.
// A non-positive pivot (ill-defined empirical covariance, sklearn raises) sets *s_flag, between the factorisation and the inverse.
__device__ __forceinline__ void vb_update_component(int k, const VbState& S, const VbCfg& c, const double* s_nk, const double* s_xk, double* s_sk,
                                                    const double* s_prior_mean, const double* s_prior_cov, int* s_flag) {
  const int K = c.K, R = c.R;
  const double nk = s_nk[k];
  if (c.prior_type == 0) {
    S.wa[k] = c.wc_prior + nk;                                    // dirichlet_distribution
    S.wb[k] = 0.0;
  } else {
    double tail = 0.0;                                            // sum_{j>k} nk_j
    for (int j = K - 1; j > k; --j) tail += s_nk[j];
    S.wa[k] = 1.0 + nk;
    S.wb[k] = c.wc_prior + tail;
  }
  const double mp = c.mean_prec_prior + nk;
  S.mprec[k] = mp;
  for (int r = 0; r < R; ++r) S.means[k * R + r] = (c.mean_prec_prior * s_prior_mean[r] + nk * s_xk[k * R + r]) / mp;
  const double dof = (double)R + nk;                              // degrees_of_freedom_prior_ = n_features
  S.dof[k] = dof;
  double* C = S.cov + (size_t)k * R * R;
  for (int i = 0; i < R; ++i)
    for (int j = 0; j < R; ++j) {
      const double di = s_xk[k * R + i] - s_prior_mean[i], dj = s_xk[k * R + j] - s_prior_mean[j];
      C[i * R + j] = (s_prior_cov[i * R + j] + nk * s_sk[(k * R + i) * R + j] + nk * c.mean_prec_prior / mp * (di * dj)) / dof;
    }
  // precisions_cholesky_ = solve_triangular(cholesky(cov, lower), I, lower).T   (s_sk slot reused as scratch for L)
  double* Lm = s_sk + (size_t)k * R * R;
  bool ok = true;
  for (int j = 0; j < R; ++j) {
    double d = C[j * R + j];
    for (int p = 0; p < j; ++p) d -= Lm[j * R + p] * Lm[j * R + p];
    if (!(d > 0.0)) { ok = false; d = 1.0; }
    const double ljj = sqrt(d);
    Lm[j * R + j] = ljj;
    for (int i = j + 1; i < R; ++i) {
      double v = C[i * R + j];
      for (int p = 0; p < j; ++p) v -= Lm[i * R + p] * Lm[j * R + p];
      Lm[i * R + j] = v / ljj;
    }
  }
  if (!ok) atomicExch(s_flag, 1);
  double* Pk = S.pchol + (size_t)k * R * R;
  for (int col = 0; col < R; ++col) {                             // column `col` of L^-1 by forward substitution
    for (int i = 0; i < R; ++i) {
      double v = (i == col) ? 1.0 : 0.0;
      for (int p = col; p < i; ++p) v -= Lm[i * R + p] * Pk[col * R + p];   // Pk[col][p] = (L^-1)[p][col] (transposed store)
      Pk[col * R + i] = (i < col) ? 0.0 : v / Lm[i * R + i];
    }
  }
}

// Component k's term of _log_wishart_norm, as _compute_lower_bound sums it.
__device__ __forceinline__ double vb_log_wishart_term(int k, const VbState& S, const VbCfg& c) {
  const int R = c.R;
  const double* Pk = S.pchol + (size_t)k * R * R;
  double ld = 0.0, lg = 0.0;
  for (int j = 0; j < R; ++j) {
    ld += log(Pk[j * R + j]);
    lg += lgamma(0.5 * (S.dof[k] - j));
  }
  ld -= 0.5 * R * log(S.dof[k]);
  return -(S.dof[k] * ld + S.dof[k] * R * 0.5 * log(2.0) + lg);
}

// _compute_lower_bound (log-Wishart, log-norm-weight) from the updated state and this iteration's sum r log r.  One thread.  s_lw, if given,
// holds vb_log_wishart_term per component (computed by a thread each): the sum over the components keeps its order.
__device__ __forceinline__ double vb_lower_bound(const VbState& S, const VbCfg& c, double entropy, const double* s_lw = nullptr) {
  const int K = c.K, R = c.R;
  double log_wishart = 0.0, sum_log_mp = 0.0, log_norm_weight;
  for (int k = 0; k < K; ++k) {
    log_wishart += s_lw != nullptr ? s_lw[k] : vb_log_wishart_term(k, S, c);
    sum_log_mp += log(S.mprec[k]);
  }
  if (c.prior_type == 0) {
    double sw = 0.0, sl = 0.0;
    for (int k = 0; k < K; ++k) { sw += S.wa[k]; sl += lgamma(S.wa[k]); }
    log_norm_weight = lgamma(sw) - sl;
  } else {
    double sb = 0.0;
    for (int k = 0; k < K; ++k) sb += lgamma(S.wa[k]) + lgamma(S.wb[k]) - lgamma(S.wa[k] + S.wb[k]);   // betaln
    log_norm_weight = -sb;
  }
  return -entropy - log_wishart - log_norm_weight - 0.5 * R * sum_log_mp;
}

// _set_parameters: the normalised weights_ (thread 0; s_ck is scratch) and the float32 copies for the mixture feed
__device__ __forceinline__ void vb_write_feed(const VbState& S, const VbCfg& c, double* s_ck, float* __restrict__ w_out, float* __restrict__ m_out,
                                              float* __restrict__ c_out, int tid, int nthreads) {
  const int K = c.K, R = c.R;
  if (tid == 0) {
    double tot = 0.0;
    if (c.prior_type == 0) {
      for (int k = 0; k < K; ++k) tot += S.wa[k];
      for (int k = 0; k < K; ++k) w_out[k] = (float)(S.wa[k] / tot);
    } else {
      double prod = 1.0;
      for (int k = 0; k < K; ++k) {
        const double s = S.wa[k] + S.wb[k];
        s_ck[k] = S.wa[k] / s * prod;
        prod *= S.wb[k] / s;
        tot += s_ck[k];
      }
      for (int k = 0; k < K; ++k) w_out[k] = (float)(s_ck[k] / tot);
    }
  }
  for (int i = tid; i < K * R; i += nthreads) m_out[i] = (float)S.means[i];
  for (int i = tid; i < K * R * R; i += nthreads) c_out[i] = (float)S.cov[i];
}

__global__ __launch_bounds__(VB_THREADS) void vbgmm_fit_kernel(const float* __restrict__ X, const int* __restrict__ labels, double* __restrict__ state, VbCfg c,
                                                               double* __restrict__ resp, float* __restrict__ w_out, float* __restrict__ m_out,
                                                               float* __restrict__ c_out) {
  const int N = c.N, K = c.K, R = c.R, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  VbState S(state, K, R);
  __shared__ double s_nk[VB_MAXK], s_ck[VB_MAXK], s_xk[VB_MAXK * VB_MAXR], s_mu[VB_MAXK * VB_MAXR];
  __shared__ double s_pc[VB_MAXK * VB_MAXR * VB_MAXR];          // precisions_cholesky_ (upper triangular), E-step operand
  __shared__ double s_sk[VB_MAXK * VB_MAXR * VB_MAXR];          // empirical covariances (M-step)
  __shared__ double s_prior_mean[VB_MAXR], s_prior_cov[VB_MAXR * VB_MAXR];
  __shared__ double s_red[VB_WAVES], s_scal[4];
  __shared__ int s_flag;
  // ---- priors from the data, as _check_parameters(X) does on every fit: mean_prior_ = X.mean(0), covariance_prior_ = cov(X.T)
  for (int r = wave; r < R; r += VB_WAVES) {
    double a = 0.0;
    for (int n = lane; n < N; n += 64) a += (double)X[(size_t)n * R + r];
    a = wave_sum_d(a);
    if (lane == 0) s_prior_mean[r] = a / N;
  }
  __syncthreads();
  for (int p = wave; p < R * R; p += VB_WAVES) {
    const int i = p / R, j = p - i * R;
    double a = 0.0;
    for (int n = lane; n < N; n += 64)
      a += ((double)X[(size_t)n * R + i] - s_prior_mean[i]) * ((double)X[(size_t)n * R + j] - s_prior_mean[j]);
    a = wave_sum_d(a);
    if (lane == 0) s_prior_cov[p] = a / (N - 1);
  }
  if (c.init_from_labels) fit_onehot(labels, N, K, resp, tid, VB_THREADS);
  __syncthreads();
  double lower_bound = c.init_from_labels ? -INFINITY : S.tail[FIT_LB];
  int n_iter = 0, converged = 0;
  // iteration 0 = _initialize(X, resp) (M-step on the one-hot responsibilities); a warm start skips it.
  for (int it = c.init_from_labels ? 0 : 1; it <= c.max_iter; ++it) {
    double entropy = 0.0;      // sum_nk resp * log_resp of this iteration's E-step (thread 0)
    if (it > 0) entropy = vb_estep(X, N, S, c, s_mu, s_pc, s_ck, s_scal, s_red, resp, tid);
    // M-step: _estimate_gaussian_parameters, the second moments CENTRED before they are summed (as sklearn does)
    for (int k = wave; k < K; k += VB_WAVES) {
      double a = 0.0;
      for (int n = lane; n < N; n += 64) a += resp[(size_t)n * K + k];
      a = wave_sum_d(a);
      if (lane == 0) s_nk[k] = a + kEps10;
    }
    __syncthreads();
    for (int p = wave; p < K * R; p += VB_WAVES) {
      const int k = p / R, r = p - k * R;
      double a = 0.0;
      for (int n = lane; n < N; n += 64) a += resp[(size_t)n * K + k] * (double)X[(size_t)n * R + r];
      a = wave_sum_d(a);
      if (lane == 0) s_xk[p] = a / s_nk[k];
    }
    __syncthreads();
    const int npair = R * (R + 1) / 2;
    for (int p = wave; p < K * npair; p += VB_WAVES) {
      const int k = p / npair;
      int q = p - k * npair, i = 0;
      while (q >= R - i) { q -= R - i; ++i; }
      const int j = i + q;
      double a = 0.0;
      for (int n = lane; n < N; n += 64)
        a += resp[(size_t)n * K + k] * ((double)X[(size_t)n * R + i] - s_xk[k * R + i]) * ((double)X[(size_t)n * R + j] - s_xk[k * R + j]);
      a = wave_sum_d(a);
      if (lane == 0) {
        a = a / s_nk[k] + (i == j ? c.reg_covar : 0.0);
        s_sk[(k * R + i) * R + j] = a;
        s_sk[(k * R + j) * R + i] = a;
      }
    }
    __syncthreads();
    if (tid == 0) s_flag = 0;
    __syncthreads();
    if (tid < K) vb_update_component(tid, S, c, s_nk, s_xk, s_sk, s_prior_mean, s_prior_cov, &s_flag);
    __syncthreads();
    if (s_flag) {
      if (tid == 0) { S.tail[FIT_LB] = lower_bound; S.tail[FIT_NITER] = n_iter; S.tail[FIT_CONVERGED] = -1.0; }
      return;
    }
    if (it == 0) continue;
    if (tid == 0) {                                                  // lower bound + convergence
      const double lb = vb_lower_bound(S, c, entropy);
      s_scal[1] = lb;
      s_flag = fabs(lb - lower_bound) < c.tol ? 2 : 0;
    }
    __syncthreads();
    lower_bound = s_scal[1];
    n_iter = it;
    if (s_flag == 2) { converged = 1; break; }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) { S.tail[FIT_LB] = lower_bound; S.tail[FIT_NITER] = n_iter; S.tail[FIT_CONVERGED] = converged; }
  vb_write_feed(S, c, s_ck, w_out, m_out, c_out, tid, VB_THREADS);
}

// The SHARDED fit (data-parallel exchange step C5, round 3): every rank keeps only ITS samples.  One variational iteration =
//   vbgmm_shard_estep_kernel   E-step on the local samples with the (replicated) current parameters + the local SUFFICIENT STATISTICS
//                              stats = [ sum r log r | n_k | sum_n r_nk x_n | sum_n r_nk x_n x_n^T ]   (1 + K + K R + K R R doubles)
//   all-reduce(stats)          over RCCL / xGMI by the host (torch.distributed; a few KB)
//   vbgmm_shard_mstep_kernel   M-step from the GLOBAL statistics, lower bound, convergence test -- identical on every rank
// The priors sklearn takes from the data (mean_prior_ = X.mean(0), covariance_prior_ = cov(X.T)) come from all-reduced raw moments.  Both
// kernels return at once when the state's `done` flag is set: the host may enqueue iterations ahead and read the flag every few iterations.
__global__ __launch_bounds__(VB_THREADS) void vbgmm_moments_kernel(const float* __restrict__ X, int N, int R, double* __restrict__ out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) out[0] = (double)N;
  for (int p = wave; p < R + R * R; p += VB_WAVES) {
    double a = 0.0;
    if (p < R) {
      for (int n = lane; n < N; n += 64) a += (double)X[(size_t)n * R + p];
    } else {
      const int i = (p - R) / R, j = (p - R) - i * R;
      for (int n = lane; n < N; n += 64) a += (double)X[(size_t)n * R + i] * (double)X[(size_t)n * R + j];
    }
    a = wave_sum_d(a);
    if (lane == 0) out[1 + p] = a;
  }
}

// One workgroup = one SLICE of `per` local samples (the statistics are additive over samples: the slices of a rank are reduced in a fixed
// order by vbgmm_stats_reduce_kernel exactly as the ranks are by the all-reduce): 79 workgroups at the 20 096 samples of the accurate fit.
__global__ __launch_bounds__(VB_THREADS) void vbgmm_shard_estep_kernel(const float* __restrict__ X, const int* __restrict__ labels,
                                                                       const double* __restrict__ state, VbCfg c, double* __restrict__ resp,
                                                                       double* __restrict__ stats, const int per, const size_t stats_stride) {
  const int K = c.K, R = c.R, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  VbState S(const_cast<double*>(state), K, R);
  if (fit_done(S.tail)) return;                                  // the fit is over: later (speculatively enqueued) iterations are no-ops
  const int n_first = blockIdx.x * per, N = min(per, c.N - n_first);
  X += (size_t)n_first * R;
  if (labels != nullptr) labels += n_first;
  resp += (size_t)n_first * K;
  stats += (size_t)blockIdx.x * stats_stride;
  __shared__ double s_ck[VB_MAXK], s_mu[VB_MAXK * VB_MAXR], s_pc[VB_MAXK * VB_MAXR * VB_MAXR], s_red[VB_WAVES], s_scal[1];
  double entropy = 0.0;
  if (c.init_from_labels) fit_onehot(labels, N, K, resp, tid, VB_THREADS);
  else entropy = vb_estep(X, N, S, c, s_mu, s_pc, s_ck, s_scal, s_red, resp, tid);
  __syncthreads();
  // local sufficient statistics (fixed order: lane-strided partial sums, then the shuffle tree)
  if (tid == 0) stats[0] = entropy;
  const FitStats<double> st(stats, K, R);
  for (int p = wave; p < K * (1 + R + R * R); p += VB_WAVES) {
    double a = 0.0;
    if (p < K) {
      for (int n = lane; n < N; n += 64) a += resp[(size_t)n * K + p];
    } else if (p < K + K * R) {
      const int k = (p - K) / R, r = (p - K) - k * R;
      for (int n = lane; n < N; n += 64) a += resp[(size_t)n * K + k] * (double)X[(size_t)n * R + r];
    } else {
      const int q = p - K - K * R, k = q / (R * R), ij = q - k * R * R, i = ij / R, j = ij - i * R;
      if (j < i) continue;                                        // (upper triangle; mirrored below)
      for (int n = lane; n < N; n += 64) a += resp[(size_t)n * K + k] * (double)X[(size_t)n * R + i] * (double)X[(size_t)n * R + j];
    }
    a = wave_sum_d(a);
    if (lane == 0) {
      if (p < K) st.nk[p] = a;
      else if (p < K + K * R) st.x[p - K] = a;
      else {
        const int q = p - K - K * R, k = q / (R * R), ij = q - k * R * R, i = ij / R, j = ij - i * R;
        st.xx[(size_t)k * R * R + i * R + j] = a;
        st.xx[(size_t)k * R * R + j * R + i] = a;
      }
    }
  }
}

__global__ __launch_bounds__(256) void vbgmm_stats_reduce_kernel(const double* __restrict__ partial, const double* __restrict__ tail, int G, int n,
                                                                 double* __restrict__ stats) {
  if (fit_done(tail)) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double a = 0.0;
  for (int g = 0; g < G; ++g) a += partial[(size_t)g * n + i];       // fixed order: slice 0, 1, ...
  stats[i] = a;
}

__global__ __launch_bounds__(256) void vbgmm_shard_mstep_kernel(const double* __restrict__ stats, const double* __restrict__ moments,
                                                                double* __restrict__ state, VbCfg c, int it, float* __restrict__ w_out,
                                                                float* __restrict__ m_out, float* __restrict__ c_out) {
  const int K = c.K, R = c.R, tid = threadIdx.x;
  VbState S(state, K, R);
  if (fit_done(S.tail)) return;
  __shared__ double s_nk[VB_MAXK], s_xk[VB_MAXK * VB_MAXR], s_sk[VB_MAXK * VB_MAXR * VB_MAXR], s_ck[VB_MAXK];
  __shared__ double s_prior_mean[VB_MAXR], s_prior_cov[VB_MAXR * VB_MAXR];
  __shared__ int s_flag, s_done;
  const double Ntot = moments[0];
  if (tid < R) s_prior_mean[tid] = moments[1 + tid] / Ntot;
  if (tid == 0) s_flag = 0;
  __syncthreads();
  if (tid < R * R) {
    const int i = tid / R, j = tid - i * R;
    s_prior_cov[tid] = (moments[1 + R + tid] - Ntot * s_prior_mean[i] * s_prior_mean[j]) / (Ntot - 1.0);
  }
  const FitStats<const double> st(stats, K, R);
  if (tid < K) s_nk[tid] = st.nk[tid] + kEps10;
  __syncthreads();
  for (int p = tid; p < K * R; p += 256) s_xk[p] = st.x[p] / s_nk[p / R];
  __syncthreads();
  // the raw second moments, centred here
  for (int p = tid; p < K * R * R; p += 256) {
    const int k = p / (R * R), ij = p - k * R * R, i = ij / R, j = ij - i * R;
    s_sk[p] = st.xx[p] / s_nk[k] - s_xk[k * R + i] * s_xk[k * R + j] + (i == j ? c.reg_covar : 0.0);
  }
  __syncthreads();
  if (tid < K) vb_update_component(tid, S, c, s_nk, s_xk, s_sk, s_prior_mean, s_prior_cov, &s_flag);
  __syncthreads();
  if (tid == 0) s_done = fit_end_iteration(S.tail, s_flag != 0, it, c.tol, c.max_iter, [&] { return vb_lower_bound(S, c, stats[0]); });
  __syncthreads();
  if (s_done != 1) return;
  vb_write_feed(S, c, s_ck, w_out, m_out, c_out, tid, 256);
}

// ================================================================================================ the WIDE fit: 8 < R <= 64
// The thread-per-sample E-step above keeps a sample in registers and every factor in LDS, which ends at R = 8.  Past it one variational iteration
// keeps the protocol of the sharded fit -- E-step + local statistics / all-reduce / M-step + convergence test, every kernel a no-op once `done` is
// set -- on the float64 MFMA passes of csrc/fit_mfma.h, which the EM fit (csrc/emgmm.hip) runs too:
//   vbwide_estep_kernel    fit_estep_slice under the policy VbwEstep: a workgroup owns 64 samples; per component the whitening quadratic form
//                          |(x - mean_k) P_k|^2, then w = ck[k] - q / 2 with the constants the finish kernel left in the state; logsumexp,
//                          responsibilities, the slice's sum r log r
//   fit_stats_kernel       n_k, sum r x~, sum r x~ x~^T about ONE shift c (the fp32-rounded global mean) over row splits; fit_reduce_kernel adds
//                          the splits (and the slices' sum r log r) in index order: stats = [ sum r log r | n_k | sum r x~ | sum r x~ x~^T ]
//   (all-reduce of stats, by the caller)
//   vbwide_mstep_kernel    one workgroup per component: weight parameters, mean precision, mean, the Wishart covariance from the shifted moments
//                          centred here (fit_centre_mean / fit_centred_cov), Cholesky factor and triangular inverse in LDS; a non-positive pivot
//                          is a status
//   vbwide_finish_kernel   one workgroup: the next E-step's constants (vb_estep_constant), then fit_end_iteration with vb_lower_bound, and at the
//                          end of the fit _set_parameters + the fp32 feed
// moments = [ sum x [R] | N | sum x~ x~^T [R,R] ]: the first R + 1 are all-reduced, then the second moments about the shift they define; from them
// mean_prior_ = X.mean(0) and covariance_prior_ = cov(X.T) = (sum x~ x~^T - N d d^T) / (N - 1), d = mean_prior_ - c.
constexpr int VBW_EXTRA = 2;             // ck[K] | cstat[K] between prec_chol and the tail

// grid (R, R): workgroup (j, i), i <= j, sums x~_i x~_j over the local samples and writes both mirrors
__global__ __launch_bounds__(256) void vbwide_moments2_kernel(const float* __restrict__ X, int N, int R, double* mom) {
  const int j = blockIdx.x, i = blockIdx.y, tid = threadIdx.x;
  if (j < i) return;
  __shared__ double s_red[4];
  const double ci = fit_shift(mom, R, i), cj = fit_shift(mom, R, j);
  double a = 0.0;
  for (int n = tid; n < N; n += 256) a += ((double)X[(size_t)n * R + i] - ci) * ((double)X[(size_t)n * R + j] - cj);
  a = block_sum_256(a, s_red, tid);
  if (tid == 0) {
    mom[R + 1 + i * R + j] = a;
    mom[R + 1 + j * R + i] = a;
  }
}

// _estimate_log_prob_resp as the policy of fit_estep_slice (what vb_estep does per row): the constant ck, the slice scalar is the sum of r log r.
struct VbwEstep {
  static constexpr int NCONST = 1;
  const double* ck;
  __device__ void load(double* s_c, int k) const { s_c[k] = ck[k]; }
  __device__ double log_term(const double* s_c, int k, double q) const { return s_c[k] - 0.5 * q; }
  __device__ double finish_row(double* wr, int K, double lse) const {
    double ent = 0.0;
    for (int k = 0; k < K; ++k) {
      const double lr = wr[k] - lse, r = exp(lr);
      wr[k] = r;
      ent += r * lr;
    }
    return ent;
  }
};

__global__ __launch_bounds__(256) void vbwide_estep_kernel(const float* __restrict__ X, const int* __restrict__ labels, const double* state, int N, int K,
                                                           int R, double* resp, double* __restrict__ ent_part) {
  VbState S(const_cast<double*>(state), K, R, VBW_EXTRA);
  if (fit_done(S.tail)) return;
  fit_estep_slice(VbwEstep{S.ck}, X, labels, S.pchol, S.means, N, K, R, resp, ent_part);
}

// _m_step for component blockIdx.x, 64 threads: what vb_update_component states per component, with the empirical covariance centred from the
// shifted moments (as emgmm_mstep_kernel) and the factorisation of fit_chol_inverse.
__global__ __launch_bounds__(64) void vbwide_mstep_kernel(const double* __restrict__ stats, const double* __restrict__ mom, double* state, VbCfg c) {
  const int K = c.K, R = c.R, k = blockIdx.x, tid = threadIdx.x;
  VbState S(state, K, R, VBW_EXTRA);
  if (fit_done(S.tail)) return;
  __shared__ double s_A[FIT_MAXR * FIT_LDC], s_s1[FIT_MAXR], s_dm[FIT_MAXR], s_dx[FIT_MAXR], s_dp[FIT_MAXR];
  const FitStats<const double> st(stats, K, R, k);
  const double* m2 = mom + R + 1;
  const double Ntot = mom[R];
  const double nk_raw = st.nk[k], nk = nk_raw + kEps10;            // nk = resp.sum(axis=0) + 10 * eps
  const double mp = c.mean_prec_prior + nk, dof = (double)R + nk;  // degrees_of_freedom_prior_ = n_features
  if (tid == 0) {
    if (c.prior_type == 0) {
      S.wa[k] = c.wc_prior + nk;                                   // dirichlet_distribution
      S.wb[k] = 0.0;
    } else {
      double tail = 0.0;                                           // sum_{j>k} nk_j
      for (int j = K - 1; j > k; --j) tail += st.nk[j] + kEps10;
      S.wa[k] = 1.0 + nk;
      S.wb[k] = c.wc_prior + tail;
    }
    S.mprec[k] = mp;
    S.dof[k] = dof;
  }
  if (tid < R) {
    const double xk = fit_centre_mean(mom, R, tid, st.x[tid], nk_raw, nk, s_s1, s_dm), cs = fit_shift(mom, R, tid);
    const double pm = mom[tid] / Ntot;                             // mean_prior_
    s_dp[tid] = pm - cs;
    s_dx[tid] = xk - pm;
    S.means[k * R + tid] = (c.mean_prec_prior * pm + nk * xk) / mp;
  }
  __syncthreads();
  double* C = S.cov + (size_t)k * R * R;
  for (int e = tid; e < R * R; e += 64) {
    const int i = e / R, j = e - i * R;
    if (j < i) continue;
    const double sk = fit_centred_cov(st.xx[e], s_s1, s_dm, i, j, nk_raw, nk, c.reg_covar);
    const double pc = (m2[e] - Ntot * s_dp[i] * s_dp[j]) / (Ntot - 1.0);                        // covariance_prior_
    const double v = (pc + nk * sk + nk * c.mean_prec_prior / mp * (s_dx[i] * s_dx[j])) / dof;   // _estimate_wishart_full
    s_A[i * FIT_LDC + j] = v;
    s_A[j * FIT_LDC + i] = v;
    C[i * R + j] = v;
    C[j * R + i] = v;
  }
  __syncthreads();
  const bool bad = fit_chol_inverse(s_A, R, S.pchol + (size_t)k * R * R, tid);
  if (tid == 0) S.cstat[k] = bad ? -1.0 : 0.0;
}

__global__ __launch_bounds__(256) void vbwide_finish_kernel(const double* __restrict__ stats, double* state, VbCfg c, int it, float* __restrict__ w_out,
                                                            float* __restrict__ m_out, float* __restrict__ c_out) {
  const int K = c.K, R = c.R, tid = threadIdx.x;
  VbState S(state, K, R, VBW_EXTRA);
  if (fit_done(S.tail)) return;
  __shared__ double s_ck[FIT_MAXK], s_stick[FIT_MAXK], s_lw[FIT_MAXK], s_dig;
  __shared__ int s_done;
  if (tid == 0) {
    double sw = 0.0;
    for (int k = 0; k < K; ++k) sw += S.wa[k];
    s_dig = c.prior_type == 0 ? vb_digamma(sw) : 0.0;
  }
  if (tid < K) {
    s_stick[tid] = c.prior_type == 0 ? 0.0 : vb_digamma(S.wb[tid]) - vb_digamma(S.wa[tid] + S.wb[tid]);
    s_lw[tid] = vb_log_wishart_term(tid, S, c);
  }
  __syncthreads();
  if (tid < K) S.ck[tid] = vb_estep_constant(tid, S.pchol + (size_t)tid * R * R, S, c, s_dig, s_stick);
  if (tid == 0) {
    bool bad = false;
    for (int k = 0; k < K; ++k) bad = bad || (S.cstat[k] < 0.0);
    s_done = fit_end_iteration(S.tail, bad, it, c.tol, c.max_iter, [&] { return vb_lower_bound(S, c, stats[0], s_lw); });
  }
  __syncthreads();
  if (s_done != 1) return;
  vb_write_feed(S, c, s_ck, w_out, m_out, c_out, tid, 256);
}

inline bool vb_bad_shape(int K, int R, int prior_type) { return K < 1 || K > VB_MAXK || R < 1 || R > VB_MAXR || (prior_type != 0 && prior_type != 1); }
inline VbCfg vb_cfg(int N, int K, int R, int prior_type, const int* labels, int max_iter = 0, double wc_prior = 0.0, double mean_prec_prior = 0.0,
                    double reg_covar = 0.0, double tol = 0.0) {
  return VbCfg{N, K, R, prior_type, max_iter, labels != nullptr ? 1 : 0, wc_prior, mean_prec_prior, reg_covar, tol};
}

}  // namespace

extern "C" {

size_t ladder_vbgmm_state_doubles(int K, int R) { return (size_t)K * (4 + R + 2 * R * R) + 4; }
size_t ladder_vbgmm_workspace_bytes(int N, int K) { return (size_t)N * K * sizeof(double); }

int ladder_vbgmm_fit(const float* X, int N, int K, int R, const int* labels, double* state, int prior_type, double wc_prior,
                     double mean_prec_prior, double reg_covar, double tol, int max_iter, float* weights, float* means,
                     float* covs, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (N < 2 || N < K || max_iter < 0 || vb_bad_shape(K, R, prior_type)) return LADDER_E_SHAPE;
  if (ws == nullptr || ws_bytes < ladder_vbgmm_workspace_bytes(N, K)) return LADDER_E_WORKSPACE;
  const VbCfg c = vb_cfg(N, K, R, prior_type, labels, max_iter, wc_prior, mean_prec_prior, reg_covar, tol);
  hipLaunchKernelGGL(vbgmm_fit_kernel, dim3(1), dim3(VB_THREADS), 0, stream, X, labels, state, c, (double*)ws, weights, means, covs);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

// ---- the sharded fit: see the kernels above.  All vectors are device doubles; the host all-reduces `moments` once and `stats` once per
// iteration (SUM over ranks) between the two launches.
size_t ladder_vbgmm_shard_stats_doubles(int K, int R) { return (size_t)1 + K + (size_t)K * R + (size_t)K * R * R; }
size_t ladder_vbgmm_shard_moments_doubles(int R) { return (size_t)1 + R + (size_t)R * R; }

int ladder_vbgmm_shard_moments(const float* X, int N, int R, double* moments, ladder_stream_t stream) {
  if (N < 1 || R < 1 || R > VB_MAXR) return LADDER_E_SHAPE;
  hipLaunchKernelGGL(vbgmm_moments_kernel, dim3(1), dim3(VB_THREADS), 0, stream, X, N, R, moments);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

// local samples per workgroup of the sharded E-step (a slice); its statistics loop is wave-per-statistic over the slice
static constexpr int VB_SLICE = 256;
static int vb_slices(int N) { return (N + VB_SLICE - 1) / VB_SLICE; }

size_t ladder_vbgmm_shard_workspace_bytes(int N, int K, int R) {
  if (N < 1 || K < 1 || R < 1) return 0;
  return ((size_t)N * K + (size_t)vb_slices(N) * ladder_vbgmm_shard_stats_doubles(K, R)) * sizeof(double);   // responsibilities + per-slice statistics
}

int ladder_vbgmm_shard_estep(const float* X, int N, int K, int R, const int* labels, const double* state, int prior_type, double* stats,
                             void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (N < 1 || vb_bad_shape(K, R, prior_type)) return LADDER_E_SHAPE;
  if (ws == nullptr || ws_bytes < ladder_vbgmm_shard_workspace_bytes(N, K, R)) return LADDER_E_WORKSPACE;
  const VbCfg c = vb_cfg(N, K, R, prior_type, labels);
  const int G = vb_slices(N), n = (int)ladder_vbgmm_shard_stats_doubles(K, R);
  double* resp = (double*)ws;
  double* partial = resp + (size_t)N * K;
  // one slice writes `stats` itself; several write per-slice partials, reduced in slice order
  hipLaunchKernelGGL(vbgmm_shard_estep_kernel, dim3(G), dim3(VB_THREADS), 0, stream, X, labels, state, c, resp, G == 1 ? stats : partial, VB_SLICE,
                     (size_t)(G == 1 ? 0 : n));
  if (G > 1)
    hipLaunchKernelGGL(vbgmm_stats_reduce_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const double*)partial,
                       fit_tail(state, ladder_vbgmm_state_doubles(K, R)), G, n, stats);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_vbgmm_shard_mstep(const double* stats, const double* moments, int K, int R, double* state, int prior_type, double wc_prior,
                             double mean_prec_prior, double reg_covar, double tol, int max_iter, int it, float* weights, float* means,
                             float* covs, ladder_stream_t stream) {
  if (max_iter < 0 || it < 0 || vb_bad_shape(K, R, prior_type)) return LADDER_E_SHAPE;
  const VbCfg c = vb_cfg(0, K, R, prior_type, nullptr, max_iter, wc_prior, mean_prec_prior, reg_covar, tol);
  hipLaunchKernelGGL(vbgmm_shard_mstep_kernel, dim3(1), dim3(256), 0, stream, stats, moments, state, c, it, weights, means, covs);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

// ---- the wide fit (8 < R <= 64; the kernels take 1 <= R <= 64): see vbwide_* above.  The caller all-reduces moments[0 .. R] after pass 0,
// moments[R + 1 ..] after pass 1, and `stats` once per iteration between the two launches.
static bool vbw_bad_shape(int K, int R, int prior_type) {
  return K < 1 || K > FIT_MAXK || R < 1 || R > FIT_MAXR || (prior_type != 0 && prior_type != 1);
}

size_t ladder_vbgmm_wide_state_doubles(int K, int R) { return (K < 1 || R < 1) ? 0 : (size_t)K * (4 + VBW_EXTRA + R + 2 * (size_t)R * R) + 4; }
size_t ladder_vbgmm_wide_stats_doubles(int K, int R) { return (K < 1 || R < 1) ? 0 : fit_stats_doubles(K, R); }
size_t ladder_vbgmm_wide_moments_doubles(int R) { return R < 1 ? 0 : (size_t)R + 1 + (size_t)R * R; }

size_t ladder_vbgmm_wide_workspace_bytes(int N, int K, int R) { return fit_sliced_workspace_bytes(N, K, R); }

int ladder_vbgmm_wide_moments(const float* X, int N, int R, double* moments, int pass, ladder_stream_t stream) {
  if (X == nullptr || moments == nullptr || N < 1 || R < 1 || R > FIT_MAXR || (pass != 0 && pass != 1)) return LADDER_E_SHAPE;
  if (fit_misaligned(moments)) return LADDER_E_ALIGN;
  if (pass == 0) hipLaunchKernelGGL(fit_colsum_kernel, dim3(R), dim3(256), 0, stream, X, N, R, moments);
  else hipLaunchKernelGGL(vbwide_moments2_kernel, dim3(R, R), dim3(256), 0, stream, X, N, R, moments);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_vbgmm_wide_estep(const float* X, int N, int K, int R, const int* labels, const double* state, int prior_type, const double* moments,
                            double* stats, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  return fit_sliced_estep(vbwide_estep_kernel, prior_type != 0 && prior_type != 1, X, N, K, R, labels, state,
                          ladder_vbgmm_wide_state_doubles(K, R), moments, stats, ws, ws_bytes, stream);
}

int ladder_vbgmm_wide_mstep(const double* stats, const double* moments, int K, int R, double* state, int prior_type, double wc_prior,
                            double mean_prec_prior, double reg_covar, double tol, int max_iter, int it, float* weights, float* means, float* covs,
                            ladder_stream_t stream) {
  if (stats == nullptr || moments == nullptr || state == nullptr || weights == nullptr || means == nullptr || covs == nullptr || max_iter < 0 ||
      it < 0 || vbw_bad_shape(K, R, prior_type))
    return LADDER_E_SHAPE;
  if (fit_misaligned(stats) || fit_misaligned(moments) || fit_misaligned(state)) return LADDER_E_ALIGN;
  const VbCfg c = vb_cfg(0, K, R, prior_type, nullptr, max_iter, wc_prior, mean_prec_prior, reg_covar, tol);
  hipLaunchKernelGGL(vbwide_mstep_kernel, dim3(K), dim3(64), 0, stream, stats, moments, state, c);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(vbwide_finish_kernel, dim3(1), dim3(256), 0, stream, stats, state, c, it, weights, means, covs);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
