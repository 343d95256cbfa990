// EM fit of the baseline "GMM" prior on the device for WIDE codes: the algorithm of csrc/emgmm.hip -- sklearn.mixture.GaussianMixture(
// covariance_type="full", init_params="kmeans") in float64 -- for 64 < R <= 256, R % 16 == 0 (cw_width_ok) and 1 <= K <= 64.  The reference's
// shipped CelebA config fits K = 50 components on code_size = 256.  Same state (csrc/em_state.h), same `stats`, same protocol; what changes is how
// the work is cut, because P_k = precisions_cholesky_[k] is 512 KB at R = 256 and no longer fits a workgroup's LDS:
//
//   emw_estep_kernel   grid (64-sample slice, component), 4 wavefronts x 16 rows.  A lane keeps its R / 4 A operands x - mu_k of
//                      v_mfma_f64_16x16x4_f64 in registers (at most 64 doubles); P_k passes through LDS one 16-column panel at a time -- column
//                      block jb has rows 0 .. 16 jb + 15 only (P_k is upper triangular: the all-zero blocks below the diagonal are never staged
//                      or multiplied), at most 32 KB, double-buffered so that panel jb + 1 is fetched while panel jb is multiplied.  |y|^2 is
//                      summed block by block, then over the 16 columns of a lane group; the log term goes to resp [N, K].
//   emw_rows_kernel    one wavefront per slice: logsumexp per row, the responsibilities in place of the log terms, the slice's sum of
//                      log_prob_norm (it = 0: the slice sum of the one-hot start is 0).
//   emw_stats_kernel   grid (component, row split of fit_split, 16-row band bi of the R x R moment).  Wavefront w owns the column blocks
//                      bi + w, bi + w + 4, ... (at most four accumulators); wavefront 0 also collects sum r x~ of its band through the unit
//                      column e_0, and band 0 the count n_k.  x~ = x - c with the one shift vector of fit_shift.
//   fit_reduce_kernel  (csrc/fit_mfma.h, unchanged) the partials in split order, the slice sums in slice order.
//   emw_mstep_kernel   one workgroup of CW_THREADS per component: weight, mean, the covariance centred from the shifted raw moments
//                      (fit_centre_mean / fit_centred_cov) written to the state, to the fp32 feed and into the component's float64 working matrix
//                      in the caller's workspace, factored there (chol_wide_factor_in_place: the panel Cholesky); the triangular inverse goes
//                      into the state a column per thread (emw_tri_inverse) and is transposed in place: precisions_cholesky_ = Linv^T dense upper
//                      triangular; the log-determinant with its terms in index order, the status.
//   emgmm_finish_kernel  (csrc/em_state.h) the end of the iteration.
// Every kernel returns at once when `done` is set; no atomics, every sum has one fixed order: a fit gives the same bits on every run, for every
// `check_every` and on every rank of a sharded fit.
#include "chol_wide.h"
#include "em_state.h"
#include "fit_mfma.h"

namespace {

constexpr int EMW_MAXSTEPS = CW_MAXR / 4;        // MFMA k-steps over the widest row
constexpr int EMW_MAXNB = CW_MAXR / CW_PANEL;    // 16-column blocks of the widest row

__host__ __device__ inline bool emw_shape_ok(int K, int R) { return K >= 1 && K <= FIT_MAXK && cw_width_ok(R); }

// ------------------------------------------------------------------------------------------------ E-step
// Column panel jb of the upper-triangular P [R,R]: rows 0 .. 16 jb + 15, columns 16 jb .. 16 jb + 15 -> s_P[row * 16 + col]; 256 threads.
__device__ __forceinline__ void emw_stage_panel(const double* __restrict__ P, int R, int jb, double* s_P, int tid) {
  const int n = (jb + 1) * CW_PANEL * CW_PANEL;
  for (int idx = tid; idx < n; idx += 256) s_P[idx] = P[(size_t)(idx >> 4) * R + CW_PANEL * jb + (idx & 15)];
}

__global__ __launch_bounds__(256) void emw_estep_kernel(const float* __restrict__ X, const int* __restrict__ labels, const double* state, int N, int K,
                                                        int R, double* resp) {
  EmState S(const_cast<double*>(state), K, R);
  if (fit_done(S.tail)) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
  const int k = blockIdx.y, n0 = blockIdx.x * FIT_SLICE, rows = min(FIT_SLICE, N - n0);
  if (labels != nullptr) {
    if (k == 0) fit_onehot(labels + n0, rows, K, resp + (size_t)n0 * K, tid, 256);
    return;
  }
  __shared__ double s_P[2][CW_MAXR * CW_PANEL];
  const int nb = R / CW_PANEL;
  const double* P = S.pchol + (size_t)k * R * R;
  const double* mu = S.means + (size_t)k * R;
  const int row = wave * 16 + m;
  const bool rv = row < rows;
  const float* xr = X + (size_t)(n0 + (rv ? row : 0)) * R;         // (row n0 exists: never dereferenced unless rv)
  double xa[EMW_MAXSTEPS];                                         // this lane's A operands: (x - mu)[4 s + kq], zero past R and past `rows`
#pragma unroll
  for (int s = 0; s < EMW_MAXSTEPS; ++s) {
    const int i = 4 * s + kq;
    xa[s] = (rv && i < R) ? (double)xr[i] - mu[i] : 0.0;
  }
  emw_stage_panel(P, R, 0, s_P[0], tid);
  __syncthreads();
  double q4[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int jb = 0; jb < EMW_MAXNB; ++jb) {
    if (jb < nb) {                                                 // (uniform over the workgroup: the barrier below is reached by all or none)
      if (jb + 1 < nb) emw_stage_panel(P, R, jb + 1, s_P[(jb + 1) & 1], tid);
      const double* sp = s_P[jb & 1];
      double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4 * (jb + 1); ++s)                       // rows past 16 jb + 15 of this column block are zero; R % 16 == 0
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[s], sp[(4 * s + kq) * CW_PANEL + m], acc, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) q4[r] += acc[r] * acc[r];
      __syncthreads();                                             // panel jb + 1 is in place, panel jb is no longer read
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) q4[r] += __shfl_xor(q4[r], o, 64);      // over the 16 columns of the lane group
  if (m == 0) {
    const double ld = S.logdet[k], lw = log(S.w[k]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rr = wave * 16 + kq + 4 * r;
      if (rr < rows) resp[(size_t)(n0 + rr) * K + k] = (-0.5 * (R * kLog2Pi + q4[r]) + ld) + lw;
    }
  }
}

// _estimate_log_prob_resp on the log terms of slice blockIdx.x, a thread per row (64 threads)
__global__ __launch_bounds__(64) void emw_rows_kernel(const int* __restrict__ labels, const double* __restrict__ tail, int N, int K, double* resp,
                                                      double* __restrict__ slice_part) {
  if (fit_done(tail)) return;
  const int tid = threadIdx.x, n0 = blockIdx.x * FIT_SLICE, rows = min(FIT_SLICE, N - n0);
  if (labels != nullptr) {
    if (tid == 0) slice_part[blockIdx.x] = 0.0;
    return;
  }
  double a = 0.0;
  if (tid < rows) {
    double* wr = resp + (size_t)(n0 + tid) * K;
    double mx = -INFINITY;
    for (int k = 0; k < K; ++k) mx = fmax(mx, wr[k]);
    double se = 0.0;
    for (int k = 0; k < K; ++k) se += exp(wr[k] - mx);
    a = log(se) + mx;                                              // log_prob_norm of the row
    for (int k = 0; k < K; ++k) wr[k] = exp(wr[k] - a);
  }
  a = wave_sum_d(a);
  if (tid == 0) slice_part[blockIdx.x] = a;
}

// ------------------------------------------------------------------------------------------------ statistics
// Grid (component, row split, band), 256 threads.  Band bi = rows 16 bi .. 16 bi + 15 of the R x R moment; wavefront w accumulates the column
// blocks bi + w + 4 q, q = 0 .. 3, that exist.  Operands come straight from global memory, as in fit_stats_kernel; the partials of split s go to
// part + s * fit_stats_doubles(K, R) in its layout, so fit_reduce_kernel adds them.
__global__ __launch_bounds__(256) void emw_stats_kernel(const float* __restrict__ X, const double* __restrict__ resp, const double* __restrict__ tail,
                                                        const double* __restrict__ mom, int N, int K, int R, int rows, double* __restrict__ part) {
  if (fit_done(tail)) return;
  const int k = blockIdx.x, bi = blockIdx.z, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
  const int nb = R / CW_PANEL;
  if (bi + wave >= nb) return;                                     // (whole wavefronts; no barrier in this pass)
  const int ia = bi * 16 + m;
  const double ca = fit_shift(mom, R, ia);
  int jb[4];
  bool vb[4];                                                      // (the same in every lane of the wavefront)
  double cb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int bj = bi + wave + 4 * q;
    vb[q] = bj < nb;
    jb[q] = vb[q] ? bj * 16 + m : 0;
    cb[q] = vb[q] ? fit_shift(mom, R, jb[q]) : 0.0;
  }
  const double e0 = (m == 0) ? 1.0 : 0.0;
  const int r0 = blockIdx.y * rows, r1 = min(N, r0 + rows);
  double4_t acc[4], acc1 = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  double nk = 0.0;
  for (int r = r0; r < r1; r += 4) {                               // (uniform trip count)
    const int row = r + kq;
    const bool ok = row < r1;
    const float* xr = X + (size_t)(ok ? row : r0) * R;
    const double rr = ok ? resp[(size_t)row * K + k] : 0.0;
    nk += rr;
    const double a = ok ? rr * ((double)xr[ia] - ca) : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (vb[q]) {
        const double b = ok ? (double)xr[jb[q]] - cb[q] : 0.0;
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
      }
    }
    if (wave == 0) acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, e0, acc1, 0, 0, 0);
  }
  const FitStats<double> p(part + (size_t)blockIdx.y * fit_stats_doubles(K, R), K, R, k);
  if (bi == 0 && wave == 0) {                                      // n_k: the rows r0 + kq + 4 t of lane group kq, then the four groups in order
    const double g0 = __shfl(nk, 0, 64), g1 = __shfl(nk, 16, 64), g2 = __shfl(nk, 32, 64), g3 = __shfl(nk, 48, 64);
    if (lane == 0) p.nk[k] = ((g0 + g1) + g2) + g3;
  }
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int i = bi * 16 + kq + 4 * rg;
    if (wave == 0 && m == 0) p.x[i] = acc1[rg];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (vb[q]) p.xx[(size_t)i * R + jb[q]] = acc[q][rg];
  }
}

// ------------------------------------------------------------------------------------------------ M-step
// X = L^-1 (lower triangular, row-major [R][R], zero-filled by the caller) of the factored W, thread c = column c, by forward substitution on the
// identity: X[i][c] = -(sum_{p = c}^{i-1} L[i][p] X[p][c]) / L[i][i].  A column is its thread's own, so no barrier separates the rows.  All lanes of
// a wavefront walk the same (i, p) from the wavefront's first column c0 on -- the terms with p < c multiply the zeros above the diagonal of X -- so
// that L[i][p] is ONE address per wavefront and X[p][c] a contiguous row segment.  (chol_wide_factor_in_place<true> keeps L^-1 transposed beside L
// and reads W[c][p] a thread per row, R doubles apart: measured 4.2 of the 4.9 ms of an M-step at R = 256 before this replaced it here.)
__device__ __forceinline__ void emw_tri_inverse(const double* __restrict__ W, int R, double* __restrict__ X) {
  const int c = threadIdx.x, c0 = c & ~63;
  if (c0 >= R) return;                                             // (whole wavefronts)
  const bool mine = c < R;
  const int cc = mine ? c : c0;                                    // lanes past R read along with column c0 and store nothing
  for (int i = c0; i < R; ++i) {
    const double* wr = W + (size_t)i * R;
    double v = 0.0;
#pragma unroll 8
    for (int p = c0; p < i; ++p) v -= wr[p] * X[(size_t)p * R + cc];
    if (mine && i >= c) X[(size_t)i * R + c] = (i == c) ? 1.0 / wr[i] : v / wr[i];
  }
}

// _compute_precision_cholesky for component k by one workgroup of CW_THREADS: W [R][R] (the component's slot of the workspace) holds the float64
// covariance on entry, published by a barrier.  Writes precisions_cholesky_[k] = Linv^T (dense, upper triangular), its log-determinant and the
// component status (-1: a non-positive or NaN pivot; precisions_cholesky_[k] is then left as it was).
__device__ void emw_prepare_component(double* W, int R, int k, EmState& S, CwShared& sh) {
  const int tid = threadIdx.x;
  const bool failed = chol_wide_factor_in_place<false>(R, W, sh);  // (the same in every thread)
  if (!failed) {
    double* Pk = S.pchol + (size_t)k * R * R;
    for (int e = tid; e < R * R; e += CW_THREADS) Pk[e] = 0.0;
    __syncthreads();
    emw_tri_inverse(W, R, Pk);                                     // Pk = L^-1, lower triangular ...
    __syncthreads();
    for (int e = tid; e < R * R; e += CW_THREADS) {                // ... transposed in place: one thread per pair below / above the diagonal
      const int i = e / R, c = e - i * R;
      if (c < i) {
        Pk[(size_t)c * R + i] = Pk[e];
        Pk[e] = 0.0;
      }
    }
    double* scratch = sh.panel;
    if (tid < R) scratch[tid] = log(1.0 / W[(size_t)tid * R + tid]);
    __syncthreads();
    if (tid == 0) {
      double ld = 0.0;
      for (int j = 0; j < R; ++j) ld += scratch[j];
      S.logdet[k] = ld;
    }
  }
  if (tid == 0) {
    if (failed) S.logdet[k] = 0.0;
    S.cstat[k] = failed ? -1.0 : 0.0;
  }
}

__global__ __launch_bounds__(CW_THREADS) void emw_mstep_kernel(const double* __restrict__ stats, const double* __restrict__ mom, double* state, int K,
                                                               int R, double reg_covar, int it, float* __restrict__ w_out, float* __restrict__ m_out,
                                                               float* __restrict__ c_out, double* wbase) {
  EmState S(state, K, R);
  if (fit_done(S.tail)) return;
  const int k = blockIdx.x, tid = threadIdx.x;
  __shared__ CwShared sh;
  __shared__ double s_s1[CW_MAXR], s_dm[CW_MAXR];
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
    S.means[(size_t)k * R + tid] = mean;
    m_out[(size_t)k * R + tid] = (float)mean;
  }
  __syncthreads();
  double* C = S.cov + (size_t)k * R * R;                           // [i][j] for i <= j, mirrored
  float* Cf = c_out + (size_t)k * R * R;
  double* W = wbase + (size_t)k * R * R;                           // K <= CW_SLOTS: a slot per component
  for (int e = tid; e < R * R; e += CW_THREADS) {
    const int i = e / R, j = e - i * R;
    if (j < i) continue;
    const double v = fit_centred_cov(st.xx[e], s_s1, s_dm, i, j, nk_raw, nk, reg_covar);
    C[i * R + j] = v;
    C[j * R + i] = v;
    W[i * R + j] = v;
    W[j * R + i] = v;
    Cf[i * R + j] = (float)v;
    Cf[j * R + i] = (float)v;
  }
  __syncthreads();
  emw_prepare_component(W, R, k, S, sh);
}

// precisions_cholesky_ / log-determinant / status of the covariances already IN the state (parameters set from outside)
__global__ __launch_bounds__(CW_THREADS) void emw_prepare_kernel(double* state, int K, int R, double* wbase) {
  EmState S(state, K, R);
  const int k = blockIdx.x, tid = threadIdx.x;
  __shared__ CwShared sh;
  const double* C = S.cov + (size_t)k * R * R;
  double* W = wbase + (size_t)k * R * R;
  for (int e = tid; e < R * R; e += CW_THREADS) W[e] = C[e];
  __syncthreads();
  emw_prepare_component(W, R, k, S, sh);
}

static_assert(FIT_MAXK <= CW_SLOTS, "the M-step gives every component its own working matrix");

}  // namespace

extern "C" {

size_t ladder_emgmm_wide_state_doubles(int K, int R) { return emw_shape_ok(K, R) ? em_state_doubles(K, R) : 0; }
size_t ladder_emgmm_wide_stats_doubles(int K, int R) { return emw_shape_ok(K, R) ? fit_stats_doubles(K, R) : 0; }
size_t ladder_emgmm_wide_shift_doubles(int R) { return cw_width_ok(R) ? (size_t)R + 1 : 0; }
size_t ladder_emgmm_wide_workspace_bytes(int N, int K, int R) { return emw_shape_ok(K, R) ? fit_sliced_workspace_bytes(N, K, R) : 0; }
size_t ladder_emgmm_wide_mstep_workspace_bytes(int K, int R) { return emw_shape_ok(K, R) ? cw_workspace_bytes(K, R) : 0; }

int ladder_emgmm_wide_shift(const float* X, int N, int R, double* moments, ladder_stream_t stream) {
  if (X == nullptr || moments == nullptr || N < 1 || !cw_width_ok(R)) return LADDER_E_SHAPE;
  if (fit_misaligned(moments)) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(fit_colsum_kernel, dim3(R), dim3(256), 0, stream, X, N, R, moments);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_emgmm_wide_estep(const float* X, int N, int K, int R, const int* labels, const double* state, const double* moments, double* stats,
                            void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (X == nullptr || state == nullptr || moments == nullptr || stats == nullptr || N < 1 || !emw_shape_ok(K, R)) return LADDER_E_SHAPE;
  if (fit_misaligned(state) || fit_misaligned(moments) || fit_misaligned(stats) || fit_misaligned(ws)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < fit_sliced_workspace_bytes(N, K, R)) return LADDER_E_WORKSPACE;
  const FitSplit sp = fit_split(N);
  const int G = fit_slices(N);
  const size_t n = fit_stats_doubles(K, R);
  const double* tail = fit_tail(state, em_state_doubles(K, R));
  double* resp = static_cast<double*>(ws);
  double* slice_part = resp + (size_t)N * K;
  double* part = slice_part + G;
  hipLaunchKernelGGL(emw_estep_kernel, dim3(G, K), dim3(256), 0, stream, X, labels, state, N, K, R, resp);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(emw_rows_kernel, dim3(G), dim3(64), 0, stream, labels, tail, N, K, resp, slice_part);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(emw_stats_kernel, dim3(K, sp.nsplit, R / CW_PANEL), dim3(256), 0, stream, X, (const double*)resp, tail, moments, N, K, R, sp.rows,
                     part);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(fit_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const double*)part, (const double*)slice_part, tail, K, R,
                     sp.nsplit, G, stats);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_emgmm_wide_mstep(const double* stats, const double* moments, int K, int R, double* state, void* ws, size_t ws_bytes, double reg_covar,
                            double tol, int max_iter, int it, float* weights, float* means, float* covs, ladder_stream_t stream) {
  if (stats == nullptr || moments == nullptr || state == nullptr || weights == nullptr || means == nullptr || covs == nullptr || !emw_shape_ok(K, R) ||
      max_iter < 0 || it < 0)
    return LADDER_E_SHAPE;
  if (fit_misaligned(stats) || fit_misaligned(moments) || fit_misaligned(state)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < cw_workspace_bytes(K, R)) return LADDER_E_WORKSPACE;
  hipLaunchKernelGGL(emw_mstep_kernel, dim3(K), dim3(CW_THREADS), 0, stream, stats, moments, state, K, R, reg_covar, it, weights, means, covs,
                     cw_workspace_base(ws));
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(emgmm_finish_kernel, dim3(1), dim3(64), 0, stream, stats, moments, state, K, R, tol, max_iter, it);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_emgmm_wide_prepare(double* state, int K, int R, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (state == nullptr || !emw_shape_ok(K, R)) return LADDER_E_SHAPE;
  if (fit_misaligned(state)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < cw_workspace_bytes(K, R)) return LADDER_E_WORKSPACE;
  hipLaunchKernelGGL(emw_prepare_kernel, dim3(K), dim3(CW_THREADS), 0, stream, state, K, R, cw_workspace_base(ws));
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(emgmm_finish_kernel, dim3(1), dim3(64), 0, stream, (const double*)nullptr, (const double*)nullptr, state, K, R, 0.0, 0, -1);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
