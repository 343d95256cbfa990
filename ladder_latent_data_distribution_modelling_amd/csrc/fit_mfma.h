// What the two wide mixture fits share on the float64 MFMA (csrc/emgmm.hip: EM on z; csrc/vbgmm.hip, the vbwide_* kernels: variational Bayes on t),
// 1 <= R <= 64, 1 <= K <= 64:
//   fit_estep_slice<Policy>                                the E-step of a 64-sample slice: one-hot start, the whitening quadratic form
//                                                          |(x - mu_k) P_k|^2 (fit_slice_rows / fit_stage_component / fit_whiten_sq), logsumexp per
//                                                          row; the policy states the fit's constants, log term and per-row finish
//   fit_colsum_kernel / fit_stats_kernel / fit_reduce_kernel   column sums; n_k, sum r x~, sum r x~ x~^T over row splits; the splits in index order
//   fit_sliced_estep / fit_sliced_workspace_bytes          the host side of an E-step: checks, workspace, the three launches
//   FitStats, fit_centre_mean / fit_centred_cov            the view into `stats`; the shifted raw moments centred in the M-step
//   fit_chol_inverse                                       Cholesky factor and its triangular inverse in LDS, by one wavefront
// Each of the two files instantiates its own copy of the three kernels; they find the `done` flag through the state's tail pointer (fit_util.h).
// No atomics: every sum has one fixed order.
//
// Operand lane maps of v_mfma_f64_16x16x4_f64: head of csrc/fid.hip (A [m = lane & 15][k = lane >> 4], B [k][n = lane & 15],
// C/D reg r: row (lane >> 4) + 4 r, col lane & 15).
#pragma once
#include "fit_util.h"

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int FIT_MAXR = 64, FIT_MAXK = 64;
constexpr int FIT_SLICE = 64;           // samples per E-step workgroup: 4 wavefronts x 16 MFMA rows
constexpr int FIT_LDP = 80;             // LDS row pitch of the staged P_k in doubles: the four k-rows of one B operand fall into different bank halves
constexpr int FIT_LDC = 65;             // LDS row pitch of the M-step's factorisation (odd: a thread per row or per column walks distinct banks)

// stats = [ one scalar | n_k [K] | sum r x~ [K,R] | sum r x~ x~^T [K,R,R] ]: one buffer, one all-reduce
__host__ __device__ inline size_t fit_stats_doubles(int K, int R) { return 1 + (size_t)K * (1 + R + (size_t)R * R); }
inline int fit_slices(int N) { return (N + FIT_SLICE - 1) / FIT_SLICE; }
// n_k [K] from component 0, sum r x~ [R] and sum r x~ x~^T [R,R] from component k on (T: double or const double)
template <class T>
struct FitStats {
  T *nk, *x, *xx;
  __device__ FitStats(T* stats, int K, int R, int k = 0) : nk(stats + 1), x(nk + K + (size_t)k * R), xx(nk + K + (size_t)K * R + (size_t)k * R * R) {}
};

// workspace of a sliced E-step: responsibilities [N, K] | per-slice scalars | per-split partial statistics
inline size_t fit_sliced_workspace_bytes(int N, int K, int R) {
  if (N < 1 || K < 1 || R < 1) return 0;
  return ((size_t)N * K + (size_t)fit_slices(N) + (size_t)fit_split(N).nsplit * fit_stats_doubles(K, R)) * sizeof(double);
}

// moments = [ sum_n x_n [R] | N | ... ], all-reduced by the caller: the shift is the GLOBAL mean rounded to fp32, the same on every rank
__device__ __forceinline__ double fit_shift(const double* mom, int R, int j) { return (double)(float)(mom[j] / mom[R]); }

// ------------------------------------------------------------------------------------------------ the whitening quadratic form of a slice
// This lane's A operands of slice row `row` (= wave * 16 + m): x[row][4 s + kq], zero past R and past the slice's `rows`.
__device__ __forceinline__ void fit_slice_rows(const float* __restrict__ X, int n0, int rows, int R, int row, int kq, double (&xa)[16]) {
  const bool rv = row < rows;
  const float* xr = X + (size_t)(n0 + (rv ? row : 0)) * R;         // (row n0 exists: never dereferenced unless rv)
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int i = 4 * s + kq;
    xa[s] = (rv && i < R) ? (double)xr[i] : 0.0;
  }
}

// Upper-triangular P [R,R] -> s_P [Rp][FIT_LDP] (zero padded to Rp = 16 ceil(R / 16)), mu [R] -> s_mu [FIT_MAXR]; 256 threads, barriers by the caller.
__device__ __forceinline__ void fit_stage_component(const double* P, const double* mu, int R, int Rp, double* s_P, double* s_mu, int tid) {
  for (int idx = tid; idx < Rp * Rp; idx += 256) {
    const int i = idx / Rp, j = idx - i * Rp;
    s_P[i * FIT_LDP + j] = (i < R && j < R) ? P[i * R + j] : 0.0;
  }
  if (tid < FIT_MAXR) s_mu[tid] = tid < R ? mu[tid] : 0.0;
}

// q4[r] = |y|^2 of slice row wave * 16 + kq + 4 r, y = (x - mu) P, the same bits in the 16 lanes of a lane group.  nb = ceil(R / 16),
// nsteps = ceil(R / 4).  Uniform: every lane reaches every MFMA.
__device__ __forceinline__ void fit_whiten_sq(const double (&xa)[16], const double* s_mu, const double* s_P, int nb, int nsteps, int m, int kq,
                                              double (&q4)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) q4[r] = 0.0;
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
    if (jb < nb) {
      double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int s = 0; s < 4 * (jb + 1); ++s) {                     // P is upper triangular: rows past 16 jb + 15 of this column block are zero
        if (s < nsteps) {
          const int i = 4 * s + kq;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[s] - s_mu[i], s_P[i * FIT_LDP + 16 * jb + m], acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) q4[r] += acc[r] * acc[r];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) q4[r] += __shfl_xor(q4[r], o, 64);      // over the 16 columns of the lane group: the same bits in every lane
}

// The E-step of slice blockIdx.x (FIT_SLICE samples, 256 threads).  labels != nullptr (iteration 0): the one-hot responsibilities, slice scalar 0.
// Else per component k: P_k = pchol[k] (upper triangular) and means[k] staged in LDS, resp[n][k] = pol.log_term(s_c, k, |(x_n - mu_k) P_k|^2);
// after the last k each row's logsumexp `lse`, then pol.finish_row(row, K, lse) turns the log terms into responsibilities and returns the row's
// share of the slice scalar, summed over the rows by wavefront 0 into slice_part[blockIdx.x].  Policy::NCONST constants per component live in LDS
// (s_c, FIT_MAXK apart), loaded by pol.load(s_c, k).
template <class Policy>
__device__ __forceinline__ void fit_estep_slice(const Policy& pol, const float* __restrict__ X, const int* __restrict__ labels, const double* pchol,
                                                const double* means, int N, int K, int R, double* resp, double* __restrict__ slice_part) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * FIT_SLICE, rows = min(FIT_SLICE, N - n0);
  if (labels != nullptr) {
    fit_onehot(labels + n0, rows, K, resp + (size_t)n0 * K, tid, 256);
    if (tid == 0) slice_part[blockIdx.x] = 0.0;
    return;
  }
  __shared__ double s_P[FIT_MAXR * FIT_LDP], s_mu[FIT_MAXR], s_c[Policy::NCONST * FIT_MAXK];
  const int nb = (R + 15) / 16, Rp = nb * 16, nsteps = (R + 3) / 4;
  double xa[16];                                                   // this lane's A operands: x[row][4 s + kq], zero past R
  fit_slice_rows(X, n0, rows, R, wave * 16 + m, kq, xa);
  if (tid < K) pol.load(s_c, tid);
  for (int k = 0; k < K; ++k) {
    __syncthreads();                                               // (the previous component's operands are no longer read)
    fit_stage_component(pchol + (size_t)k * R * R, means + k * R, R, Rp, s_P, s_mu, tid);
    __syncthreads();
    double q4[4];
    fit_whiten_sq(xa, s_mu, s_P, nb, nsteps, m, kq, q4);
    if (m == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rr = wave * 16 + kq + 4 * r;
        if (rr < rows) resp[(size_t)(n0 + rr) * K + k] = pol.log_term(s_c, k, q4[r]);
      }
    }
  }
  __syncthreads();
  double a = 0.0;
  if (tid < rows) {
    double* wr = resp + (size_t)(n0 + tid) * K;
    double mx = -INFINITY;
    for (int k = 0; k < K; ++k) mx = fmax(mx, wr[k]);
    double se = 0.0;
    for (int k = 0; k < K; ++k) se += exp(wr[k] - mx);
    a = pol.finish_row(wr, K, log(se) + mx);
  }
  if (wave == 0) {
    a = wave_sum_d(a);
    if (lane == 0) slice_part[blockIdx.x] = a;
  }
}

// ------------------------------------------------------------------------------------------------ statistics
// The three kernels both fits launch; each translation unit instantiates its own copy.
namespace {

// mom = [ sum_n x_n [R] | N ]: one workgroup per column (column_sum_256)
__global__ __launch_bounds__(256) void fit_colsum_kernel(const float* __restrict__ X, int N, int R, double* __restrict__ mom) {
  const int j = blockIdx.x, tid = threadIdx.x;
  __shared__ double s_red[4];
  const double a = column_sum_256(X, N, R, j, s_red, tid);
  if (tid == 0) {
    mom[j] = a;
    if (j == 0) mom[R] = (double)N;
  }
}

// Grid (component, row split), 256 threads.  Wavefront w owns rows 16 w .. 16 w + 15 of the R x R moment: the column blocks q >= w as MFMA
// accumulators, plus one block whose B operand is the unit column e_0, which collects sum r x~ in its column 0.  Operands come straight from global
// memory; x~ = x - c with ONE shift vector c for all components (fit_shift).  Partials of split s go to part + s * fit_stats_doubles(K, R).
__global__ __launch_bounds__(256) void fit_stats_kernel(const float* __restrict__ X, const double* __restrict__ resp, const double* __restrict__ tail,
                                                        const double* __restrict__ mom, int N, int K, int R, int rows, double* __restrict__ part) {
  if (fit_done(tail)) return;
  const int k = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
  const int nb = (R + 15) / 16;
  if (wave >= nb) return;                                          // (whole wavefronts; no barrier in this pass)
  const int ia = wave * 16 + m;
  const bool va = ia < R;
  const double ca = va ? fit_shift(mom, R, ia) : 0.0;
  int jb[4];
  bool vb[4];
  double cb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    jb[q] = 16 * q + m;
    vb[q] = jb[q] < R;
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
    const double a = (ok && va) ? rr * ((double)xr[ia] - ca) : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q >= wave && q < nb) {
        const double b = (ok && vb[q]) ? (double)xr[jb[q]] - cb[q] : 0.0;
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
      }
    }
    acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, e0, acc1, 0, 0, 0);
  }
  const FitStats<double> p(part + (size_t)blockIdx.y * fit_stats_doubles(K, R), K, R, k);
  if (wave == 0) {                                                 // n_k: the rows r0 + kq + 4 t of lane group kq, then the four groups in order
    const double g0 = __shfl(nk, 0, 64), g1 = __shfl(nk, 16, 64), g2 = __shfl(nk, 32, 64), g3 = __shfl(nk, 48, 64);
    if (lane == 0) p.nk[k] = ((g0 + g1) + g2) + g3;
  }
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int i = wave * 16 + kq + 4 * rg;
    if (i >= R) continue;
    if (m == 0) p.x[i] = acc1[rg];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q >= wave && q < nb && vb[q]) p.xx[(size_t)i * R + jb[q]] = acc[q][rg];
  }
}

// stats[e] = sum over the splits in index order, a thread per element (grid ceil(fit_stats_doubles / 256) x 256 threads); of the second moments
// only [i][j], i <= j, was computed: the lower triangle reads its mirror, so the moment is exactly symmetric.  Element 0 = the slices' scalar
// partials in slice order.
__global__ __launch_bounds__(256) void fit_reduce_kernel(const double* __restrict__ part, const double* __restrict__ slice_part,
                                                         const double* __restrict__ tail, int K, int R, int nsplit, int nslices,
                                                         double* __restrict__ stats) {
  if (fit_done(tail)) return;
  const size_t n = fit_stats_doubles(K, R), e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  double a = 0.0;
  if (e == 0) {
    for (int g = 0; g < nslices; ++g) a += slice_part[g];
  } else {
    size_t src = e;
    const size_t xx0 = 1 + (size_t)K + (size_t)K * R;
    if (e >= xx0) {
      const size_t q = e - xx0, kk = q / ((size_t)R * R), ij = q - kk * R * R, i = ij / R, j = ij - i * R;
      if (j < i) src = xx0 + kk * R * R + j * R + i;
    }
    for (int s = 0; s < nsplit; ++s) a += part[(size_t)s * n + src];
  }
  stats[e] = a;
}

}  // namespace

// The host side of a sliced E-step: `estep` (signature of fit_estep_slice's wrappers) over the slices, then the statistics and their reduction.
// state_doubles: the length of `state`, whose tail holds `done`; bad_shape: what the caller refuses beyond the checks below.
template <class EstepKernel>
inline int fit_sliced_estep(EstepKernel estep, bool bad_shape, const float* X, int N, int K, int R, const int* labels, const double* state,
                            size_t state_doubles, const double* moments, double* stats, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (bad_shape || X == nullptr || state == nullptr || moments == nullptr || stats == nullptr || N < 1 || K < 1 || K > FIT_MAXK || R < 1 || R > FIT_MAXR)
    return LADDER_E_SHAPE;
  if (fit_misaligned(state) || fit_misaligned(moments) || fit_misaligned(stats) || fit_misaligned(ws)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < fit_sliced_workspace_bytes(N, K, R)) return LADDER_E_WORKSPACE;
  const FitSplit sp = fit_split(N);
  const int G = fit_slices(N);
  const size_t n = fit_stats_doubles(K, R);
  const double* tail = fit_tail(state, state_doubles);
  double* resp = static_cast<double*>(ws);
  double* slice_part = resp + (size_t)N * K;
  double* part = slice_part + G;
  hipLaunchKernelGGL(estep, dim3(G), dim3(256), 0, stream, X, labels, state, N, K, R, resp, slice_part);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(fit_stats_kernel, dim3(K, sp.nsplit), dim3(256), 0, stream, X, (const double*)resp, tail, moments, N, K, R, sp.rows, part);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(fit_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const double*)part, (const double*)slice_part, tail, K, R,
                     sp.nsplit, G, stats);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

// ------------------------------------------------------------------------------------------------ the M-step's centring
// Component k's moments about the shift c (FitStats) -> sum r x / nk, with s1 and d = mean - c left in LDS for fit_centred_cov.  Thread j < R.
__device__ __forceinline__ double fit_centre_mean(const double* mom, int R, int j, double s1, double nk_raw, double nk, double* s_s1, double* s_dm) {
  const double c = fit_shift(mom, R, j);
  const double mean = (s1 + c * nk_raw) / nk;
  s_s1[j] = s1;
  s_dm[j] = mean - c;
  return mean;
}

// sum r (x - mean)(x - mean)^T / nk + reg_covar at [i][j] = (S2 - s1 d^T - d s1^T + n_k d d^T) / nk from xx = S2[i][j]; after a barrier.
__device__ __forceinline__ double fit_centred_cov(double xx, const double* s_s1, const double* s_dm, int i, int j, double nk_raw, double nk,
                                                  double reg_covar) {
  const double v = xx - (s_s1[i] * s_dm[j] + s_dm[i] * s_s1[j]) + nk_raw * s_dm[i] * s_dm[j];
  return v / nk + (i == j ? reg_covar : 0.0);
}

// ------------------------------------------------------------------------------------------------ factorisation
// _compute_precision_cholesky for one component, by ONE wavefront (64 threads): A [R][FIT_LDC] in LDS holds the covariance on entry.  Left-looking
// Cholesky, thread i = row i; then the triangular inverse, thread c = column c of L^-1, kept in the strict upper triangle of A (A[c][i] = L^-1[i][c])
// beside L, whose diagonal stays in A[j][j].  Writes Pk = precisions_cholesky_ [R,R] (upper triangular) and returns, in every thread, whether a
// pivot was non-positive (sklearn: LinAlgError -> ValueError("... ill-defined empirical covariance ...")); such a pivot is replaced by 1.
__device__ __forceinline__ bool fit_chol_inverse(double* A, int R, double* __restrict__ Pk, int tid) {
  __shared__ double s_d;
  __shared__ int s_bad;
  if (tid == 0) s_bad = 0;
  for (int j = 0; j < R; ++j) {
    double v = 0.0;
    if (tid >= j && tid < R) {
      v = A[tid * FIT_LDC + j];
      for (int p = 0; p < j; ++p) v -= A[tid * FIT_LDC + p] * A[j * FIT_LDC + p];
      if (tid == j) s_d = v;
    }
    __syncthreads();
    double d = s_d;
    if (!(d > 0.0)) {
      if (tid == j) s_bad = 1;
      d = 1.0;
    }
    const double ljj = sqrt(d);
    if (tid == j) A[j * FIT_LDC + j] = ljj;
    else if (tid > j && tid < R) A[tid * FIT_LDC + j] = v / ljj;
    __syncthreads();
  }
  if (tid < R) {
    const int c = tid;
    const double xc = 1.0 / A[c * FIT_LDC + c];
    for (int i = c + 1; i < R; ++i) {
      double v = -A[i * FIT_LDC + c] * xc;
      for (int p = c + 1; p < i; ++p) v -= A[i * FIT_LDC + p] * A[c * FIT_LDC + p];
      A[c * FIT_LDC + i] = v / A[i * FIT_LDC + i];
    }
    for (int i = 0; i < R; ++i) Pk[c * R + i] = (i < c) ? 0.0 : (i == c ? xc : A[c * FIT_LDC + i]);
  }
  __syncthreads();
  return s_bad != 0;
}
