// The float64 factorisation of a WIDE covariance (64 < R <= 256, R % 16 == 0), shared by the prepare paths of the wide mixture
// (csrc/mixture_wide.hip) and of the wide sampler (csrc/sample.hip), which factor the fp32 feed copy (chol_wide_factor), and by the M-step of the
// wide EM fit (csrc/emgmm_wide.hip), which factors its float64 covariance where it stands (chol_wide_factor_in_place).
// One workgroup of CW_THREADS = 256 threads per component, thread i = row i.
//
// The working matrix W [R][R] (float64, row-major) lives in a caller-provided slot of global memory -- a 256 x 256 float64 matrix is 512 KB,
// a workgroup has 160 KB of LDS -- and only a 16-column panel of it sits in LDS at a time:
//   for each panel j0 = 0, 16, ...:   left-looking update of W[j0.., j0..j0+15] by the columns before j0 (the 16 pivot rows staged in LDS, 64
//                                     columns at a time), the panel factored in LDS column by column, then written back
// On return the lower triangle of W holds L (cov = L L^T).  With INVERSE the strict upper triangle holds L^-1 transposed, W[c][i] = Linv[i][c] for
// i > c, by forward substitution on the identity (thread c = column c); Linv[c][c] = 1 / W[c][c] stays implicit (cw_linv reads either).
// A non-positive or NaN pivot ends the factorisation: the function returns true in EVERY thread and W is left half done -- a status for the
// caller to report, never a trap or a silent NaN.  Plain __syncthreads() only; a workgroup reads nothing another workgroup writes.
#pragma once
#include "common.h"

constexpr int CW_THREADS = 256;        // = the largest R
constexpr int CW_MINR = 80, CW_MAXR = 256, CW_PANEL = 16, CW_CHUNK = 64;
constexpr int CW_PITCH = CW_PANEL + 1; // LDS row pitch of the panel in doubles (odd: a thread per row walks distinct banks)
constexpr int CW_SLOTS = 128;          // workgroups of a prepare launch = working matrices in the workspace; component k uses slot k % CW_SLOTS

__host__ __device__ inline bool cw_width_ok(int R) { return R >= CW_MINR && R <= CW_MAXR && (R % CW_PANEL) == 0; }
inline int cw_slots(int K) { return K < CW_SLOTS ? K : CW_SLOTS; }
inline size_t cw_workspace_bytes(int K, int R) {
  if (K < 1 || !cw_width_ok(R)) return 0;
  return (size_t)cw_slots(K) * R * R * sizeof(double) + 256;
}
inline double* cw_workspace_base(void* ws) { return reinterpret_cast<double*>(ladder_align256(ws)); }

// LDS of one factorisation (static, 43 KB)
struct CwShared {
  double panel[CW_MAXR * CW_PITCH];    // rows j0 .. R-1 of the current panel
  double rows[CW_CHUNK * CW_PANEL];    // [q][c] = W[j0 + c][q0 + q]: the 16 pivot rows over a 64-column chunk
};

// Linv[i][c] of a factored W (INVERSE), i >= c
__device__ __forceinline__ double cw_linv(const double* W, int R, int i, int c) { return i == c ? 1.0 / W[(size_t)c * R + c] : W[(size_t)c * R + i]; }

// The factorisation of a W already filled in place (the lower triangle and the diagonal blocks are read), after the barrier that publishes it.
template <bool INVERSE>
__device__ __forceinline__ bool chol_wide_factor_in_place(int R, double* W, CwShared& sh) {
  const int tid = threadIdx.x, i = tid;
  bool failed = false;
  for (int j0 = 0; j0 < R && !failed; j0 += CW_PANEL) {
    const bool mine = i >= j0 && i < R;
    double acc[CW_PANEL];
#pragma unroll
    for (int c = 0; c < CW_PANEL; ++c) acc[c] = mine ? W[(size_t)i * R + j0 + c] : 0.0;
    for (int q0 = 0; q0 < j0; q0 += CW_CHUNK) {
      const int nq = min(CW_CHUNK, j0 - q0);
      __syncthreads();                                   // (the previous chunk is no longer read)
      for (int e = tid; e < nq * CW_PANEL; e += CW_THREADS) {
        const int c = e / nq, q = e - c * nq;
        sh.rows[q * CW_PANEL + c] = W[(size_t)(j0 + c) * R + q0 + q];
      }
      __syncthreads();
      if (mine) {
        const double* wi = W + (size_t)i * R + q0;
        for (int q = 0; q < nq; ++q) {
          const double a = wi[q];
#pragma unroll
          for (int c = 0; c < CW_PANEL; ++c) acc[c] -= a * sh.rows[q * CW_PANEL + c];
        }
      }
    }
    if (mine) {
#pragma unroll
      for (int c = 0; c < CW_PANEL; ++c) sh.panel[i * CW_PITCH + c] = acc[c];
    }
    for (int c = 0; c < CW_PANEL; ++c) {
      const int j = j0 + c;
      __syncthreads();                                   // (row j's update of the previous column is in place)
      const double d = sh.panel[j * CW_PITCH + c];       // the same value in every thread: the exit below is uniform
      if (!(d > 0.0)) {
        failed = true;
        break;
      }
      const double piv = sqrt(d);
      const bool below = i > j && i < R;
      double l = 0.0;
      if (below) {
        l = sh.panel[i * CW_PITCH + c] / piv;
        sh.panel[i * CW_PITCH + c] = l;
      }
      __syncthreads();
      if (below)
        for (int c2 = c + 1; c2 < CW_PANEL; ++c2) sh.panel[i * CW_PITCH + c2] -= l * sh.panel[(j0 + c2) * CW_PITCH + c];
    }
    __syncthreads();
    if (!failed && mine) {
      for (int c = 0; c < CW_PANEL; ++c) {
        const int j = j0 + c;
        if (i > j) W[(size_t)i * R + j] = sh.panel[i * CW_PITCH + c];
        else if (i == j) W[(size_t)i * R + j] = sqrt(sh.panel[i * CW_PITCH + c]);
      }
    }
    __syncthreads();                                     // W's panel is visible to the workgroup; the LDS panel is free
  }
  if (failed) return true;
  if (INVERSE) {
    if (i < R) {
      const int c = i;
      double* wc = W + (size_t)c * R;                    // row c: L[c][0..c], then Linv[c+1..][c]
      const double xc = 1.0 / wc[c];
      for (int r = c + 1; r < R; ++r) {
        const double* wr = W + (size_t)r * R;
        double v = -wr[c] * xc;
        for (int p = c + 1; p < r; ++p) v -= wr[p] * wc[p];
        wc[r] = v / wr[r];
      }
    }
    __syncthreads();
  }
  return false;
}

// W = the float64 copy of an fp32 covariance [R,R], then the factorisation above.
template <bool INVERSE>
__device__ __forceinline__ bool chol_wide_factor(const float* __restrict__ cov, int R, double* W, CwShared& sh) {
  for (int e = threadIdx.x; e < R * R; e += CW_THREADS) W[e] = (double)cov[e];
  __syncthreads();
  return chol_wide_factor_in_place<INVERSE>(R, W, sh);
}

// sum_j log L[j][j] of a factored W, the terms added in index order; the same value in every thread.  `scratch`: CW_MAXR doubles of LDS.
__device__ __forceinline__ double cw_log_diag_sum(const double* W, int R, double* scratch) {
  __shared__ double s_sum;
  if ((int)threadIdx.x < R) scratch[threadIdx.x] = log(W[(size_t)threadIdx.x * R + threadIdx.x]);
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0;
    for (int j = 0; j < R; ++j) a += scratch[j];
    s_sum = a;
  }
  __syncthreads();
  return s_sum;
}
