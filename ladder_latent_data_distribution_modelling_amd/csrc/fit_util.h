// What the three mixture-fit files (csrc/vbgmm.hip, csrc/emgmm.hip, csrc/kmeans.hip) share on the host side and in reductions, and the protocol of
// a fit iteration that the EM fit and both sharded variational fits follow: the `done` test, the one-hot start, the end of an iteration.
#pragma once
#include "common.h"
#include "gmm_packed.h"            // for kLog2Pi alone: the fit files leave its packed fp32 macros unused

constexpr double kEps10 = 10.0 * 2.220446049250313e-16;           // 10 * np.finfo(float64).eps: sklearn's nk = resp.sum(axis=0) + 10 eps

// Every fit state ends with these four doubles (codes/mixture_fit.py reads them): lower_bound_, n_iter_, converged_ (-1: a non-positive
// Cholesky pivot, sklearn raises ValueError there) and the `done` flag that turns the kernels of later iterations into no-ops.
// (kmeans.hip keeps inertia_ and its own status code in the first and third place.)
enum { FIT_LB = 0, FIT_NITER = 1, FIT_CONVERGED = 2, FIT_DONE = 3 };
constexpr int FIT_TAIL = 4;

// The tail of a state of `n` doubles, and THE `done` test: the fit is over, iterations enqueued past the end are no-ops.
inline const double* fit_tail(const double* state, size_t n) { return state + n - FIT_TAIL; }
__device__ __forceinline__ bool fit_done(const double* tail) { return tail[FIT_DONE] != 0.0; }

// _initialize_parameters: one-hot responsibilities of N rows from the k-means labels
__device__ __forceinline__ void fit_onehot(const int* __restrict__ labels, int N, int K, double* __restrict__ resp, int tid, int nthreads) {
  for (size_t i = tid; i < (size_t)N * K; i += nthreads) resp[i] = (labels[i / K] == (int)(i % K)) ? 1.0 : 0.0;
}

// The end of iteration `it`, by one thread.  bad: a non-positive Cholesky pivot (ill-defined empirical covariance, sklearn raises) -> status -1.
// it < 0: only that status is folded into the tail; it == 0 (_initialize): no lower bound yet; else lower_bound() -- called in this branch
// alone -- against the previous one and `tol`, n_iter_, converged_.  -> 2: bad pivot, 1: the fit ended here (the caller writes the feed), 0: it goes on.
template <class LowerBound>
__device__ __forceinline__ int fit_end_iteration(double* tail, bool bad, int it, double tol, int max_iter, LowerBound lower_bound) {
  if (bad) {
    tail[FIT_CONVERGED] = -1.0;
    tail[FIT_DONE] = 1.0;
    return 2;
  }
  if (it < 0) return 0;
  bool over = it >= max_iter;
  if (it == 0) {
    tail[FIT_LB] = -INFINITY;
    tail[FIT_NITER] = 0.0;
  } else {
    const double lb = lower_bound();
    const bool conv = fabs(lb - tail[FIT_LB]) < tol;
    tail[FIT_LB] = lb;
    tail[FIT_NITER] = (double)it;
    if (conv) tail[FIT_CONVERGED] = 1.0;
    over = over || conv;
  }
  if (over) tail[FIT_DONE] = 1.0;
  return over ? 1 : 0;
}

// Row splits of the MFMA statistics kernels: at most 32 splits of at least 128 rows, rows per split a multiple of 4 (one MFMA k-step).
struct FitSplit {
  int rows, nsplit;
};
inline FitSplit fit_split(int N) {
  FitSplit p;
  int rows = (N + 31) / 32;
  rows = rows < 128 ? 128 : rows;
  p.rows = (rows + 3) / 4 * 4;
  p.nsplit = (N + p.rows - 1) / p.rows;
  return p;
}

inline bool fit_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

// Sum over the 256 threads: the shuffle tree, then the four wavefronts in order.  EVERY thread must call it (two barriers); s_w: 4 doubles
// of LDS; the result is valid in thread 0.
__device__ __forceinline__ double block_sum_256(double a, double* s_w, int tid) {
  a = wave_sum_d(a);
  if ((tid & 63) == 0) s_w[tid >> 6] = a;
  __syncthreads();
  const double r = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
  __syncthreads();
  return r;
}

// Sum of column j of X [N, R] by one workgroup of 256 threads: thread-strided partial sums, then block_sum_256.
__device__ __forceinline__ double column_sum_256(const float* __restrict__ X, int N, int R, int j, double* s_w, int tid) {
  double a = 0.0;
  for (int n = tid; n < N; n += 256) a += (double)X[(size_t)n * R + j];
  return block_sum_256(a, s_w, tid);
}
