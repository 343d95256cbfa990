// What the two EM fits of the "GMM" prior share (csrc/emgmm.hip: 1 <= R <= 64; csrc/emgmm_wide.hip: 80 <= R <= 256): the state layout and the
// end of an iteration.  Each translation unit instantiates its own copy of the finish kernel, as with the kernels of fit_mfma.h.
//
// state (doubles): weights [K] | means [K,R] | covariances [K,R,R] | precisions_cholesky [K,R,R] | log_det [K] | component status [K] |
//                  the tail of csrc/fit_util.h: lower_bound_, n_iter_, converged_, done
#pragma once
#include "fit_util.h"

namespace {

struct EmState {
  double *w, *means, *cov, *pchol, *logdet, *cstat, *tail;
  __host__ __device__ EmState(double* s, int K, int R) {
    w = s;
    means = w + K;
    cov = means + (size_t)K * R;
    pchol = cov + (size_t)K * R * R;
    logdet = pchol + (size_t)K * R * R;
    cstat = logdet + K;
    tail = cstat + K;
  }
};

__host__ __device__ inline size_t em_state_doubles(int K, int R) { return (size_t)K * (3 + R + 2 * (size_t)R * R) + 4; }

// The end of iteration `it`, one thread: component status, lower bound of this iteration's E-step, convergence test, n_iter_.
// it < 0: after a prepare kernel -- only the status is folded into the tail.
__global__ void emgmm_finish_kernel(const double* __restrict__ stats, const double* __restrict__ mom, double* state, int K, int R, double tol, int max_iter,
                                    int it) {
  EmState S(state, K, R);
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (it >= 0 && fit_done(S.tail)) return;
  bool bad = false;
  for (int k = 0; k < K; ++k) bad = bad || (S.cstat[k] < 0.0);
  fit_end_iteration(S.tail, bad, it, tol, max_iter, [&] { return stats[0] / mom[R]; });      // np.mean(log_prob_norm) over ALL samples
}

}  // namespace
