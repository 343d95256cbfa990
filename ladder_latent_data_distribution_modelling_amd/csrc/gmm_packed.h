// The packed full-covariance mixture component of the narrow-latent (R <= 8) kernels and its per-component arithmetic: shared by the
// mixture log-prob kernels (csrc/mixture.hip) and the shortest-likely-path kernel (csrc/slp.hip).
//
//   packed[k] = { c_k = log w_k - log sum w - sum_i log L_ii - R/2 log 2pi, mean_k[R], Linv_k (lower tri, row-major) }
//
// with L_k the Cholesky factor of the covariance, so that  log (w_k N(t; m_k, Sigma_k)) = c_k - 0.5 |Linv_k (t - m_k)|^2.
#pragma once
#include "common.h"

constexpr double kLog2Pi = 1.8378770664093453;

template <int R>
struct GmmPacked {
  static constexpr int MEAN = 1, TRI = 1 + R, NT = R * (R + 1) / 2, STRIDE = 1 + R + NT;   // offsets of mean / Linv, floats of Linv / of a component
};

// The helpers below are macros, not functions, for one reason: these kernels promise results that are stable bit for bit, and the
// compiler contracts (fma) and pairs (v_pk_*) the fp32 products by what it finds around them.  A forced-inline function is optimised
// on its own before it is inlined; the same statements then reach the vectoriser in another order, it pairs them differently, and the
// last bits move (observed on gfx950: function forms changed the multiply / fma / packed mix of every kernel of mixture.hip, and of
// slp_optimise_kernel at some R).  Expanded in place, every kernel keeps the arithmetic it has always had, and there is still one copy
// of it.  A macro names every loop variable its arguments may use among its parameters: (i, j) the entry of the triangle, q its index.

// { body } for every entry (i, j <= i) of the lower triangle, in the packed (row-major) order q = 0 .. NT - 1.
#define GMM_TRI_EACH(R, i, j, q, ...)                                \
  {                                                                  \
    int q = 0;                                                       \
    _Pragma("unroll") for (int i = 0; i < R; ++i)                    \
      _Pragma("unroll") for (int j = 0; j < R; ++j)                  \
        if (j <= i) {                                                \
          __VA_ARGS__;                                               \
          ++q;                                                       \
        }                                                            \
  }

// Declares y_[R] = Linv (t - mean), the whitened residual of one component, and maha = |y_|^2.  `Li_q`: the expression in q for entry
// q of the packed Linv (prm[TRI + q], or a register array's element), `d_j`: the expression in j for (t - mean)[j].
#define GMM_WHITEN(R, q, Li_q, j, d_j, y_, maha)                     \
  float y_[R], maha = 0.f;                                           \
  {                                                                  \
    int q = 0;                                                       \
    _Pragma("unroll") for (int i_ = 0; i_ < R; ++i_) {               \
      float yi = 0.f;                                                \
      _Pragma("unroll") for (int j = 0; j < R; ++j)                  \
        if (j <= i_) {                                               \
          yi += (Li_q) * (d_j);                                      \
          ++q;                                                       \
        }                                                            \
      y_[i_] = yi;                                                   \
      maha += yi * yi;                                               \
    }                                                                \
  }

// Declares v_[R] = Linv^T y_, the back-projection: Sigma^-1 (t - mean) = Linv^T Linv (t - mean) = v_.
#define GMM_BACK_PROJECT(R, q, Li_q, y_, v_)                         \
  float v_[R];                                                       \
  _Pragma("unroll") for (int j = 0; j < R; ++j) v_[j] = 0.f;         \
  GMM_TRI_EACH(R, i_, j_, q, v_[j_] += (Li_q) * y_[i_])

// One step of the online log-sum-exp over a lane's components: folds the log-prob `lp` into the running maximum `mx` and declares
// `sc`, the factor that carries everything accumulated under the old maximum over to the new one, and `ex`, the term of this
// component:  se = se * sc + ex.  A component of weight exactly 0 has c_k = lp = -inf: while the running maximum is still -inf both
// differences would be NaN, which would then live on in every later step (and, in slp.hip, through every iteration and the chained
// state) -- such a component contributes nothing instead.
#define GMM_LSE_STEP(lp, mx, sc, ex)                                                                              \
  const float m2_ = fmaxf(mx, lp);                                                                                \
  const float sc = (mx == -INFINITY) ? 0.f : __expf(mx - m2_), ex = (m2_ == -INFINITY) ? 0.f : __expf(lp - m2_); \
  mx = m2_
