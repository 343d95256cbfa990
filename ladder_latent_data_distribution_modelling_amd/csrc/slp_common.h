// The part of the shortest-likely-path iteration that does not depend on how the mixture term is computed: shared by the narrow kernel
// (csrc/slp.hip, R <= 8, R a template constant) and the wide one (csrc/slp_wide.hip, 8 < R <= 64, R a run-time value).  All of it is
// float64 with contraction off, so the statements give the same bits whether `R` is a constant the compiler unrolls over or a loop
// bound it reads at run time (codes/interpolation.py: path_terms and SLPInterpolator.optimise are the host forms).
//
// Both kernels keep, in LDS and for the whole launch: s_full = start | the n_step points | end, the Adam moments s_m / s_v, and per
// iteration the unit vectors s_unit [n_step + 1, R], d std / d len s_c [n_step + 1], s_scal = {path length, std, Adam step size}, the fp32
// mixture gradient s_gn [n_step, R] (dense) and the log-probs s_lp [n_step].
#pragma once
#include "common.h"

constexpr int SLP_THREADS = 256, SLP_WAVES = SLP_THREADS / 64, SLP_MAX_STEP = 64;

struct SlpArgs {
  const float* start;
  const float* end;
  float* pts;
  const float* packed;         // narrow: ladder_gmm_prepare's buffer; wide: ladder_gmm_prepare_dense's
  int K, n_step, n_iter, t0;
  double lr, beta1, beta2, eps, clip, w_path, w_equal;
  double* state;
  double* record;
  size_t plane;                // P * n_step * R: elements of one plane of `state` (points | m | v)
};

// End points, points and moments of path p into LDS: from `state` when the launch resumes (t0 > 0), else from pts with zero moments.
__device__ __forceinline__ void slp_load_path(const SlpArgs& A, const int R, const int tid, const size_t p, double* s_full, double* s_m, double* s_v) {
  const int n = A.n_step, ne = n * R;
  const size_t base = p * (size_t)ne;
  double* s_pts = s_full + R;
  if (tid < R) {
    s_full[tid] = (double)A.start[p * R + tid];
    s_full[(n + 1) * R + tid] = (double)A.end[p * R + tid];
  }
  for (int e = tid; e < ne; e += SLP_THREADS) {
    if (A.t0 > 0) {
      s_pts[e] = A.state[base + e];
      s_m[e] = A.state[A.plane + base + e];
      s_v[e] = A.state[2 * A.plane + base + e];
    } else {
      s_pts[e] = (double)A.pts[base + e];
      s_m[e] = 0.0;
      s_v[e] = 0.0;
    }
  }
}

// The fp32 rounding of the points to pts, the float64 points and moments to `state`.
__device__ __forceinline__ void slp_store_path(const SlpArgs& A, const int R, const int tid, const size_t p, const double* s_full, const double* s_m, const double* s_v) {
  const int ne = A.n_step * R;
  const size_t base = p * (size_t)ne;
  const double* s_pts = s_full + R;
  for (int e = tid; e < ne; e += SLP_THREADS) {
    A.pts[base + e] = (float)s_pts[e];
    if (A.state != nullptr) {
      A.state[base + e] = s_pts[e];
      A.state[A.plane + base + e] = s_m[e];
      A.state[2 * A.plane + base + e] = s_v[e];
    }
  }
}

// Path algebra of iteration `it` for ONE wavefront (all 64 lanes active): segment lengths, their mean / population std, the unit vectors,
// d std / d len and the bias-corrected Adam step size of the absolute iteration t0 + it + 1.
__device__ __forceinline__ void slp_path_algebra(const SlpArgs& A, const int R, const int lane, const int it, const double* s_full, double* s_unit, double* s_c,
                                                 double* s_scal) {
#pragma clang fp contract(off)
  const int ns = A.n_step + 1;                             // segments; a lane owns segments lane and lane + 64 (ns <= 65)
  double ln_[2] = {0.0, 0.0}, sum = 0.0;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int s = lane + 64 * h;
    if (s < ns) {
      double q = 0.0;
#pragma unroll
      for (int j = 0; j < R; ++j) {
        const double d = s_full[(s + 1) * R + j] - s_full[s * R + j];
        q += d * d;
      }
      ln_[h] = sqrt(q);
      sum += ln_[h];
    }
  }
  sum = wave_sum_d(sum);
  const double mean = sum / (double)ns;
  double var = 0.0;
#pragma unroll
  for (int h = 0; h < 2; ++h)
    if (lane + 64 * h < ns) var += (ln_[h] - mean) * (ln_[h] - mean);
  var = wave_sum_d(var) / (double)ns;
  const double sd = sqrt(var);                             // population standard deviation (tf.math.reduce_std)
  const double cden = (double)ns * fmax(sd, 1e-30);
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int s = lane + 64 * h;
    if (s < ns) {
      const double den = fmax(ln_[h], 1e-30);
#pragma unroll
      for (int j = 0; j < R; ++j) s_unit[s * R + j] = (s_full[(s + 1) * R + j] - s_full[s * R + j]) / den;
      s_c[s] = (ln_[h] - mean) / cden;                     // d std / d len_s
    }
  }
  if (lane == 0) {
    const double t = (double)(A.t0 + it + 1);
    s_scal[0] = sum;
    s_scal[1] = sd;
    s_scal[2] = A.lr * sqrt(1.0 - pow(A.beta2, t)) / (1.0 - pow(A.beta1, t));
  }
}

// Phase B for the whole workgroup: every thread owns elements of the [n_step, R] point array -- raw gradient in float64, element-wise
// clip, Adam moments and the step; wavefront 0 sums -log p over the points in double (lane-strided, then the fixed shuffle tree) and
// writes the record row of iteration `it`.
__device__ __forceinline__ void slp_clip_adam_record(const SlpArgs& A, const int R, const int tid, const size_t p, const int it, double* s_full, double* s_m,
                                                     double* s_v, const double* s_unit, const double* s_c, const double* s_scal, const float* s_gn,
                                                     const float* s_lp) {
#pragma clang fp contract(off)
  const int lane = tid & 63, wv = tid >> 6, n = A.n_step, ne = n * R;
  double* s_pts = s_full + R;
  const double step = s_scal[2];
  for (int e = tid; e < ne; e += SLP_THREADS) {
    const int i = e / R, j = e - i * R;
    const double u0 = s_unit[i * R + j], u1 = s_unit[(i + 1) * R + j];
    const double g_len = u0 - u1;                          // + from the segment ending at p_i, - from the one leaving it
    const double g_std = s_c[i] * u0 - s_c[i + 1] * u1;
    double g = A.w_path * g_len + A.w_equal * g_std + (double)s_gn[e];
    g = fmin(fmax(g, -A.clip), A.clip);                    // model.ClipIfNotNone
    const double m = A.beta1 * s_m[e] + (1.0 - A.beta1) * g;
    const double v = A.beta2 * s_v[e] + (1.0 - A.beta2) * g * g;
    s_m[e] = m;
    s_v[e] = v;
    s_pts[e] = s_pts[e] - step * m / (sqrt(v) + A.eps);
  }
  if (A.record != nullptr && wv == 0) {
    double nll = 0.0;
    for (int i = lane; i < n; i += 64) nll -= (double)s_lp[i];
    nll = wave_sum_d(nll);
    if (lane == 0) {
      double* r = A.record + (p * (size_t)A.n_iter + it) * 4;
      r[0] = A.w_path * s_scal[0] + A.w_equal * s_scal[1] + nll;
      r[1] = s_scal[0];
      r[2] = s_scal[1];
      r[3] = nll;
    }
  }
}
