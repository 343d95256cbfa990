// Batched shortest-likely-path (SLP) interpolation: the optimisation loop of the reference's notebook
// `latent-space-interpolation-mnist.ipynb` (cells 18-23) for P paths at once, the whole clip + Adam loop inside ONE launch.
//
//     objective(pts) = w_path * sum_i |p_{i+1} - p_i|  +  w_equal * std_i |p_{i+1} - p_i|  -  sum_i log p_GM(p_i)
//
// One workgroup (4 wavefronts) per path; paths never communicate, so a path's result does not depend on P or on its index.  The only
// synchronisation is __syncthreads(), reached by every thread: n_iter, n_step and K are uniform over the workgroup.  No atomics.
//
// Per iteration:
//   phase A  mixture term: a wavefront takes a point (points beyond the wave count are looped over), lane = component, K in chunks of 64,
//            the per-component arithmetic of gmm_packed.h (shared with csrc/mixture.hip): lp_k = c_k - 0.5 |Linv_k (t - m_k)|^2 in
//            fp32 at the fp32-rounded point, online log-sum-exp per lane, then across lanes by wave shuffles; the gradient numerators
//            sum_k exp(lp_k - max) Linv_k^T y_k ride the same rescaling.  The LAST wavefront -- the one with the fewest points when n_step is
//            no multiple of 4 -- also forms the segment lengths, their mean / population std, the unit vectors and d std / d len in float64
//            (codes/interpolation.py: path_terms, same guards) and the bias-corrected Adam step size of this iteration.
//   phase B  every thread owns elements of the [n_step, R] point array: raw gradient in float64, element-wise clip, Adam moments and the
//            step, all float64 as in SLPInterpolator.optimise; wavefront 0 sums -log p over the points in double (lane-strided, then the
//            fixed shuffle tree) and writes the record row.
// Points and both moments live in LDS as float64 for the whole launch; `state` carries them between chained launches, and because the
// step size is a function of the absolute iteration number t (pow, not a running product) a chained run equals a single launch bit for bit.
// Everything but the mixture term -- loading and storing a path, the path algebra, phase B -- is csrc/slp_common.h, shared with the kernel for
// wide representations (csrc/slp_wide.hip, 8 < R <= 64).
#include "common.h"
#include "gmm_packed.h"
#include "slp_common.h"

namespace {

// LDS budget for the packed mixture: 4096 floats = 16 KB (K = 64, R = 8 is 2880 floats = 11.5 KB; with the <= 21 KB of float64 path state a
// workgroup stays below 40 KB, four workgroups per CU).  A larger mixture is read from global memory, where its <= 180 KB stay cache-resident.
constexpr int SLP_LDS_FLOATS = 4096;

// log p(t) and -d log p / d t of one point for the calling wavefront (all 64 lanes active); results valid on every lane.
template <int R>
__device__ __forceinline__ float slp_point(const float* __restrict__ prm_base, int K, int lane, const float (&t_)[R], float (&gout)[R]) {
  constexpr int STRIDE = GmmPacked<R>::STRIDE, MEAN = GmmPacked<R>::MEAN, TRI = GmmPacked<R>::TRI;
  float mx = -INFINITY, se = 0.f, g_[R];
#pragma unroll
  for (int j = 0; j < R; ++j) g_[j] = 0.f;
  for (int k = lane; k < K; k += 64) {
    const float* prm = prm_base + (size_t)k * STRIDE;
    GMM_WHITEN(R, q, prm[TRI + q], j, t_[j] - prm[MEAN + j], y_, maha);
    const float lp = prm[0] - 0.5f * maha;
    GMM_LSE_STEP(lp, mx, sc, ex);
    se = se * sc + ex;
    GMM_BACK_PROJECT(R, q, prm[TRI + q], y_, v_);
#pragma unroll
    for (int j = 0; j < R; ++j) g_[j] = g_[j] * sc + ex * v_[j];
  }
  const float gm = wave_max(mx);
  const float sc = (mx == -INFINITY) ? 0.f : __expf(mx - gm);   // lanes without a component
  se = wave_sum(se * sc);
  const float inv = 1.f / se;
#pragma unroll
  for (int j = 0; j < R; ++j) gout[j] = wave_sum(g_[j] * sc) * inv;   // -d lp / d t_j = sum_k r_k (Sigma_k^-1 (t - m_k))_j
  return gm + logf(se);
}

template <int R>
__global__ __launch_bounds__(SLP_THREADS) void slp_optimise_kernel(SlpArgs A) {
  __shared__ double s_full[(SLP_MAX_STEP + 2) * R];          // start | the n_step points | end
  __shared__ double s_m[SLP_MAX_STEP * R], s_v[SLP_MAX_STEP * R];
  __shared__ double s_unit[(SLP_MAX_STEP + 1) * R], s_c[SLP_MAX_STEP + 1];
  __shared__ double s_scal[3];                               // path length, std of the segment lengths, Adam step size
  __shared__ float s_gn[SLP_MAX_STEP * R], s_lp[SLP_MAX_STEP];
  __shared__ float s_packed[SLP_LDS_FLOATS];

  constexpr int STRIDE = GmmPacked<R>::STRIDE;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = A.n_step, K = A.K;
  const size_t p = blockIdx.x;
  const double* s_pts = s_full + R;
  const bool in_lds = K * STRIDE <= SLP_LDS_FLOATS;

  if (in_lds)
    for (int i = tid; i < K * STRIDE; i += SLP_THREADS) s_packed[i] = A.packed[i];
  slp_load_path(A, R, tid, p, s_full, s_m, s_v);
  __syncthreads();

  for (int it = 0; it < A.n_iter; ++it) {
    // ---- phase A: mixture term per point; the last wavefront also does the path algebra
    for (int i = wv; i < n; i += SLP_WAVES) {
      float t_[R], g_[R];
#pragma unroll
      for (int j = 0; j < R; ++j) t_[j] = (float)s_pts[i * R + j];
      const float lp = in_lds ? slp_point<R>(s_packed, K, lane, t_, g_) : slp_point<R>(A.packed, K, lane, t_, g_);
      if (lane == 0) {
        s_lp[i] = lp;
#pragma unroll
        for (int j = 0; j < R; ++j) s_gn[i * R + j] = g_[j];
      }
    }
    if (wv == SLP_WAVES - 1) slp_path_algebra(A, R, lane, it, s_full, s_unit, s_c, s_scal);
    __syncthreads();

    // ---- phase B: clip + Adam on the n_step * R elements, record row
    slp_clip_adam_record(A, R, tid, p, it, s_full, s_m, s_v, s_unit, s_c, s_scal, s_gn, s_lp);
    __syncthreads();
  }

  slp_store_path(A, R, tid, p, s_full, s_m, s_v);
}

}  // namespace

extern "C" {

size_t ladder_slp_state_bytes(int P, int n_step, int R) {
  if (P < 1 || n_step < 1 || R < 1) return 0;
  return (size_t)3 * P * n_step * R * sizeof(double);
}

int ladder_slp_optimise(const float* start, const float* end, float* pts, const float* packed, int K, int R, int P, int n_step, int n_iter,
                        int t0, double lr, double beta1, double beta2, double eps, double clip, double w_path, double w_equal, double* state,
                        double* record, ladder_stream_t stream) {
  if (start == nullptr || end == nullptr || pts == nullptr || packed == nullptr) return LADDER_E_SHAPE;
  if (K < 1 || K > 1024 || P < 1 || n_step < 1 || n_step > SLP_MAX_STEP || n_iter < 1 || n_iter > 4096 || t0 < 0) return LADDER_E_SHAPE;
  if (t0 > 0 && state == nullptr) return LADDER_E_SHAPE;
  SlpArgs A{start, end, pts, packed, K, n_step, n_iter, t0, lr, beta1, beta2, eps, clip, w_path, w_equal, state, record, (size_t)0};
  LADDER_R_SWITCH(R, A.plane = (size_t)P * n_step * RR; hipLaunchKernelGGL(slp_optimise_kernel<RR>, dim3((unsigned)P), dim3(SLP_THREADS), 0, stream, A));
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
