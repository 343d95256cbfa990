// Component arithmetic of the equally weighted diagonal Gaussian mixture (the VampPrior, codes/base.py:216-254), shared by the training term on a
// wide code (csrc/diag_mixture_wide.hip) and the per-row log-density of the evaluation (csrc/iwll.hip): the prepared form of the components
// (m, 1/s, c_k), a lane's share of sum_j u_j^2 with u = (t - m_k) / s_k formed directly, and the component's log-density from it.
#pragma once
#include "common.h"

namespace {
constexpr float kHalfLog2Pi = 0.91893853320467274f;

// One wavefront per component: m (copy), 1/s and c_k = -sum_j log s_kj - Z/2 log 2pi - log K.  Rows of m and 1/s are `ld` >= Z floats apart; the
// columns [Z, ld) are written as zeros, so a reader that takes whole 16-byte groups of a padded row adds exact zeros for them.
__global__ __launch_bounds__(64) void dw_prepare_kernel(const float* __restrict__ cm, const float* __restrict__ cs, int Z, int ld, int K,
                                                        float* __restrict__ m, float* __restrict__ is, float* __restrict__ c) {
  const int k = blockIdx.x, lane = threadIdx.x;
  float ls = 0.f;
  for (int z = lane; z < Z; z += 64) {
    const float s = cs[(size_t)k * Z + z];
    m[(size_t)k * ld + z] = cm[(size_t)k * Z + z];
    is[(size_t)k * ld + z] = 1.f / s;
    ls += logf(s);
  }
  for (int z = Z + lane; z < ld; z += 64) {
    m[(size_t)k * ld + z] = 0.f;
    is[(size_t)k * ld + z] = 0.f;
  }
  ls = wave_sum(ls);
  if (lane == 0) c[k] = -ls - (float)Z * kHalfLog2Pi - logf((float)K);
}

// A lane's four consecutive dimensions of one (point, component) pair: its share of sum_j ((t_j - m_kj) / s_kj)^2, combined as (0 + 1) + (2 + 3).
__device__ __forceinline__ float dw_quad_partial(const float (&t)[4], const float4 mv, const float4 iv) {
  const float u0 = (t[0] - mv.x) * iv.x, u1 = (t[1] - mv.y) * iv.y, u2 = (t[2] - mv.z) * iv.z, u3 = (t[3] - mv.w) * iv.w;
  return (u0 * u0 + u1 * u1) + (u2 * u2 + u3 * u3);
}
// log (1/K) N(t; m_k, diag s_k^2) from the lanes' shares; every lane of the wavefront gets the value.
__device__ __forceinline__ float dw_component_logp(float partial, float ck) { return fmaf(-0.5f, wave_sum(partial), ck); }
}  // namespace
