// What the batch-norm and instance-norm passes of csrc/norm.hip share: the normalise expression and its backward counterpart, written once
// for 1 or 4 consecutive channels; the finalisation of the fp64 statistics record; the coefficient loaders; the fixed-order combination of
// a workgroup's row lanes.
#pragma once
#include "common.h"

// V values of consecutive channels (V = 4: one 16-byte access, C % 4 == 0 and a 16-byte aligned base).
template <typename S, int V>
struct alignas(sizeof(S) * V < 16 ? sizeof(S) * V : 16) Lanes {
  S v[V];
};
template <int V>
__device__ __forceinline__ Lanes<float, V> lanes_load(const float* __restrict__ p) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    return {{t.x, t.y, t.z, t.w}};
  } else {
    return {{p[0]}};
  }
}
template <typename S, int V>
__device__ __forceinline__ void lanes_store(S* __restrict__ p, const Lanes<S, V>& a) {
  if constexpr (V == 4 && sizeof(S) == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
  } else {
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = a.v[j];
  }
}
template <typename S, int V>
__device__ __forceinline__ Lanes<S, V> lanes_fill(S s) {
  Lanes<S, V> a;
#pragma unroll
  for (int j = 0; j < V; ++j) a.v[j] = s;
  return a;
}
// max(m, max_j |a_j|)
template <int V>
__device__ __forceinline__ float lanes_absmax(float m, const Lanes<float, V>& a) {
  if constexpr (V == 4) return fmaxf(fmaxf(m, fmaxf(fabsf(a.v[0]), fabsf(a.v[1]))), fmaxf(fabsf(a.v[2]), fabsf(a.v[3])));
  else return fmaxf(m, fabsf(a.v[0]));
}

// ---- the normalise expression ----------------------------------------------------------------------------------------------------------
// y = act(scale * xhat + shift), xhat = (x - mean) * rstd.  Batch norm: scale = gamma, shift = beta.  Instance norm + style modulation:
// scale = style[0:C] + 1, shift = style[C:2C].
// ROUNDING IS SPELLED OUT HERE: the library is built with -ffp-contract=fast, under which the compiler decides per call site -- and, where
// the vectoriser pairs operations, per channel of a float4 -- which products it fuses into the addition that consumes them (a
// `#pragma clang fp contract(off)` does not stop it: the option also lets the backend fuse whatever it meets).  The copies of these
// expressions that the kernels carried before had ended up with the fusions below at (nearly) every site.  Here the fused operations are
// fmaf and a product that is to be rounded on its own passes through rounded(), so every caller rounds alike whatever surrounds the call.
__device__ __forceinline__ float rounded(float v) {
  asm("" : "+v"(v));                                   // (no instruction: the compiler just cannot see through it)
  return v;
}
template <int V>
struct NormCoef {
  float mean[V], rstd[V], scale[V], shift[V];
};
// xhat, and y in front of the activation: one subtraction, one product, one fused multiply-add
template <int V>
__device__ __forceinline__ void norm_pre(const Lanes<float, V>& x, const NormCoef<V>& k, Lanes<float, V>& xh, Lanes<float, V>& pre) {
#pragma unroll
  for (int j = 0; j < V; ++j) {
    xh.v[j] = (x.v[j] - k.mean[j]) * k.rstd[j];
    pre.v[j] = fmaf(k.scale[j], xh.v[j], k.shift[j]);
  }
}
template <int V>
__device__ __forceinline__ Lanes<float, V> norm_act(const Lanes<float, V>& x, const NormCoef<V>& k, int act) {
  Lanes<float, V> xh, y;
  norm_pre(x, k, xh, y);
#pragma unroll
  for (int j = 0; j < V; ++j) y.v[j] = ladder_act_fn(y.v[j], act);
  return y;
}
__device__ __forceinline__ float norm_act(float x, const NormCoef<1>& k, int act) { return norm_act<1>({{x}}, k, act).v[0]; }
// backward: xh = xhat, grad = act'(y); the gradient in front of the activation is dp = dy * grad
template <int V>
__device__ __forceinline__ void norm_bwd_terms(const Lanes<float, V>& x, const NormCoef<V>& k, int act, Lanes<float, V>& xh, Lanes<float, V>& grad) {
  norm_pre(x, k, xh, grad);
#pragma unroll
  for (int j = 0; j < V; ++j) grad.v[j] = ladder_act_grad_from_out(grad.v[j], act);
}
__device__ __forceinline__ void norm_bwd_terms(float x, const NormCoef<1>& k, int act, float& xh, float& grad) {
  Lanes<float, 1> h, g;
  norm_bwd_terms<1>({{x}}, k, act, h, g);
  xh = h.v[0];
  grad = g.v[0];
}
// ... its two running sums: dp and dp * xh are both rounded before they are added (every statistics kernel; which slot of a record each
// sum lands in is the layer's business)
template <int V>
__device__ __forceinline__ void norm_bwd_accumulate(const Lanes<float, V>& x, const Lanes<float, V>& dy, const NormCoef<V>& k, int act,
                                                    Lanes<float, V>& sum_dp, Lanes<float, V>& sum_dp_xh) {
  Lanes<float, V> xh, grad;
  norm_bwd_terms(x, k, act, xh, grad);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const float dp = rounded(dy.v[j] * grad.v[j]);
    sum_dp.v[j] += dp;
    sum_dp_xh.v[j] += rounded(dp * xh.v[j]);
  }
}
// ... and dx = scale * rstd * (dp - m1 - xh * m2), m1 = mean of dp, m2 = mean of dp * xh over the normalised axis: dp is never rounded
// (dy * grad - m1 is one fused operation), nor is xh * m2
template <int V>
__device__ __forceinline__ Lanes<float, V> norm_dx(const Lanes<float, V>& xh, const Lanes<float, V>& dy, const Lanes<float, V>& grad, const NormCoef<V>& k,
                                                   const Lanes<float, V>& m1, const Lanes<float, V>& m2) {
  Lanes<float, V> dx;
#pragma unroll
  for (int j = 0; j < V; ++j) dx.v[j] = (k.scale[j] * k.rstd[j]) * fmaf(-xh.v[j], m2.v[j], fmaf(dy.v[j], grad.v[j], -m1.v[j]));
  return dx;
}

// ---- coefficients ------------------------------------------------------------------------------------------------------------------------
// mean and 1 / sd of channel c from the fp64 statistics record (sum x | sum x^2, 2C doubles; see the record's description in norm.hip)
__device__ __forceinline__ void bn_moments(const float* __restrict__ record, int C, int c, double count, float eps, float& mean, float& rstd) {
  const double* s64 = reinterpret_cast<const double*>(record);
  const double m = s64[c] / count;
  double var = s64[C + c] / count - m * m;
  if (var < 0.0) var = 0.0;
  mean = (float)m;
  rstd = (float)(1.0 / sqrt(var + (double)eps));
}
// batch norm: mean_rstd [2C] = mean | 1 / sd
template <int V>
__device__ __forceinline__ NormCoef<V> bn_coef(const float* __restrict__ mean_rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                               int C, int c) {
  const Lanes<float, V> mu = lanes_load<V>(mean_rstd + c), rs = lanes_load<V>(mean_rstd + C + c), g = lanes_load<V>(gamma + c), be = lanes_load<V>(beta + c);
  NormCoef<V> k;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    k.mean[j] = mu.v[j]; k.rstd[j] = rs.v[j]; k.scale[j] = g.v[j]; k.shift[j] = be.v[j];
  }
  return k;
}
// instance norm of sample n: mean_rstd [N][2C] = mean | 1 / sd, style [N][2C] = scale - 1 | shift
template <int V>
__device__ __forceinline__ NormCoef<V> in_coef(const float* __restrict__ mean_rstd, const float* __restrict__ style, int n, int C, int c) {
  const size_t o = (size_t)n * 2 * C + c;
  const Lanes<float, V> mu = lanes_load<V>(mean_rstd + o), rs = lanes_load<V>(mean_rstd + o + C), s0 = lanes_load<V>(style + o), s1 = lanes_load<V>(style + o + C);
  NormCoef<V> k;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    k.mean[j] = mu.v[j]; k.rstd[j] = rs.v[j]; k.scale[j] = s0.v[j] + 1.f; k.shift[j] = s1.v[j];
  }
  return k;
}

// ---- row lanes of a workgroup, combined in a fixed order ---------------------------------------------------------------------------------
struct LaneAdd {
  template <typename S> static __device__ __forceinline__ S f(S a, S b) { return a + b; }
};
struct LaneMin {
  static __device__ __forceinline__ float f(float a, float b) { return fminf(a, b); }
};
struct LaneMax {
  static __device__ __forceinline__ float f(float a, float b) { return fmaxf(a, b); }
};
// 16 row lanes x 16 channel quads: sm[lane][quad] holds every lane's value (written before a barrier); lane 0 first, then 1 .. 15 in order.
// (A sum may start from lane 0 instead of from zero: every lane's accumulator starts at +0, so none holds -0, and 0 + s = s bit for bit.)
template <typename Op, typename S>
__device__ __forceinline__ Lanes<S, 4> rowlane16_reduce(const Lanes<S, 4> (*sm)[16], int cq) {
  Lanes<S, 4> t = sm[0][cq];
#pragma unroll
  for (int k = 1; k < 16; ++k) {
    const Lanes<S, 4> v = sm[k][cq];
#pragma unroll
    for (int j = 0; j < 4; ++j) t.v[j] = Op::f(t.v[j], v.v[j]);
  }
  return t;
}
// 4 row lanes x 64 channels: pairwise.  EVERY thread must call it (two barriers, so sm can be reused); valid in every thread.
template <typename S>
__device__ __forceinline__ S block_rowlane_sum(S v, S (*sm)[64], int rl, int cl) {
  __syncthreads();
  sm[rl][cl] = v;
  __syncthreads();
  return (sm[0][cl] + sm[1][cl]) + (sm[2][cl] + sm[3][cl]);
}
