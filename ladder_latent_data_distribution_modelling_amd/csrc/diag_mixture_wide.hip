// VampPrior term on a WIDE code: crossEntropy_prior of prior "vampPrior" (codes/base.py:216-254, 361-370) for 80 <= Z <= 256, Z % 16 == 0 -- the
// equally weighted mixture of K diagonal Gaussians whose components are the encoder's outputs on the pseudo-inputs, over S = L*B MC samples
// t = mu[b] + sd[b] * eps[l,b].  Same outputs and signs as ladder_diag_mixture_fwd_bwd (csrc/mixture.hip), which keeps Z <= 64.
//
// The narrow kernel (workgroup per batch row, four private [K,Z] accumulator pairs in LDS) would need 410 KB of LDS at K = 50, Z = 256.  Here the two
// reductions of the term get a launch each, in the layout that makes each of them cheap:
//
//   prepare     one wavefront per component: m (copy), 1/s, c_k = -sum_j log s_kj - Z/2 log 2pi - log K into the workspace.
//   resp        the sum over Z.  A wavefront takes DW_NS samples, a lane four consecutive dimensions of each; per component one 16-byte load of m and
//               of 1/s serves all DW_NS samples, u = (t - m_k) / s_k is formed directly (never the expanded quadratic), a wavefront reduction gives
//               lp[s,k].  Lane k % 64 keeps lp[s,k]; it alone writes and re-reads that entry of r [S, Kp] for the max-subtracted log-sum-exp and
//               r = exp(lp - lse), so no other thread's store is ever read inside this launch.  float64 partial of lse per workgroup.
//   accumulate  the sums over the samples.  Grid (sample slice, chunk of DW_KC components), a thread is a latent dimension and keeps the chunk's
//               m, 1/s and both accumulators (2 * DW_KC) in registers; r[s, chunk] is four 16-byte loads at a wavefront-uniform address.  A slice is
//               (batch rows b = g, g + nbg, ..; a contiguous range of l), so the same pass also gives the chunk's share of dmu / dsd per row.
//               Every slice writes one [K,Z] partial pair, every (chunk, l-range) one [B,Z] partial pair.
//   reduce x2, sum   fixed-order sums of the partials (four interleaved running sums per element, combined as (0+1)+(2+3)).
//
// No floating-point atomics, no grid-wide synchronisation, no [S,K,Z] array; every partial that is read was written by the same call.
#include "diag_mixture_common.h"   // prepare kernel + component arithmetic, shared with csrc/iwll.hip

namespace {
constexpr int DW_NS = 4;                        // samples per wavefront of the resp launch
constexpr int DW_KC = 16;                       // components per workgroup of the accumulate launch
constexpr int DW_SLICES = 256;                  // sample slices of the accumulate launch: one per CU
constexpr size_t DW_PART_BYTES = (size_t)64 << 20;   // cap on the slices' [K,Z] partial pairs (K = 1024, Z = 256: 32 slices)

// How a shape is cut up, and where its pieces sit in the (256-byte aligned) workspace.  The query and the launch both come through here.
struct DwPlan {
  int nbg, lper, lsplit, nkc, kp, nblk;
  size_t o_m, o_is, o_c, o_r, o_lp, o_pm, o_ps, o_gm, o_gs, bytes;
};

size_t dw_align(size_t n) { return (n + 255) & ~(size_t)255; }

bool dw_shape_ok(int L, int B, int Z, int K) {
  return L >= 1 && B >= 1 && K >= 1 && K <= 1024 && Z >= 80 && Z <= 256 && Z % 16 == 0 && (size_t)L * B <= ((size_t)1 << 30);
}

DwPlan dw_plan(int L, int B, int Z, int K) {
  DwPlan p;
  const size_t S = (size_t)L * B, KZ = (size_t)K * Z;
  size_t cap = DW_PART_BYTES / (2 * KZ * sizeof(float));
  cap = cap < 1 ? 1 : (cap > DW_SLICES ? DW_SLICES : cap);
  p.nbg = B < (int)cap ? B : (int)cap;
  int ls = (int)cap / p.nbg;
  ls = ls < 1 ? 1 : (ls > L ? L : ls);
  p.lper = (L + ls - 1) / ls;
  p.lsplit = (L + p.lper - 1) / p.lper;                     // no empty l-range
  p.nkc = (K + DW_KC - 1) / DW_KC;
  p.kp = p.nkc * DW_KC;
  p.nblk = (int)((S + 4 * DW_NS - 1) / (4 * DW_NS));
  const size_t slices = (size_t)p.nbg * p.lsplit, parts = (size_t)p.nkc * p.lsplit;
  size_t o = 0;
  p.o_m = o;  o += dw_align(KZ * sizeof(float));
  p.o_is = o; o += dw_align(KZ * sizeof(float));
  p.o_c = o;  o += dw_align((size_t)K * sizeof(float));
  p.o_r = o;  o += dw_align(S * p.kp * sizeof(float));
  p.o_lp = o; o += dw_align((size_t)p.nblk * sizeof(double));
  p.o_pm = o; o += dw_align(slices * KZ * sizeof(float));
  p.o_ps = o; o += dw_align(slices * KZ * sizeof(float));
  p.o_gm = o; o += dw_align(parts * B * Z * sizeof(float));
  p.o_gs = o; o += dw_align(parts * B * Z * sizeof(float));
  p.bytes = o + 256;                                        // the entry aligns the caller's pointer itself
  return p;
}

__global__ __launch_bounds__(256) void dw_resp_kernel(const float* __restrict__ mu, const float* __restrict__ sd, const float* __restrict__ eps,
                                                      const float* __restrict__ m, const float* __restrict__ is, const float* __restrict__ c,
                                                      long S, int B, int Z, int K, int Kp, float* r, double* __restrict__ blk_lp) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int z0 = 4 * lane;
  const bool on = z0 < Z;                            // Z % 16 == 0: a lane holds four dimensions or none
  const long sbase = ((long)blockIdx.x * 4 + wv) * DW_NS;
  float t[DW_NS][4];
#pragma unroll
  for (int i = 0; i < DW_NS; ++i) {
    const long s = sbase + i < S ? sbase + i : S - 1;   // a wavefront past the end repeats the last sample and stores nothing
    const size_t b = (size_t)(s % B);
#pragma unroll
    for (int j = 0; j < 4; ++j) t[i][j] = on ? fmaf(sd[b * Z + z0 + j], eps[(size_t)s * Z + z0 + j], mu[b * Z + z0 + j]) : 0.f;
  }
  float mx[DW_NS];
#pragma unroll
  for (int i = 0; i < DW_NS; ++i) mx[i] = -INFINITY;
  // lp[s,k] -> r[s,k], lane k % 64 the owner; the padding k in [K, Kp) gets -inf, so its responsibility is an exact 0
  for (int kc = 0; kc < Kp; kc += 64) {
    float mine[DW_NS];
#pragma unroll
    for (int i = 0; i < DW_NS; ++i) mine[i] = -INFINITY;
    const int kend = K - kc < 64 ? K - kc : 64;
    for (int kk = 0; kk < kend; ++kk) {
      const size_t row = (size_t)(kc + kk) * Z + z0;
      const float4 mv = on ? *reinterpret_cast<const float4*>(m + row) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 iv = on ? *reinterpret_cast<const float4*>(is + row) : make_float4(0.f, 0.f, 0.f, 0.f);
      const float ck = c[kc + kk];
#pragma unroll
      for (int i = 0; i < DW_NS; ++i) {
        const float v = dw_component_logp(dw_quad_partial(t[i], mv, iv), ck);
        if (lane == kk) mine[i] = v;
      }
    }
    if (kc + lane < Kp) {
#pragma unroll
      for (int i = 0; i < DW_NS; ++i) {
        if (sbase + i < S) r[(size_t)(sbase + i) * Kp + kc + lane] = mine[i];
        mx[i] = fmaxf(mx[i], mine[i]);
      }
    }
  }
  double acc_lp = 0.0;
#pragma unroll
  for (int i = 0; i < DW_NS; ++i) {
    if (sbase + i >= S) continue;                    // wavefront-uniform
    float* row = r + (size_t)(sbase + i) * Kp;
    const float top = wave_max(mx[i]);
    float se = 0.f;
    for (int k = lane; k < Kp; k += 64) se += expf(row[k] - top);
    se = wave_sum(se);
    const float lse = top + logf(se);
    acc_lp += (double)lse;
    for (int k = lane; k < Kp; k += 64) row[k] = expf(row[k] - lse);
  }
  __shared__ double red[4];
  if (lane == 0) red[wv] = acc_lp;
  __syncthreads();
  if (threadIdx.x == 0) blk_lp[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void dw_accum_kernel(const float* __restrict__ mu, const float* __restrict__ sd, const float* __restrict__ eps,
                                                       const float* __restrict__ m, const float* __restrict__ is, const float* __restrict__ r,
                                                       int L, int B, int Z, int K, int Kp, int nbg, int lper, int lsplit,
                                                       float* __restrict__ pm, float* __restrict__ ps, float* __restrict__ gm_part,
                                                       float* __restrict__ gs_part) {
  const int z = threadIdx.x;
  const bool on = z < Z;
  const int slice = blockIdx.x, kc = blockIdx.y;
  const int bg = slice % nbg, lj = slice / nbg;
  const int l0 = lj * lper, l1 = l0 + lper < L ? l0 + lper : L;
  const int k0 = kc * DW_KC;
  float mk[DW_KC], ik[DW_KC], am[DW_KC], as[DW_KC];
#pragma unroll
  for (int j = 0; j < DW_KC; ++j) {
    const bool v = on && k0 + j < K;                  // a padding component: m = 1/s = r = 0, so it adds exact zeros
    mk[j] = v ? m[(size_t)(k0 + j) * Z + z] : 0.f;
    ik[j] = v ? is[(size_t)(k0 + j) * Z + z] : 0.f;
    am[j] = 0.f;
    as[j] = 0.f;
  }
  for (int b = bg; b < B; b += nbg) {
    const float m_ = on ? mu[(size_t)b * Z + z] : 0.f, s_ = on ? sd[(size_t)b * Z + z] : 0.f;
    float g_mu = 0.f, g_sd = 0.f;
    for (int l = l0; l < l1; ++l) {
      const size_t s = (size_t)l * B + b;
      const float e = on ? eps[s * Z + z] : 0.f;
      const float t = fmaf(s_, e, m_);
      const float4* rr = reinterpret_cast<const float4*>(r + s * Kp + k0);   // the same address in every lane
      float rv[DW_KC];
#pragma unroll
      for (int j = 0; j < DW_KC / 4; ++j) {
        const float4 q = rr[j];
        rv[4 * j] = q.x; rv[4 * j + 1] = q.y; rv[4 * j + 2] = q.z; rv[4 * j + 3] = q.w;
      }
      float gt = 0.f;
#pragma unroll
      for (int j = 0; j < DW_KC; ++j) {
        const float u = (t - mk[j]) * ik[j];
        const float ru = rv[j] * u;                   // s_k * dlogp/dm_k of this sample
        am[j] += ru;
        as[j] = fmaf(rv[j], fmaf(u, u, -1.f), as[j]);
        gt = fmaf(-ru, ik[j], gt);                    // dlogp/dt
      }
      g_mu += gt;
      g_sd = fmaf(gt, e, g_sd);
    }
    if (on) {
      const size_t o = (((size_t)kc * lsplit + lj) * B + b) * Z + z;
      gm_part[o] = g_mu;
      gs_part[o] = g_sd;
    }
  }
  if (on) {
#pragma unroll
    for (int j = 0; j < DW_KC; ++j)
      if (k0 + j < K) {
        const size_t o = ((size_t)slice * K + k0 + j) * Z + z;
        pm[o] = am[j] * ik[j];
        ps[o] = as[j] * ik[j];
      }
  }
}

// dst[i] = sum_p src[p][i], i < n, for two arrays (blockIdx.y): four running sums over p = g, g + 4, .. combined as (0 + 1) + (2 + 3)
__global__ __launch_bounds__(256) void dw_reduce_kernel(const float* __restrict__ src0, const float* __restrict__ src1, int P, size_t n,
                                                        float* __restrict__ dst0, float* __restrict__ dst1) {
  __shared__ float sh[4][64];
  const float* src = blockIdx.y ? src1 : src0;
  float* dst = blockIdx.y ? dst1 : dst0;
  const int lane = threadIdx.x & 63, g = threadIdx.x >> 6;
  const size_t i = (size_t)blockIdx.x * 64 + lane;
  float a = 0.f;
  if (i < n)
    for (int p = g; p < P; p += 4) a += src[(size_t)p * n + i];
  sh[g][lane] = a;
  __syncthreads();
  if (g == 0 && i < n) dst[i] = (sh[0][lane] + sh[1][lane]) + (sh[2][lane] + sh[3][lane]);
}

__global__ __launch_bounds__(64) void dw_sum_kernel(const double* __restrict__ blk_lp, int n, float* __restrict__ out) {
  double s = 0.0;                                     // lane-strided partial sums, then a fixed-order shuffle tree
  for (int i = threadIdx.x; i < n; i += 64) s += blk_lp[i];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) out[0] = (float)s;
}
}  // namespace

extern "C" {

size_t ladder_diag_mixture_wide_workspace_bytes(int L, int B, int Z, int K) { return dw_shape_ok(L, B, Z, K) ? dw_plan(L, B, Z, K).bytes : 0; }

int ladder_diag_mixture_wide_fwd_bwd(const float* mu, const float* sd, const float* eps, const float* comp_mean, const float* comp_sd, int L, int B,
                                     int Z, int K, float* sum_logp, float* dmu, float* dsd, float* dcomp_mean, float* dcomp_sd, void* ws,
                                     size_t ws_bytes, ladder_stream_t stream) {
  if (!dw_shape_ok(L, B, Z, K)) return LADDER_E_SHAPE;
  const DwPlan p = dw_plan(L, B, Z, K);
  if (ws == nullptr || ws_bytes < p.bytes) return LADDER_E_WORKSPACE;
  char* w = (char*)(((uintptr_t)ws + 255) & ~(uintptr_t)255);
  float* m = (float*)(w + p.o_m);
  float* is = (float*)(w + p.o_is);
  float* c = (float*)(w + p.o_c);
  float* r = (float*)(w + p.o_r);
  double* blk_lp = (double*)(w + p.o_lp);
  float* pm = (float*)(w + p.o_pm);
  float* ps = (float*)(w + p.o_ps);
  float* gm = (float*)(w + p.o_gm);
  float* gs = (float*)(w + p.o_gs);
  const long S = (long)L * B;
  const size_t KZ = (size_t)K * Z, BZ = (size_t)B * Z;
  const int slices = p.nbg * p.lsplit;
  hipLaunchKernelGGL(dw_prepare_kernel, dim3(K), dim3(64), 0, stream, comp_mean, comp_sd, Z, Z, K, m, is, c);
  hipLaunchKernelGGL(dw_resp_kernel, dim3(p.nblk), dim3(256), 0, stream, mu, sd, eps, (const float*)m, (const float*)is, (const float*)c, S, B, Z, K,
                     p.kp, r, blk_lp);
  hipLaunchKernelGGL(dw_accum_kernel, dim3(slices, p.nkc), dim3((Z + 63) / 64 * 64), 0, stream, mu, sd, eps, (const float*)m, (const float*)is,
                     (const float*)r, L, B, Z, K, p.kp, p.nbg, p.lper, p.lsplit, pm, ps, gm, gs);
  hipLaunchKernelGGL(dw_reduce_kernel, dim3((unsigned)((KZ + 63) / 64), 2), dim3(256), 0, stream, (const float*)pm, (const float*)ps, slices, KZ,
                     dcomp_mean, dcomp_sd);
  hipLaunchKernelGGL(dw_reduce_kernel, dim3((unsigned)((BZ + 63) / 64), 2), dim3(256), 0, stream, (const float*)gm, (const float*)gs,
                     p.nkc * p.lsplit, BZ, dmu, dsd);
  hipLaunchKernelGGL(dw_sum_kernel, dim3(1), dim3(64), 0, stream, (const double*)blk_lp, p.nblk, sum_logp);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}
}  // extern "C"
