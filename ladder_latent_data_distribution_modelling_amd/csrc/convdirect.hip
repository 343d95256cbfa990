// Direct (no MFMA) convolution kernels for tiny channel counts, where a GEMM tile would be mostly padding: conv_smallcin_kernel (1x1 from
// 3 channels), conv_cout1_kernel (5x5 VALID to one channel) and conv1x1_smallcout_kernel (1x1 to <= 4 channels), with their eligibility
// rules and launchers (called by the exports of igemm.hip / igemm_wgrad.hip) and the exports that are theirs alone.
#include "igemm.h"

namespace {

// ---- direct convolution from a 3-channel tensor: backward-data of the CelebA output conv (1x1, 3 -> 128 channels) ----------------
// K = 3 is far too short for an MFMA K-loop; the call is bound by reading the activation-derivative gate and writing dx (1.07 GB
// each at B=128): the generic gather kernel ran it at 2.2 TB/s, this one at 4.6 TB/s.  One thread owns 4 output channels, holds
// their K x 4 filter taps in registers for the whole launch and walks output pixels grid-stride; the lanes of a pixel read the same
// input words (broadcast, L1-resident) and store one contiguous Cout*4-byte row.  Accumulation order = (kh, kw, ci).
// (A 3x3 / Cin=3 instantiation for enc.conv2d forward measured 176 us against 133 us for the MFMA gather kernel -- VALU-bound on
// its 27 broadcast loads + 108 FMAs per thread -- so the forward keeps the gather kernel.)
template <int KH_, int KW_, int CIN, bool GATE>
__global__ __launch_bounds__(256) void conv_smallcin_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                            const float* __restrict__ bias, float* __restrict__ y,
                                                            const float* __restrict__ gate, int H, int W, int Wo, int Cout,
                                                            int stride, int pad_t, int pad_l, int act, int M, FastDiv div_howo,
                                                            FastDiv div_wo, int HoWo) {
  constexpr int K = KH_ * KW_ * CIN;
  const int cq = Cout >> 2;                         // channel quads per pixel (power of two, 4..64)
  const int q = threadIdx.x & (cq - 1);
  const int ppb = 256 / cq;                         // pixels per block step
  const int pl = threadIdx.x / cq;
  float4 wr[K];
#pragma unroll
  for (int k = 0; k < K; ++k) wr[k] = *reinterpret_cast<const float4*>(w + (size_t)k * Cout + q * 4);
  float4 b4 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (bias != nullptr) b4 = *reinterpret_cast<const float4*>(bias + q * 4);
  for (int m = blockIdx.x * ppb + pl; m < M; m += gridDim.x * ppb) {
    const int n = (int)fdiv((uint32_t)m, div_howo);
    const int r = m - n * HoWo;
    const int oh = (int)fdiv((uint32_t)r, div_wo), ow = r - oh * Wo;
    const int ih0 = oh * stride - pad_t, iw0 = ow * stride - pad_l;
    const float* xn = x + (size_t)n * H * W * CIN;
    float4 acc = b4;
#pragma unroll
    for (int kh = 0; kh < KH_; ++kh) {
      const int ih = ih0 + kh;
      const bool okh = (unsigned)ih < (unsigned)H;
#pragma unroll
      for (int kw = 0; kw < KW_; ++kw) {
        const int iw = iw0 + kw;
        const bool ok = okh && (unsigned)iw < (unsigned)W;
        const float* px = xn + ((ok ? ih : 0) * W + (ok ? iw : 0)) * CIN;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) {
          const float v = ok ? px[ci] : 0.f;
          const float4 ww = wr[(kh * KW_ + kw) * CIN + ci];
          acc.x = fmaf(v, ww.x, acc.x);
          acc.y = fmaf(v, ww.y, acc.y);
          acc.z = fmaf(v, ww.z, acc.z);
          acc.w = fmaf(v, ww.w, acc.w);
        }
      }
    }
    const size_t o = (size_t)m * Cout + q * 4;
    if (GATE) {                                     // dx *= act'(y_prev) evaluated from the layer-below's OUTPUT
      const float4 g = *reinterpret_cast<const float4*>(gate + o);
      acc.x *= ladder_act_grad_from_out(g.x, act);
      acc.y *= ladder_act_grad_from_out(g.y, act);
      acc.z *= ladder_act_grad_from_out(g.z, act);
      acc.w *= ladder_act_grad_from_out(g.w, act);
    } else {
      acc.x = ladder_act_fn(acc.x, act);
      acc.y = ladder_act_fn(acc.y, act);
      acc.z = ladder_act_fn(acc.z, act);
      acc.w = ladder_act_fn(acc.w, act);
    }
    *reinterpret_cast<float4*>(y + o) = acc;
  }
}

}  // namespace

bool smallcin_eligible(int Cin, int Cout, int KH, int KW) {
  static const bool off = getenv("LADDER_DISABLE_SMALLCIN") != nullptr;
  const int cq = Cout >> 2;
  return !off && KH == 1 && KW == 1 && Cin == 3 && (Cout & 3) == 0 && cq >= 4 && cq <= 64 && (cq & (cq - 1)) == 0;
}

int launch_smallcin(const float* x, const float* w, const float* bias, float* y, const float* gate, int N, int H, int W, int Cin,
                    int Ho, int Wo, int Cout, int KH, int stride, int pad_t, int pad_l, int act, hipStream_t st) {
  if (!ladder_aligned16(w) || !ladder_aligned16(y) || (bias != nullptr && !ladder_aligned16(bias)) ||
      (gate != nullptr && !ladder_aligned16(gate)))
    return LADDER_E_ALIGN;
  const long Ml = (long)N * Ho * Wo;
  if (Ml >= (1L << 31)) return LADDER_E_SHAPE;
  const int M = (int)Ml, ppb = 256 / (Cout >> 2);
  long blocks = (Ml + ppb - 1) / ppb;
  if (blocks > 256L * 16) blocks = 256L * 16;        // two residency rounds of the chip, grid-stride beyond that
  const FastDiv dhw = make_fastdiv(Ho * Wo), dw = make_fastdiv(Wo);
#define LADDER_SMALLCIN(KH_, KW_, CIN_, G_)                                                                                      \
  hipLaunchKernelGGL((conv_smallcin_kernel<KH_, KW_, CIN_, G_>), dim3((unsigned)blocks), dim3(256), 0, st, x, w, bias, y, gate, H, W, \
                     Wo, Cout, stride, pad_t, pad_l, act, M, dhw, dw, Ho * Wo)
  if (KH != 1 || Cin != 3) return LADDER_E_SHAPE;
  if (gate != nullptr) LADDER_SMALLCIN(1, 1, 3, true); else LADDER_SMALLCIN(1, 1, 3, false);
#undef LADDER_SMALLCIN
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

namespace {

// ---- single-output-channel 5x5 VALID convolution: the MNIST decoders' output layer (codes/models.py:141-148, 308-315) -----------
// [B,32,32,Cin] -> [B,28,28,1] is a per-pixel dot product of length 25*Cin: as a GEMM it wastes 31/32 of an N tile (329 us forward,
// 381 us filter gradient at B = 256, Cin = 64 -- a fifth of the MNIST-fashion iteration).  Direct form: lane = input channel, a
// wavefront walks one output row (64/Cin rows when Cin < 64) left to right keeping the KH x KW input window in registers -- each
// step loads ONE new column (KH loads) instead of KH*KW -- and reduces over the channel lanes with shuffles.  The filter gradient
// uses the same sliding window with dy as the broadcast scalar and 25 accumulators per lane.
template <int KH_, int KW_, int CL, bool WGRAD>
__global__ __launch_bounds__(256) void conv_cout1_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, float* __restrict__ y,
                                                         const float* __restrict__ dy, float* __restrict__ part, int H, int W, int Ho,
                                                         int Wo, int act, int rows_total) {
  constexpr int RPW = 64 / CL, KT = KH_ * KW_;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ci = lane % CL, rg = lane / CL;
  float wr[KT], acc[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    wr[t] = WGRAD ? 0.f : w[t * CL + ci];
    acc[t] = 0.f;
  }
  const float b = (!WGRAD && bias != nullptr) ? bias[0] : 0.f;
  float bsum = 0.f;
  for (int rb = (blockIdx.x * 4 + wv) * RPW; rb < rows_total; rb += gridDim.x * 4 * RPW) {
    const int row = rb + rg;
    const bool valid = row < rows_total;
    const int rc = valid ? row : rows_total - 1;
    const int n = rc / Ho, oh = rc - n * Ho;
    const float* xr = x + ((size_t)n * H + oh) * W * CL + ci;         // input row oh (pad 0), column 0
    float win[KH_][KW_];
#pragma unroll
    for (int kh = 0; kh < KH_; ++kh)
#pragma unroll
      for (int kw = 0; kw < KW_ - 1; ++kw) win[kh][kw] = xr[((size_t)kh * W + kw) * CL];
    for (int ow0 = 0; ow0 < Wo; ow0 += KW_) {
#pragma unroll
      for (int p = 0; p < KW_; ++p) {
        const int ow = ow0 + p;
        if (ow < Wo) {                                                 // wave-uniform
#pragma unroll
          for (int kh = 0; kh < KH_; ++kh) win[kh][(p + KW_ - 1) % KW_] = xr[((size_t)kh * W + ow + KW_ - 1) * CL];
          if (WGRAD) {
            const float g = valid ? dy[(size_t)rc * Wo + ow] : 0.f;
#pragma unroll
            for (int kh = 0; kh < KH_; ++kh)
#pragma unroll
              for (int kw = 0; kw < KW_; ++kw) acc[kh * KW_ + kw] = fmaf(win[kh][(p + kw) % KW_], g, acc[kh * KW_ + kw]);
            bsum += g;
          } else {
            float s = 0.f;
#pragma unroll
            for (int kh = 0; kh < KH_; ++kh)
#pragma unroll
              for (int kw = 0; kw < KW_; ++kw) s = fmaf(win[kh][(p + kw) % KW_], wr[kh * KW_ + kw], s);
#pragma unroll
            for (int o = CL / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (ci == 0 && valid) y[(size_t)row * Wo + ow] = ladder_act_fn(s + b, act);
          }
        }
      }
    }
  }
  if (WGRAD) {
    // block partial [KT][CL] (+ bias): sum the 4 waves x RPW row groups in LDS in a fixed order
    __shared__ float red[4][64];
    float* out = part + (size_t)blockIdx.x * (KT * CL + 1);
    for (int t = 0; t <= KT; ++t) {
      red[wv][lane] = t < KT ? acc[t] : bsum;
      __syncthreads();
      if (threadIdx.x < CL) {
        float v = 0.f;
        for (int q = 0; q < 4; ++q)
          for (int g2 = 0; g2 < RPW; ++g2) v += red[q][g2 * CL + threadIdx.x];
        if (t < KT) out[t * CL + threadIdx.x] = v;
        else if (threadIdx.x == 0) out[KT * CL] = v;
      }
      __syncthreads();
    }
  }
}

}  // namespace

bool cout1_eligible(int Cin, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int H, int W, int Ho, int Wo) {
  static const bool off = getenv("LADDER_DISABLE_COUT1") != nullptr;
  return !off && Cout == 1 && KH == 5 && KW == 5 && stride == 1 && pad_t == 0 && pad_l == 0 && Ho == H - 4 && Wo == W - 4 &&
         (Cin == 16 || Cin == 32 || Cin == 64);
}
static int cout1_blocks(int rows, int Cin) {
  const int rpb = 4 * (64 / Cin);
  int b = (rows + rpb - 1) / rpb;
  return b > 1024 ? 1024 : b;
}
size_t cout1_wgrad_ws_bytes(int N, int Ho, int Cin) { return (size_t)cout1_blocks(N * Ho, Cin) * (25 * Cin + 1) * sizeof(float); }

namespace {

// ---- 1x1 convolution to <= 4 channels over a wide map: the CelebA output layer (codes/models.py:580-586) -----------------------
// [B,128,128,128] -> 3 channels is HBM-bound (1.07 GB in, 25 MB out).  Forward: 32 lanes share a pixel (lane = channel quad, one
// coalesced 512-byte row), each lane keeps its 4 x COUT filter taps in registers, partial dot products are combined with shuffles.
// Backward: ONE pass over x produces all three results -- dx = (dy . W^T) * act'(x) (x is the producing layer's output, so the
// activation-derivative gate costs no extra read), dW += x^T dy and db += dy -- where separate backward-data and filter-gradient
// kernels each streamed the 1.07 GB tensor (0.44 + 0.32 ms -> 0.45 ms).
template <int COUT, bool BWD>
__global__ __launch_bounds__(256) void conv1x1_smallcout_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ bias, float* __restrict__ y,
                                                                const float* __restrict__ dy, float* __restrict__ dx,
                                                                float* __restrict__ part, int Cin, int act, int M,
                                                                float* __restrict__ dxamax, int rows_per_sample) {
  float dmax = 0.f;                                 // max |dx| written by this thread (backward, optional absmax record)
  // per-sample record of dx (rows_per_sample > 0): gridDim.x = N * bps workgroups, the bps workgroups of a sample sweep ITS pixels
  // grid-stride (128 concurrent 64 KB stripes at batch 128; one contiguous run per workgroup measured 13 % slower), one commit each
  const bool ps_rec = BWD && dxamax != nullptr && rows_per_sample > 0;
  const int bps = ps_rec ? gridDim.x / (M / rows_per_sample) : 1;
  const int ps_n = ps_rec ? blockIdx.x / bps : 0, ps_bx = ps_rec ? blockIdx.x - ps_n * bps : 0;
  const int cq = Cin >> 2;                          // channel quads per pixel (power of two, 4..64)
  const int q = threadIdx.x & (cq - 1), pl = threadIdx.x / cq, ppb = 256 / cq;
  float4 wr[COUT];                                  // wr[o] = w[4q..4q+3][o]
#pragma unroll
  for (int o = 0; o < COUT; ++o)
    wr[o] = make_float4(w[(size_t)(4 * q + 0) * COUT + o], w[(size_t)(4 * q + 1) * COUT + o], w[(size_t)(4 * q + 2) * COUT + o],
                        w[(size_t)(4 * q + 3) * COUT + o]);
  float4 gw[COUT];
  float gb[COUT];
#pragma unroll
  for (int o = 0; o < COUT; ++o) {
    gw[o] = make_float4(0.f, 0.f, 0.f, 0.f);
    gb[o] = 0.f;
  }
  constexpr int U = 1;                              // (U = 4 pixels in flight per thread measured slower: 553 vs 443 us backward)
  const int per_round = (ps_rec ? bps : gridDim.x) * ppb;
  const int steps = ((ps_rec ? rows_per_sample : M) + per_round * U - 1) / (per_round * U);
  for (int it = 0; it < steps; ++it) {              // uniform trip count: the shuffles below need whole wavefronts
    int mm[U];
    float4 xu[U];

#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (ps_rec) {
        const int r = (it * bps + ps_bx) * ppb + pl;               // pixel inside the sample
        mm[u] = r < rows_per_sample ? ps_n * rows_per_sample + r : M;
      } else {
        mm[u] = ((it * U + u) * gridDim.x + blockIdx.x) * ppb + pl;
      }
      xu[u] = mm[u] < M ? *reinterpret_cast<const float4*>(x + (size_t)mm[u] * Cin + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int m = mm[u];
      const bool ok = m < M;
      const float4 xv = xu[u];
      if (!BWD) {
        float s[COUT];
#pragma unroll
        for (int o = 0; o < COUT; ++o) {
          s[o] = fmaf(xv.x, wr[o].x, fmaf(xv.y, wr[o].y, fmaf(xv.z, wr[o].z, xv.w * wr[o].w)));
          for (int d = cq >> 1; d > 0; d >>= 1) s[o] += __shfl_xor(s[o], d, 64);
        }
        if (q == 0 && ok) {
#pragma unroll
          for (int o = 0; o < COUT; ++o) y[(size_t)m * COUT + o] = ladder_act_fn(s[o] + (bias != nullptr ? bias[o] : 0.f), act);
        }
      } else {
        float g[COUT];
#pragma unroll
        for (int o = 0; o < COUT; ++o) g[o] = ok ? dy[(size_t)m * COUT + o] : 0.f;
        float4 d4 = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int o = 0; o < COUT; ++o) {
          d4.x = fmaf(g[o], wr[o].x, d4.x); d4.y = fmaf(g[o], wr[o].y, d4.y);
          d4.z = fmaf(g[o], wr[o].z, d4.z); d4.w = fmaf(g[o], wr[o].w, d4.w);
          gw[o].x = fmaf(xv.x, g[o], gw[o].x); gw[o].y = fmaf(xv.y, g[o], gw[o].y);
          gw[o].z = fmaf(xv.z, g[o], gw[o].z); gw[o].w = fmaf(xv.w, g[o], gw[o].w);
          gb[o] += g[o];
        }
        if (ok && dx != nullptr) {
          d4.x *= ladder_act_grad_from_out(xv.x, act); d4.y *= ladder_act_grad_from_out(xv.y, act);
          d4.z *= ladder_act_grad_from_out(xv.z, act); d4.w *= ladder_act_grad_from_out(xv.w, act);
          *reinterpret_cast<float4*>(dx + (size_t)m * Cin + q * 4) = d4;
          dmax = fmaxf(fmaxf(dmax, fmaxf(fabsf(d4.x), fabsf(d4.y))), fmaxf(fabsf(d4.z), fabsf(d4.w)));
        }
      }
    }
  }
  if (BWD) {
    // block partial: [Cin][COUT] filter gradient + [COUT] bias gradient, pixel lanes combined in LDS in a fixed order
    __shared__ float red[256];
    float* out = part + (size_t)blockIdx.x * ((size_t)Cin * COUT + COUT);
#pragma unroll
    for (int t = 0; t < 4 * COUT + COUT; ++t) {
      float v;
      if (t < 4 * COUT) {
        const float4 gv = gw[t >> 2];
        const int e = t & 3;
        v = e == 0 ? gv.x : (e == 1 ? gv.y : (e == 2 ? gv.z : gv.w));
      } else {
        v = (q == 0) ? gb[t - 4 * COUT] : 0.f;
      }
      red[threadIdx.x] = v;
      __syncthreads();
      if (pl == 0) {
        float a = 0.f;
        for (int r = 0; r < ppb; ++r) a += red[r * cq + q];
        if (t < 4 * COUT) out[(size_t)(4 * q + (t & 3)) * COUT + (t >> 2)] = a;
        else if (q == 0) out[(size_t)Cin * COUT + (t - 4 * COUT)] = a;
      }
      __syncthreads();
    }
    if (ps_rec) amax_commit_block_sample(dmax, dxamax, ps_n);
    else if (dxamax != nullptr) amax_commit_block(dmax, dxamax);
  }
}

// Block partials with trailing bias slots, ws[S][n+nb]: out[i] = sum_s ws[s][i] (i < n), bias_out[j] = sum_s ws[s][n+j].
// 16 threads per output, each summing every 16th partial, then a fixed-order LDS combine (as reduce_splits_wide_kernel).
__global__ __launch_bounds__(256) void reduce_partials_multi_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                                    float* __restrict__ bias_out, int S, int n, int nb) {
  __shared__ float part[16][17];
  const int o = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + o;
  float a = 0.f;
  if (i < n + nb)
    for (int z = g; z < S; z += 16) a += ws[(size_t)z * (n + nb) + i];
  part[g][o] = a;
  __syncthreads();
  if (g == 0 && i < n + nb) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += part[k][o];
    if (i < n) out[i] = t;
    else if (bias_out != nullptr) bias_out[i - n] = t;
  }
}

}  // namespace

bool smallcout_eligible(int Cin, int Cout, int KH, int KW, int stride, long M) {
  static const bool off = getenv("LADDER_DISABLE_SMALLCOUT") != nullptr;
  const int cq = Cin >> 2;
  return !off && KH == 1 && KW == 1 && stride == 1 && Cout >= 1 && Cout <= 4 && (Cin & 3) == 0 && cq >= 4 && cq <= 64 &&
         (cq & (cq - 1)) == 0 && M >= 65536 && M < (1L << 31);
}
int smallcout_blocks(long M, int Cin) {
  const long ppb = 256 / (Cin >> 2);
  long b = (M + ppb - 1) / ppb;
  return (int)(b > 2048 ? 2048 : b);
}

// ---- one launcher per kernel: a null dy selects the forward instantiation, dy the backward one -----------------------------------------
void launch_cout1(const float* x, const float* w, const float* bias, float* y, const float* dy, float* part, float* dw, float* db, int N,
                  int H, int W, int Cin, int Ho, int Wo, int act, hipStream_t st) {
  const int rows = N * Ho, blocks = cout1_blocks(rows, Cin), kn = 25 * Cin;
#define LADDER_COUT1(CL_, WG_) \
  hipLaunchKernelGGL((conv_cout1_kernel<5, 5, CL_, WG_>), dim3(blocks), dim3(256), 0, st, x, w, bias, y, dy, part, H, W, Ho, Wo, act, rows)
#define LADDER_COUT1_CIN(WG_) \
  do { if (Cin == 64) LADDER_COUT1(64, WG_); else if (Cin == 32) LADDER_COUT1(32, WG_); else LADDER_COUT1(16, WG_); } while (0)
  if (dy == nullptr) { LADDER_COUT1_CIN(false); return; }
  LADDER_COUT1_CIN(true);
#undef LADDER_COUT1_CIN
#undef LADDER_COUT1
  hipLaunchKernelGGL(reduce_partials_multi_kernel, dim3((kn + 1 + 15) / 16), dim3(256), 0, st, (const float*)part, dw, db, blocks, kn, 1);
}

void launch_smallcout(const float* x, const float* w, const float* bias, float* y, const float* dy, float* dx, float* part, int Cin, int Cout,
                      int act, int M, float* dxamax, int rows_per_sample, int blocks, hipStream_t st) {
#define LADDER_SCO(CO_, BWD_) \
  hipLaunchKernelGGL((conv1x1_smallcout_kernel<CO_, BWD_>), dim3(blocks), dim3(256), 0, st, x, w, bias, y, dy, dx, part, Cin, act, M, dxamax, rows_per_sample)
#define LADDER_SCO_COUT(BWD_) \
  switch (Cout) { case 1: LADDER_SCO(1, BWD_); break; case 2: LADDER_SCO(2, BWD_); break; case 3: LADDER_SCO(3, BWD_); break; default: LADDER_SCO(4, BWD_); }
  if (dy != nullptr) { LADDER_SCO_COUT(true) } else { LADDER_SCO_COUT(false) }
#undef LADDER_SCO_COUT
#undef LADDER_SCO
}

extern "C" {

int ladder_conv1x1_smallcout_eligible(long M, int Cin, int Cout) { return smallcout_eligible(Cin, Cout, 1, 1, 1, M) ? 1 : 0; }

size_t ladder_conv1x1_smallcout_bwd_workspace_bytes(long M, int Cin, int Cout) {
  return (size_t)smallcout_blocks(M, Cin) * ((size_t)Cin * Cout + Cout) * sizeof(float);
}

int ladder_conv1x1_smallcout_bwd(const float* x, const float* dy, const float* w, float* dx, float* dw, float* db, long M, int Cin,
                                 int Cout, int gate_act, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  return ladder_conv1x1_smallcout_bwd_absmax(x, dy, w, dx, dw, db, M, Cin, Cout, gate_act, ws, ws_bytes, nullptr, 0, stream);
}

int ladder_conv1x1_smallcout_bwd_absmax(const float* x, const float* dy, const float* w, float* dx, float* dw, float* db, long M, int Cin,
                                        int Cout, int gate_act, void* ws, size_t ws_bytes, float* dx_absmax, long rows_per_sample,
                                        ladder_stream_t stream) {
  if (!smallcout_eligible(Cin, Cout, 1, 1, 1, M)) return LADDER_E_SHAPE;
  int rps = (rows_per_sample > 0 && rows_per_sample < (1L << 30) && (M % rows_per_sample) == 0) ? (int)rows_per_sample : 0;
  if (dx_absmax != nullptr && (dx == nullptr || hipMemsetAsync(dx_absmax, 0, LADDER_ABSMAX_FLOATS * sizeof(float), stream) != hipSuccess))
    return LADDER_E_SHAPE;
  if (!ladder_aligned16(x) || (dx != nullptr && !ladder_aligned16(dx))) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_conv1x1_smallcout_bwd_workspace_bytes(M, Cin, Cout)) return LADDER_E_WORKSPACE;
  int blocks = smallcout_blocks(M, Cin);
  const int kn = Cin * Cout;
  if (rps > 0) {                                              // per-sample record: N * bps workgroups (<= the partial-sum slots of the workspace)
    const long nsmp = M / rps, ppb = 256 / (Cin >> 2);
    long bps = blocks / nsmp;
    if (bps > (rps + ppb - 1) / ppb) bps = (rps + ppb - 1) / ppb;
    if (nsmp > blocks || bps < 1) rps = 0; else blocks = (int)(nsmp * bps);
  }
  float* part = (float*)ws;
  launch_smallcout(x, w, nullptr, nullptr, dy, dx, part, Cin, Cout, gate_act, (int)M, dx_absmax, rps, blocks, stream);
  // partial layout per block: [Cin*Cout filter gradient | Cout bias gradient]
  hipLaunchKernelGGL(reduce_partials_multi_kernel, dim3((kn + Cout + 15) / 16), dim3(256), 0, stream, (const float*)part, dw, db, blocks, kn, Cout);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
