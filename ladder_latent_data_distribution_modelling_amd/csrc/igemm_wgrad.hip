// Filter / weight gradients of the strict-fp32 convolution and dense layers (the forward family is igemm.hip):
//   igemm_wgrad_kernel<...> dW[K x N] = A_gather^T[K x M] * dY[M x N], split over M with a fixed-order second-stage reduction
//                           (bit-reproducible), bias gradient fused.
//   wgrad3x3_halo_kernel    filter gradient of the 3x3 layers (Cin % 64 == 0), all 9 taps fused over LDS-DMA-staged 1x32-pixel patches,
//                           12 balanced wavefronts x 6 MFMA tiles (~120 TF; ablation: 126 without staging, 133 without the
//                           per-patch barrier as well).
//   reduce_splits_*         the fixed-order second stage every split filter gradient of the project ends in (WgradTail, igemm.h).
#include "igemm.h"

namespace {

// dW[K x N] (+= over pixel split) = A_gather^T * dY.  GEMM-M here is the filter index k' = (r,s,ci).
#ifndef IGEMM_WG_MINW
#define IGEMM_WG_MINW 3
#endif
template <int BM, int BN, int WM, int WN, bool VECA, bool VECB>
__global__ __launch_bounds__(kThreads, (BM * BN >= 128 * 128) ? IGEMM_WG_MINW : 1) void igemm_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                               float* __restrict__ out, float* __restrict__ bias_part,
                                                               const IgemmDesc d, const int tiles_n, const int m_per_split) {
  constexpr int TM = BM / WM, TN = BN / WN, MI = TM / 32, NI = TN / 32;
  constexpr int A_UNITS = BK * (BM / 4), B_UNITS = BK * (BN / 4);
  constexpr int AU = (A_UNITS + kThreads - 1) / kThreads, BU = (B_UNITS + kThreads - 1) / kThreads;
  __shared__ __attribute__((aligned(16))) float At[2][BK * BM];
  __shared__ __attribute__((aligned(16))) float Bt[2][BK * BN];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int wm = wid / WN, wn = wid % WN;
  const int tile = blockIdx.x;
  const int k0t = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
  const int HoWo = d.Ho * d.Wo;
  const int p_begin = blockIdx.y * m_per_split;
  const int p_end = min(d.M, p_begin + m_per_split);

  // per-thread filter coordinates (fixed) for the A tile
  int a_pr[AU], a_kq[AU], a_r[AU][VECA ? 1 : 4], a_s[AU][VECA ? 1 : 4], a_ci[AU][VECA ? 1 : 4];
  bool a_kok[AU][VECA ? 1 : 4];
#pragma unroll
  for (int i = 0; i < AU; ++i) {
    const int u = tid + i * kThreads;
    a_pr[i] = u / (BM / 4);
    a_kq[i] = u % (BM / 4);
#pragma unroll
    for (int j = 0; j < (VECA ? 1 : 4); ++j) {
      const int k = k0t + a_kq[i] * 4 + j;
      a_kok[i][j] = (u < A_UNITS) && k < d.K;
      const int kk = a_kok[i][j] ? k : 0;
      const int rs = kk / d.Cin;
      a_ci[i][j] = kk - rs * d.Cin;
      a_r[i][j] = rs / d.KW;
      a_s[i][j] = rs - a_r[i][j] * d.KW;
    }
  }
  int b_pr[BU], b_nq[BU];
#pragma unroll
  for (int i = 0; i < BU; ++i) {
    const int u = tid + i * kThreads;
    b_pr[i] = u / (BN / 4);
    b_nq[i] = u % (BN / 4);
  }

  // bias gradient (column sums of dY) rides along in the k'-tile-0 workgroups: they already stream every dY row
  const bool do_bias = (bias_part != nullptr) && (tile / tiles_n == 0);
  float4 bsum[BU];
#pragma unroll
  for (int i = 0; i < BU; ++i) bsum[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 ra[AU], rb[BU];
  auto load_chunk = [&](int c) {
    const int pc = p_begin + c * BK;
#pragma unroll
    for (int i = 0; i < AU; ++i) {
      const int p = pc + a_pr[i];
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (p < p_end) {
        const uint32_t n_img = fdiv((uint32_t)p, d.div_howo), rem = (uint32_t)p - n_img * HoWo;
        const int ho = (int)fdiv(rem, d.div_wo), wo = (int)rem - ho * d.Wo;
        const long img = (long)n_img * d.H * d.W * d.Cin;
        const int bh = ho * d.stride - d.pad_t, bw = wo * d.stride - d.pad_l;
        if (VECA) {
          const long off = a_kok[i][0] ? gather_off(d, img, bh, bw, a_r[i][0], a_s[i][0], a_ci[i][0]) : -1;
          const float4 t = ld4(off >= 0 ? x + off : g_zero16);
          v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (a_kok[i][VECA ? 0 : j]) {
              const long off = gather_off(d, img, bh, bw, a_r[i][VECA ? 0 : j], a_s[i][VECA ? 0 : j], a_ci[i][VECA ? 0 : j]);
              if (off >= 0) v[j] = x[off];
            }
          }
        }
      }
      ra[i] = make_float4(v[0], v[1], v[2], v[3]);
    }
#pragma unroll
    for (int i = 0; i < BU; ++i) {
      const int p = pc + b_pr[i], n = n0 + b_nq[i] * 4;
      const bool inb = (tid + i * kThreads < B_UNITS) && p < p_end;
      if (VECB) {
        rb[i] = ld4((inb && n < d.Cout) ? dy + (long)p * d.Cout + n : g_zero16);
      } else {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (inb && n + j < d.Cout) ? dy[(long)p * d.Cout + n + j] : 0.f;
        rb[i] = make_float4(v[0], v[1], v[2], v[3]);
      }
      if (do_bias) {
        bsum[i].x += rb[i].x; bsum[i].y += rb[i].y; bsum[i].z += rb[i].z; bsum[i].w += rb[i].w;
      }
    }
  };
  auto store_chunk = [&](int buf) {
#pragma unroll
    for (int i = 0; i < AU; ++i)
      if (tid + i * kThreads < A_UNITS) *reinterpret_cast<float4*>(&At[buf][a_pr[i] * BM + a_kq[i] * 4]) = ra[i];
#pragma unroll
    for (int i = 0; i < BU; ++i)
      if (tid + i * kThreads < B_UNITS) *reinterpret_cast<float4*>(&Bt[buf][b_pr[i] * BN + b_nq[i] * 4]) = rb[i];
  };

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  const int nchunks = (p_end - p_begin + BK - 1) / BK;
  if (nchunks > 0) {
    load_chunk(0);
    store_chunk(0);
  }
  __syncthreads();
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) load_chunk(c + 1);
    const float* Ab = &At[buf][lh * BM + wm * TM + l31];
    const float* Bb = &Bt[buf][lh * BN + wn * TN + l31];
#pragma unroll
    for (int kk = 0; kk < BK; kk += 2) {
      float a[MI], b[NI];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) a[mi] = Ab[kk * BM + mi * 32];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) b[ni] = Bb[kk * BN + ni * 32];
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
    }
    if (c + 1 < nchunks) store_chunk(buf ^ 1);
    __syncthreads();
  }

  float* o = out + (size_t)blockIdx.y * d.K * d.Cout;
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int n = n0 + wn * TN + ni * 32 + l31;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k = k0t + wm * TM + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (k < d.K && n < d.Cout) o[(long)k * d.Cout + n] = acc[mi][ni][e];
      }
    }
  }
  if (do_bias) {   // fixed-order reduction of the per-thread column sums through LDS (all MFMA reads of Bt are done)
    __syncthreads();
#pragma unroll
    for (int i = 0; i < BU; ++i)
      if (tid + i * kThreads < B_UNITS) *reinterpret_cast<float4*>(&Bt[0][b_pr[i] * BN + b_nq[i] * 4]) = bsum[i];
    __syncthreads();
    if (tid < BN && n0 + tid < d.Cout) {
      float sacc = 0.f;
#pragma unroll
      for (int r = 0; r < BK; ++r) sacc += Bt[0][r * BN + tid];
      bias_part[(size_t)blockIdx.y * d.Cout + n0 + tid] = sacc;
    }
  }
}

__global__ void reduce_splits_kernel(const float* __restrict__ ws, float* __restrict__ out, int S, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
  for (int z = 0; z < S; ++z) s += ws[(size_t)z * n + i];  // fixed order
  out[i] = s;
}

// Many partials of a SHORT vector (filter gradients of the image-side convs: up to 1024 splits of a few thousand floats, and every
// fused bias gradient): 16 threads share one output, each summing every 16th partial, then a fixed-order LDS tree.  The serial
// version above needs `S` dependent loads per thread with only n threads in flight (235 us for enc.conv2d's 768 x 3456 partials).
__global__ __launch_bounds__(256) void reduce_splits_wide_kernel(const float* __restrict__ ws, float* __restrict__ out, int S, size_t n) {
  __shared__ float part[16][17];
  const int o = threadIdx.x & 15, g = threadIdx.x >> 4;
  const size_t i = (size_t)blockIdx.x * 16 + o;
  float s = 0.f;
  if (i < n)
    for (int z = g; z < S; z += 16) s += ws[(size_t)z * n + i];
  part[g][o] = s;
  __syncthreads();
  if (g == 0 && i < n) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += part[k][o];   // fixed order
    out[i] = t;
  }
}

}  // namespace

void launch_reduce_splits(const float* ws, float* out, int S, size_t n, hipStream_t st) {
  if (S >= 32 && n * 16 <= ((size_t)1 << 24))
    hipLaunchKernelGGL(reduce_splits_wide_kernel, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, st, ws, out, S, n);
  else
    hipLaunchKernelGGL(reduce_splits_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, ws, out, S, n);
}

// ---- wgrad planning (shared by the workspace query and the launcher)
WgradPlan plan_wgrad(long M, int K, int Cout) {
  WgradPlan p;
  p.bn = Cout > 64 ? 128 : (Cout > 32 ? 64 : 32);
  p.bm = (K > 64 || p.bn != 64) ? 128 : 64;
  if (p.bn == 128 && K <= 64) { p.bm = 64; p.bn = 64; }
  p.tiles_k = (K + p.bm - 1) / p.bm;
  p.tiles_n = (Cout + p.bn - 1) / p.bn;
  const long tiles = (long)p.tiles_k * p.tiles_n;
  // fill whole rounds of the chip: 256 CUs x 3 resident workgroups; two rounds when the reduction is long enough
  const long slots = 256 * 3;
  long s = (2 * slots) / tiles;
  const long max_s = (M + 255) / 256;              // at least 256 pixels (16 chunks) per split
  if (s > max_s) s = max_s;
  if (s * tiles > slots && s * tiles < 2 * slots) s = slots / tiles;   // avoid a partially filled second round
  // the partial sums are written and re-read once: keep them <= ~48 MB (one round of the chip is enough for wide filters)
  if (s * tiles > slots && (size_t)s * K * Cout * sizeof(float) > ((size_t)48 << 20)) s = slots / tiles > 0 ? slots / tiles : 1;
  if (s < 1) s = 1;
  if (s > 1024) s = 1024;
  long mps = (M + s - 1) / s;
  mps = (mps + BK - 1) / BK * BK;
  p.m_per_split = (int)mps;
  p.splits = (int)((M + mps - 1) / mps);
  return p;
}

template <int BM, int BN, int WM, int WN>
static int launch_wgrad(const float* x, const float* dy, float* out, float* bias_part, const IgemmDesc& d, const WgradPlan& p, hipStream_t st) {
  const bool veca = (d.Cin % 4) == 0, vecb = (d.Cout % 4) == 0;
  dim3 grid(p.tiles_k * p.tiles_n, p.splits), block(kThreads);
  if (veca && vecb) hipLaunchKernelGGL((igemm_wgrad_kernel<BM, BN, WM, WN, true, true>), grid, block, 0, st, x, dy, out, bias_part, d, p.tiles_n, p.m_per_split);
  else if (veca) hipLaunchKernelGGL((igemm_wgrad_kernel<BM, BN, WM, WN, true, false>), grid, block, 0, st, x, dy, out, bias_part, d, p.tiles_n, p.m_per_split);
  else if (vecb) hipLaunchKernelGGL((igemm_wgrad_kernel<BM, BN, WM, WN, false, true>), grid, block, 0, st, x, dy, out, bias_part, d, p.tiles_n, p.m_per_split);
  else hipLaunchKernelGGL((igemm_wgrad_kernel<BM, BN, WM, WN, false, false>), grid, block, 0, st, x, dy, out, bias_part, d, p.tiles_n, p.m_per_split);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

// ---------------------------------------------------------------------------------------------------------------
namespace {

// Filter gradient of a 3x3 / stride 1 / SAME convolution with an LDS-staged input halo patch (tap-fused).
// One workgroup = 12 wavefronts (a balanced 3 per SIMD) owns a (64 input channels x 128 output channels) slab of dW for all 9
// taps = 72 MFMA tiles of 32x32, reduced over a range of 1x32-pixel patches.  Wavefront -> (filter row r, input-channel half cb,
// output-channel pair njp); its 6 tiles are the taps (r, 0..2) x the 2 channel blocks of the pair: per 2-pixel k-step it reads
// 3 halo fragments (one per column shift) and 2 dY fragments and issues 6 MFMAs -- 0.83 LDS reads per MFMA (the first version
// of this kernel: 2.0, 111 TF/s; shared-dY assignment: 1.33, 119 TF/s).  Per patch the 3x(32+2) input halo (64 channels, 26 KB)
// and the 32x128 dY tile (16 KB) are brought into LDS ONCE by LDS-DMA (global_load_lds, no staging registers) and serve all 9
// taps; the generic kernel streams both operands once per tap.  A fragment = halo shifted by (r,s), lane = ci; B = dY rows.
// Patch shapes (round 4): 1 x 32 pixels for maps at least 32 wide; 2 x 16 and 4 x 8 for the 16 x 16 and 8 x 8 decoder maps (the halo of a
// squarer patch is smaller: 72 / 60 halo pixels per 32 against 102) -- the generic kernel streamed both operands once per tap there
// (~88 TF against ~125 TF here).  The pixel index of a k-step maps to (row, column) of the patch at compile time (PW is a power of two).
constexpr int WH_CI = 64, WH_CO = 128, WH_PIX = 32;
constexpr int WH_THREADS = 768;
// Stride 2 (S = 2; SAME padding of an even map = one zero line below / right, none above / left): the input footprint of a patch is
// (2 PH + 1) x (2 PW + 1) pixels, tap (r, s) of output pixel (i, j) reads footprint pixel (2 i + r, 2 j + s) -- the same kernel with a
// pixel stride of 2 in the fragment addresses (encoder conv2d_1 ... 3: 522 / 251 / 138 us on the generic kernel at batch 128).
template <int PH, int PW, int S> struct WhGeom {
  static constexpr int HW = S * PW + 3 - S, HH = S * PH + 3 - S;
  static constexpr int XU = HH * HW * (WH_CI / 4), DU = WH_PIX * (WH_CO / 4);             // float4 units per patch
  static constexpr int XN = (XU + WH_THREADS - 1) / WH_THREADS, DN = (DU + WH_THREADS - 1) / WH_THREADS;   // 3 (2 for the small patches; 5 / 4 / 4 at stride 2), 2
  static constexpr int XF = HH * HW * WH_CI, DF = WH_PIX * WH_CO;                          // floats per buffer
};
#ifndef IGEMM_WH_MINW
#define IGEMM_WH_MINW 3
#endif
template <int PH, int PW, int S>
__global__ __launch_bounds__(WH_THREADS, IGEMM_WH_MINW) void wgrad3x3_halo_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                  float* __restrict__ out, float* __restrict__ bias_part,
                                                                  const int N, const int H, const int W, const int Cin,
                                                                  const int Cout, const int tiles_co, const int patches_per_split) {
  // H, W: the OUTPUT map (= the input map at stride 1; the input map is S H x S W)
  using G = WhGeom<PH, PW, S>;
  static_assert(PH * PW == WH_PIX && (PW & (PW - 1)) == 0 && (PW % 2) == 0, "32-pixel patches, rows of a power of two");
  constexpr int WH_HW = G::HW, WH_XF = G::XF, WH_DF = G::DF;
  // ONE LDS object (hipcc serialises LDS-DMA against ds_reads when several __shared__ objects exist): [buf][halo | dY]
  __shared__ __attribute__((aligned(16))) float lds[2 * (WH_XF + WH_DF)];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wv = tid >> 6;            // 12 wavefronts
  const int l31 = lane & 31, lh = lane >> 5;
  const int ci0 = (blockIdx.x / tiles_co) * WH_CI, co0 = (blockIdx.x % tiles_co) * WH_CO;
  const int WP = W / PW, HP = H / PH;
  const int q_total = N * HP * WP;
  const int q0 = blockIdx.y * patches_per_split, q1 = min(q_total, q0 + patches_per_split);
  const int r = wv >> 2, cb = (wv >> 1) & 1, njp = wv & 1;
  const int a_off = (r * WH_HW + S * lh) * WH_CI + cb * 32 + l31;      // + s * WH_CI for the column shift s
  const int b_off = WH_XF + lh * WH_CO + njp * 64 + l31;               // + j * 32 for the second block of the pair
  // bias: the centre-tap tiles (r = 1, s = 1) of the cb = 0 wavefronts cover every output channel exactly once.
  const bool do_bias = (bias_part != nullptr) && (ci0 == 0) && r == 1 && cb == 0;

  f32x16 acc[6];                                       // [j][s]
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
  float bsum[2] = {0.f, 0.f};

  auto stage_patch = [&](int q, int buf) {
    const int n = q / (HP * WP), rem = q - n * (HP * WP);
    const int hp = rem / WP, h0 = hp * PH, w0 = (rem - hp * WP) * PW;
    float* xb = &lds[buf * (WH_XF + WH_DF)];
    float* db = xb + WH_XF;
#pragma unroll
    for (int i = 0; i < G::XN; ++i) {
      const int u = tid + i * WH_THREADS;
      if (u < G::XU) {
        const int pix = u >> 4, q4 = u & 15;
        const int hr = pix / WH_HW, hc = pix - hr * WH_HW;
        const int hi = S * h0 - (2 - S) + hr, wi = S * w0 - (2 - S) + hc;
        const bool ok = hi >= 0 && hi < S * H && wi >= 0 && wi < S * W;
        const float* src = ok ? x + (((long)n * (S * H) + hi) * (S * W) + wi) * Cin + ci0 + q4 * 4 : g_zero16;
        __builtin_amdgcn_global_load_lds(src, xb + u * 4, 16, 0, 0);
      }
    }
#pragma unroll
    for (int i = 0; i < G::DN; ++i) {
      const int u = tid + i * WH_THREADS;
      if (u < G::DU) {
        const int p = u >> 5, q4 = u & 31;
        const bool ok = (co0 + q4 * 4) < Cout;
        const float* src = ok ? dy + (((long)n * H + h0 + p / PW) * W + w0 + (p & (PW - 1))) * Cout + co0 + q4 * 4 : g_zero16;
        __builtin_amdgcn_global_load_lds(src, db + u * 4, 16, 0, 0);
      }
    }
  };

  if (q0 < q1) stage_patch(q0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  for (int q = q0; q < q1; ++q) {
    const int buf = (q - q0) & 1;
    if (q + 1 < q1) stage_patch(q + 1, buf ^ 1);
    const float* base = &lds[buf * (WH_XF + WH_DF)];
#pragma unroll 4
    for (int ks = 0; ks < WH_PIX / 2; ++ks) {
      float a[3], b[2];
      const int arow = S * (((2 * ks) / PW) * WH_HW + ((2 * ks) & (PW - 1))) * WH_CI;     // pixel 2ks(+lh) of the patch -> halo row/col
#pragma unroll
      for (int s = 0; s < 3; ++s) a[s] = base[a_off + s * WH_CI + arow];
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = base[b_off + j * 32 + 2 * ks * WH_CO];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int s = 0; s < 3; ++s) acc[j * 3 + s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[j], acc[j * 3 + s], 0, 0, 0);
      if (do_bias) {
        bsum[0] += b[0];
        bsum[1] += b[1];
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wavefront's LDS-DMA pieces of the next patch have landed
    __syncthreads();
  }

#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int n = co0 + njp * 64 + j * 32 + l31;
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      float* o = out + ((size_t)blockIdx.y * 9 + (3 * r + s)) * Cin * Cout;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int ci = ci0 + cb * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (n < Cout) o[(size_t)ci * Cout + n] = acc[j * 3 + s][e];
      }
    }
    if (do_bias) {
      const float v = bsum[j] + __shfl_down(bsum[j], 32, 64);   // odd + even pixels of the k-step pairs
      if (lh == 0 && n < Cout) bias_part[(size_t)blockIdx.y * Cout + n] = v;
    }
  }
}

}  // namespace

WgradHaloPlan plan_wgrad_halo(const IgemmDesc& d) {
  WgradHaloPlan p{false, 0, 0, 1, 0, 0, 1};
  if (halo_disabled()) return p;
#if IGEMM_HALO
  static const int small_env = getenv("LADDER_WGRAD_SMALL_PATCHES") ? atoi(getenv("LADDER_WGRAD_SMALL_PATCHES")) : 1;   // (test switch)
  const int pw = (d.Wo % 32) == 0 ? 32 : (small_env && d.Wo == 16 && (d.Ho % 2) == 0) ? 16 : (small_env && d.Wo == 8 && (d.Ho % 4) == 0) ? 8 : 0;
  const bool s1 = d.stride == 1 && d.pad_t == 1 && d.pad_l == 1 && d.Ho == d.H && d.Wo == d.W;
  const bool s2 = small_env && d.stride == 2 && d.pad_t == 0 && d.pad_l == 0 && d.H == 2 * d.Ho && d.W == 2 * d.Wo;
  if (!(d.KH == 3 && d.KW == 3 && (s1 || s2) && d.ups == 1 && (d.Cin % WH_CI) == 0 && (d.Cout % 4) == 0 && d.Cout >= 64 && pw != 0))
    return p;
  p.stride = s2 ? 2 : 1;
  const long q_total = (long)d.N * d.Ho * d.Wo / WH_PIX;
  if (pw == 32 && s1 ? q_total < 4096 : q_total * (d.Cin / WH_CI) * ((d.Cout + WH_CO - 1) / WH_CO) < 4096) return p;   // small launches stay on the generic kernel
  p.pw = pw;
  p.tiles_ci = d.Cin / WH_CI;
  p.tiles_co = (d.Cout + WH_CO - 1) / WH_CO;
  const long pairs = (long)p.tiles_ci * p.tiles_co;
  long s = ((pw < 32 || s2 ? 1 : IGEMM_WH_BLOCKS) * 256L) / pairs;   // whole rounds of the chip (small maps: one -- 690 / 718 / 765 / 792 us for 1 ... 4 rounds on 16x16 512 -> 256 at batch 128: the partial tiles cost more than the tail)
  if (s > q_total / 16) s = q_total / 16;
  if (s < 1) s = 1;
  p.pps = (int)((q_total + s - 1) / s);
  p.splits = (int)((q_total + p.pps - 1) / p.pps);
  p.ok = true;
#endif
  return p;
}

static size_t wgrad_ws_bytes(long M, int K, int Cout) {
  const WgradPlan p = plan_wgrad(M, K, Cout);
  const size_t a = p.splits > 1 ? (size_t)p.splits * K * Cout * sizeof(float) : 0;
  return a + (size_t)p.splits * Cout * sizeof(float);   // + per-split bias partials
}

static size_t wgrad_ws_bytes_desc(const IgemmDesc& d) {
  const WgradHaloPlan hp = plan_wgrad_halo(d);
  size_t need = wgrad_ws_bytes(d.M, d.K, d.Cout);
  if (hp.ok) {
    const size_t h = ((hp.splits > 1 ? (size_t)hp.splits * d.K * d.Cout : 0) + (size_t)hp.splits * d.Cout) * sizeof(float);
    if (h > need) need = h;
  }
  return need;
}

static int run_wgrad(const float* x, const float* dy, float* dw, float* db, const IgemmDesc& d, void* ws, size_t ws_bytes, hipStream_t st) {
  if (d.M <= 0 || d.K <= 0 || d.Cout <= 0) return LADDER_E_SHAPE;
  if (!ladder_aligned16(x) || !ladder_aligned16(dy) || !ladder_aligned16(dw)) return LADDER_E_ALIGN;
  if (ws_bytes < wgrad_ws_bytes_desc(d) || ws == nullptr) return LADDER_E_WORKSPACE;
  const WgradHaloPlan hp = plan_wgrad_halo(d);
  if (hp.ok) {
    const WgradTail t = wgrad_tail(ws, hp.splits, (size_t)d.K * d.Cout, d.Cout, dw, db, true);
    const dim3 grid(hp.tiles_ci * hp.tiles_co, hp.splits), block(WH_THREADS);
#define LADDER_WH_LAUNCH(PH_, PW_, S_) \
  hipLaunchKernelGGL((wgrad3x3_halo_kernel<PH_, PW_, S_>), grid, block, 0, st, x, dy, t.part, t.bias_part, d.N, d.Ho, d.Wo, d.Cin, d.Cout, hp.tiles_co, hp.pps)
    if (hp.stride == 1) {
      if (hp.pw == 32) LADDER_WH_LAUNCH(1, 32, 1); else if (hp.pw == 16) LADDER_WH_LAUNCH(2, 16, 1); else LADDER_WH_LAUNCH(4, 8, 1);
    } else {
      if (hp.pw == 32) LADDER_WH_LAUNCH(1, 32, 2); else if (hp.pw == 16) LADDER_WH_LAUNCH(2, 16, 2); else LADDER_WH_LAUNCH(4, 8, 2);
    }
#undef LADDER_WH_LAUNCH
    return t.reduce(st);
  }
  const WgradPlan p = plan_wgrad(d.M, d.K, d.Cout);
  const WgradTail t = wgrad_tail(ws, p.splits, (size_t)d.K * d.Cout, d.Cout, dw, db, true);
  int rc;
  if (p.bm == 128 && p.bn == 128) rc = launch_wgrad<128, 128, 2, 2>(x, dy, t.part, t.bias_part, d, p, st);
  else if (p.bm == 128 && p.bn == 64) rc = launch_wgrad<128, 64, 4, 1>(x, dy, t.part, t.bias_part, d, p, st);
  else if (p.bm == 128 && p.bn == 32) rc = launch_wgrad<128, 32, 4, 1>(x, dy, t.part, t.bias_part, d, p, st);
  else rc = launch_wgrad<64, 64, 2, 2>(x, dy, t.part, t.bias_part, d, p, st);
  if (rc != LADDER_OK) return rc;
  return t.reduce(st);
}

extern "C" {

int ladder_reduce_splits(const float* ws, float* out, int splits, size_t n, ladder_stream_t stream) {
  if (splits <= 0 || n == 0) return LADDER_E_SHAPE;
  launch_reduce_splits(ws, out, splits, n, stream);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

size_t ladder_conv2d_bwd_filter_workspace_bytes(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW) {
  // upper bound over the stride/pad variants of this geometry (the halo path needs stride 1 / pad 1 / Ho==H, or stride 2 / pad 0 / H==2Ho)
  size_t need = wgrad_ws_bytes_desc(conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, 1, 1, 1, 1, 0));
  if (H == 2 * Ho && W == 2 * Wo) {
    const size_t n2 = wgrad_ws_bytes_desc(conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, 2, 1, 0, 0, 0));
    if (n2 > need) need = n2;
  }
  if (cout1_eligible(Cin, Cout, KH, KW, 1, 0, 0, H, W, Ho, Wo) && cout1_wgrad_ws_bytes(N, Ho, Cin) > need) need = cout1_wgrad_ws_bytes(N, Ho, Cin);
  return need;
}

int ladder_conv2d_bwd_filter_kernel_id(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t,
                                       int pad_l) {
  // 9128 = wgrad3x3_halo_kernel (tap-fused, LDS-DMA staged); 0 = any other filter-gradient path
  return plan_wgrad_halo(conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, 1, pad_t, pad_l, 0)).ok ? 9128 : 0;
}

int ladder_conv2d_bwd_filter(const float* x, const float* dy, float* dw, float* db, int N, int H, int W, int Cin, int Ho,
                             int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, void* ws, size_t ws_bytes,
                             ladder_stream_t stream) {
  if (!conv_shape_ok(N, H, W, Cin, Ho, Wo, KH, KW, stride)) return LADDER_E_SHAPE;
  if (cout1_eligible(Cin, Cout, KH, KW, stride, pad_t, pad_l, H, W, Ho, Wo)) {
    if (ws == nullptr || ws_bytes < cout1_wgrad_ws_bytes(N, Ho, Cin)) return LADDER_E_WORKSPACE;
    launch_cout1(x, nullptr, nullptr, nullptr, dy, (float*)ws, dw, db, N, H, W, Cin, Ho, Wo, 0, stream);
    LADDER_CHECK_LAUNCH();
    return LADDER_OK;
  }
  return run_wgrad(x, dy, dw, db, conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, 1, pad_t, pad_l, LADDER_ACT_NONE), ws, ws_bytes, stream);
}

size_t ladder_dense_bwd_weight_workspace_bytes(int M, int K, int N) {
  const size_t a = wgrad_ws_bytes(M, K, N), b = dense_wgrad_f32_ok(M, K, N) ? dense_wgrad_f32_ws_bytes(M, K, N) : 0;
  return a > b ? a : b;
}

int ladder_dense_bwd_weight(const float* x, const float* dy, float* dw, float* db, int M, int K, int N, void* ws,
                            size_t ws_bytes, ladder_stream_t stream) {
  if (dense_wgrad_f32_ok(M, K, N)) {                             // (csrc/densef32.hip: the filter gradients of the projected decoder pairs)
    if (ws == nullptr || ws_bytes < dense_wgrad_f32_ws_bytes(M, K, N)) return LADDER_E_WORKSPACE;
    if (!ladder_aligned16(dw)) return LADDER_E_ALIGN;
    int splits, mps;
    dense_wgrad_f32_plan(M, K, N, &splits, &mps);
    const WgradTail t = wgrad_tail(ws, splits, (size_t)K * N, N, dw, db);
    const int rc = dense_wgrad_f32_launch(x, dy, t.part, t.bias_part, M, K, N, splits, mps, stream);
    if (rc != LADDER_OK) return rc;
    return t.reduce(stream);
  }
  return run_wgrad(x, dy, dw, db, dense_desc(M, K, N, LADDER_ACT_NONE), ws, ws_bytes, stream);
}

}  // extern "C"
