// The opt-in split-precision (f16x3 / bf16x3 / bf16x6, split16.h) forms of the gather kernels of igemm.hip / igemm_wgrad.hip; the 3x3 halo
// layers have their own kernels in convsplit.hip.
#include "igemm.h"

namespace {

// The gather kernel on split operands (precision formats of split16.h / convsplit.hip): 128x128 tile, 4 wavefronts of 64x64, 32-channel
// K chunks = two 32x32x16 MFMA K-steps.  A is gathered exactly like igemm_fwd_kernel's fast path (tap table + validity mask) but from the
// PRE-SPLIT 16-bit planes of the input (ladder_presplit: an element is re-read once per tap and per output-channel tile, 18-36 times;
// splitting it in this kernel each time cost 38 % of its run time) straight into LDS ([plane][k-step][channel octet][row][8 x 16 bit]:
// a fragment = 32 consecutive 16-byte slots); B comes pre-split from ladder_filter_pack_split, whose blocks already have that layout.
constexpr int GS_BM = 128, GS_BN = 128, GS_BK = 32;

// ladder_presplit leaves behind the planes: 16 zero bytes (the source of padding taps), then a 16-byte header whose first word says
// whether the planes carry one scale per SAMPLE (f16x3, mode-1 absmax record) or one for the tensor.
__device__ __forceinline__ bool planes_per_sample(const uint16_t* planes, size_t plane_elems, int ns) {
  return reinterpret_cast<const uint32_t*>(planes + (size_t)ns * plane_elems)[4] != 0u;
}
constexpr int GS_PLANE = 2 * 2 * 128 * 16;      // bytes per plane of either operand tile (8192)

template <int PREC>
__global__ __launch_bounds__(kThreads, 2) void igemm_fwd_split_kernel(const uint16_t* __restrict__ xp, const size_t plane_elems,
                                                                     const uint4* __restrict__ wp,
                                                                     const float* __restrict__ bias, float* __restrict__ y,
                                                                     const IgemmDesc d, const int tiles_n, float* __restrict__ part,
                                                                     const int chunks_per_split, const float* __restrict__ gate,
                                                                     const int gate_act, const float* __restrict__ xamax,
                                                                     const float* __restrict__ wamax, float* __restrict__ stats_part) {
  constexpr int NS = Fmt<PREC>::NS;
  constexpr bool F16 = Fmt<PREC>::F16;
  constexpr int OPB = NS * GS_PLANE;                       // bytes of one operand tile
  constexpr int AU = GS_BM * (GS_BK / 8) / kThreads;       // 2 (row, channel octet) units per thread, NS 16-byte loads each
  constexpr int B_CHUNKS = 2 * NS * 256;                   // 16-byte chunks of the B tile (two packed blocks)
  constexpr int BU = B_CHUNKS / kThreads;                  // 4 (NS=2) / 6 (NS=3)
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * 2 * OPB];   // [buffer][A | B]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int wm = wid >> 1, wn = wid & 1;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (tile / tiles_n) * GS_BM, cot = tile % tiles_n, n0 = cot * GS_BN;
  const int HoWo = d.Ho * d.Wo;
  const int nslabs16 = d.Cin / 16;
  // f16x3: the planes were scaled by ladder_presplit -- with ONE scale for the tensor or with one per sample (flag word behind the
  // planes); a GEMM row is one output pixel = one sample, so the un-scale factor is a per-row constant (table in LDS for the epilogue)
  float tmax = 0.f, cw = 1.f;
  bool x_ps = false;
  if (F16) {
    tmax = amax_load(xamax);
    cw = scale_from_absmax(amax_load(wamax));
    x_ps = planes_per_sample(xp, plane_elems, NS);
  }
  // (thread r < 128 fetches the scale of tile row r now: the load has the whole main loop to arrive)
  float my_row_scale = 1.f;
  if (F16 && tid < GS_BM) my_row_scale = scale_for_sample(xamax, (int)fdiv((uint32_t)min(m0 + tid, d.M - 1), d.div_howo), x_ps, tmax);

  long a_off[AU];                                          // element offset of the unit at tap (0,0), channel slab 0
  uint32_t a_mask[AU];
  int a_dst[AU];
#pragma unroll
  for (int i = 0; i < AU; ++i) {
    const int u = tid + i * kThreads;
    const int row = u >> 2, oct = u & 3;                   // oct = k-step * 2 + channel octet of the 32-channel chunk
    const int m = m0 + row;
    const bool ok = m < d.M;
    const uint32_t mm = ok ? m : 0;
    const uint32_t n_img = fdiv(mm, d.div_howo), rem = mm - n_img * HoWo;
    const uint32_t ho = fdiv(rem, d.div_wo), wo = rem - ho * d.Wo;
    const int bh = (int)ho * d.stride - d.pad_t, bw = (int)wo * d.stride - d.pad_l;
    a_off[i] = (long)n_img * d.H * d.W * d.Cin + ((long)bh * d.W + bw) * d.Cin + oct * 8;
    uint32_t msk = 0;
    if (ok)
      for (int t = 0; t < d.ntaps; ++t) {
        const int nh = bh + d.tap_dh[t], nw = bw + d.tap_dw[t];
        if (nh >= 0 && nh < d.H && nw >= 0 && nw < d.W) msk |= 1u << t;
      }
    a_mask[i] = msk;
    a_dst[i] = (oct * 128 + row) * 16;
  }

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  static_assert(AU == 2, "two A units per thread");
  uint4 ra00, ra01, ra02, ra10, ra11, ra12;                // [unit][plane]  (named: hipcc demotes a uint4 array captured by two
  uint4 rb0, rb1, rb2, rb3, rb4, rb5;                      //  lambdas to LDS)
  static_assert(BU == 4 || BU == 6, "B staging rounds");
  auto load_chunk = [&](int c) {
    const int t = c % d.ntaps, ci0 = (c / d.ntaps) * GS_BK;
    const long coff = ((long)d.tap_dh[t] * d.W + d.tap_dw[t]) * d.Cin + ci0;
#define GS_ASRC(i_, p_) *reinterpret_cast<const uint4*>(((a_mask[i_] >> t) & 1u) ? (const void*)(xp + (size_t)(p_) * plane_elems + a_off[i_] + coff) \
                                                                             : (const void*)g_zero16)
    ra00 = GS_ASRC(0, 0); ra01 = GS_ASRC(0, 1); ra10 = GS_ASRC(1, 0); ra11 = GS_ASRC(1, 1);
    if (NS > 2) { ra02 = GS_ASRC(0, 2); ra12 = GS_ASRC(1, 2); }
#undef GS_ASRC
    const uint4* bs = wp + (((size_t)d.tap_w[t] * nslabs16 + ci0 / 16) * tiles_n + cot) * (NS * 256);
    // unit i = (k-step i / NS, plane i % NS), 256 threads x 16 B each
#define GS_BSRC(i_) bs[(size_t)((i_) / NS) * tiles_n * (NS * 256) + ((i_) % NS) * 256 + tid]
    rb0 = GS_BSRC(0); rb1 = GS_BSRC(1); rb2 = GS_BSRC(2); rb3 = GS_BSRC(3);
    if (BU > 4) { rb4 = GS_BSRC(4); rb5 = GS_BSRC(5); }
#undef GS_BSRC
  };
  auto store_chunk = [&](int buf) {
    unsigned char* Ab = lds + buf * 2 * OPB;
#define GS_ADST(i_, p_) *reinterpret_cast<uint4*>(Ab + (p_) * GS_PLANE + a_dst[i_])
    GS_ADST(0, 0) = ra00; GS_ADST(0, 1) = ra01; GS_ADST(1, 0) = ra10; GS_ADST(1, 1) = ra11;
    if (NS > 2) { GS_ADST(0, 2) = ra02; GS_ADST(1, 2) = ra12; }
#undef GS_ADST
#define GS_BDST(i_) *reinterpret_cast<uint4*>(Ab + OPB + ((i_) % NS) * GS_PLANE + (((i_) / NS) * 256 + tid) * 16)
    GS_BDST(0) = rb0; GS_BDST(1) = rb1; GS_BDST(2) = rb2; GS_BDST(3) = rb3;
    if (BU > 4) { GS_BDST(4) = rb4; GS_BDST(5) = rb5; }
#undef GS_BDST
  };
  auto mma_chunk = [&](int buf) {
    const unsigned char* Ab = lds + buf * 2 * OPB + (lh * 128 + wm * 64 + l31) * 16;
    const unsigned char* Bb = lds + buf * 2 * OPB + OPB + (lh * 128 + wn * 64 + l31) * 16;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 a[2][NS], b[2][NS];
#pragma unroll
      for (int p = 0; p < NS; ++p) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) a[mi][p] = *reinterpret_cast<const uint4*>(Ab + p * GS_PLANE + ks * 4096 + mi * 512);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) b[ni][p] = *reinterpret_cast<const uint4*>(Bb + p * GS_PLANE + ks * 4096 + ni * 512);
      }
#pragma unroll
      for (int sum = NS - 1; sum >= 0; --sum)
#pragma unroll
        for (int pa = 0; pa <= sum; ++pa) {
          const int pb = sum - pa;
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma16<F16>(a[mi][pa], b[ni][pb], acc[mi][ni]);
        }
    }
  };

  const int c_begin = blockIdx.y * chunks_per_split;
  const int nchunks = min(d.ntaps * (d.Cin / GS_BK), c_begin + chunks_per_split);
  load_chunk(c_begin);
  store_chunk(0);
  __syncthreads();
  for (int c = c_begin; c < nchunks; ++c) {
    const int buf = (c - c_begin) & 1;
    if (c + 1 < nchunks) load_chunk(c + 1);
    mma_chunk(buf);
    if (c + 1 < nchunks) store_chunk(buf ^ 1);
    __syncthreads();
  }

  float* const row_unscale = reinterpret_cast<float*>(lds);   // (the operand tiles are dead after the last barrier of the main loop)
  if (F16) {
    if (tid < GS_BM) row_unscale[tid] = 1.f / (my_row_scale * cw);       // exact: powers of two
    __syncthreads();
  }
  if (part != nullptr) {   // split-K partial: un-scaled accumulators, bias/activation applied by splitk_epilogue_kernel
    float* o = part + (size_t)blockIdx.y * d.M * d.Cout;
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int n = n0 + wn * 64 + ni * 32 + l31;
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = m0 + wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
          if (m < d.M && n < d.Cout) o[(long)m * d.Cout + n] = F16 ? acc[mi][ni][e] * row_unscale[m - m0] : acc[mi][ni][e];
        }
    }
    return;
  }
  const bool dense_out = d.out_sh == 1 && d.out_sw == 1 && d.OH == d.Ho && d.OW == d.Wo;
  // batch-norm statistics of what is written (lane = output channel: the column sums are local), stats_part [tile_m][4][Cout] =
  // sum | sum of squares | min | max per tile, reduced by ladder_bn_stats_minmax_from_partials
  float st0[2] = {0.f, 0.f}, st1[2] = {0.f, 0.f}, smn[2] = {INFINITY, INFINITY}, smx[2] = {-INFINITY, -INFINITY};
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int n = n0 + wn * 64 + ni * 32 + l31;
    const float bv = (bias != nullptr && n < d.Cout) ? bias[n] : 0.f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (m < d.M && n < d.Cout) {
          long row = m;
          if (!dense_out) {
            const uint32_t n_img = fdiv((uint32_t)m, d.div_howo), rem = (uint32_t)m - n_img * HoWo;
            const uint32_t ho = fdiv(rem, d.div_wo), wo = rem - ho * d.Wo;
            row = ((long)n_img * d.OH + d.out_h0 + (long)ho * d.out_sh) * d.OW + d.out_w0 + (long)wo * d.out_sw;
          }
          float v = ladder_act_fn((F16 ? acc[mi][ni][e] * row_unscale[m - m0] : acc[mi][ni][e]) + bv, d.act);
          if (gate != nullptr) v *= ladder_act_grad_from_out(gate[row * d.Cout + n], gate_act);
          y[row * d.Cout + n] = v;
          st0[ni] += v;
          st1[ni] += v * v;
          smn[ni] = fminf(smn[ni], v);
          smx[ni] = fmaxf(smx[ni], v);
        }
      }
    }
  }
  if (stats_part != nullptr) {
    float* sred = reinterpret_cast<float*>(lds);             // [which 4][wm 2][128 channels] (the operand tiles are dead)
    __syncthreads();
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const float a0 = st0[ni] + __shfl_xor(st0[ni], 32, 64), a1 = st1[ni] + __shfl_xor(st1[ni], 32, 64);
      const float a2 = fminf(smn[ni], __shfl_xor(smn[ni], 32, 64)), a3 = fmaxf(smx[ni], __shfl_xor(smx[ni], 32, 64));
      if (lh == 0) {
        const int cc = wn * 64 + ni * 32 + l31;
        sred[(0 * 2 + wm) * 128 + cc] = a0;
        sred[(1 * 2 + wm) * 128 + cc] = a1;
        sred[(2 * 2 + wm) * 128 + cc] = a2;
        sred[(3 * 2 + wm) * 128 + cc] = a3;
      }
    }
    __syncthreads();
    for (int t = tid; t < 4 * 128; t += kThreads) {
      const int which = t >> 7, c = t & 127;
      const float v0 = sred[(which * 2 + 0) * 128 + c], v1 = sred[(which * 2 + 1) * 128 + c];
      const float r = which < 2 ? v0 + v1 : (which == 2 ? fminf(v0, v1) : fmaxf(v0, v1));
      if (n0 + c < d.Cout) stats_part[((size_t)(tile / tiles_n) * 4 + which) * d.Cout + n0 + c] = r;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// Filter / weight gradient on split operands: dW[k' x n] = sum_pixels A[pixel][k'] * dY[pixel][n], k' = (tap, ci).  The reduction index
// is the pixel while both operands are channel-contiguous in memory, so the LDS images stay [32-channel block][pixel][32 ch x 16 bit]
// (written by plain 8-byte stores of split float4s) and the MFMA fragments -- 8 consecutive pixels of one channel per lane -- are
// fetched with the transposing LDS read (ds_read_b64_tr_b16; see wgrad3x3_split_kernel in convsplit.hip for the layout argument).
// 128 x 128 tile (one filter tap x 128 input channels, Cin % 128 == 0), 4 wavefronts of 64x64, 32-pixel chunks, pixel range split
// over gridDim.y with a fixed-order second stage.
constexpr int GW_BLK = 32 * 64;                 // bytes of one 32-channel block of a 32-pixel chunk (2048)
constexpr int GW_PLANE = 4 * GW_BLK;            // 128 channels (8192)
typedef short gw_s16x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint4 gw_tr_frag(const unsigned char* p) {
  const gw_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) gw_s16x4*)(p));
  const gw_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) gw_s16x4*)(p + 4 * 64));
  const uint2 a = __builtin_bit_cast(uint2, lo), b = __builtin_bit_cast(uint2, hi);
  return make_uint4(a.x, a.y, b.x, b.y);
}
template <bool F16>
__device__ __forceinline__ float gw_frag_sum(const uint4 f) {
  const uint32_t w[4] = {f.x, f.y, f.z, f.w};
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (F16) {
      const f32x2 v = __builtin_convertvector(__builtin_bit_cast(f16x2, w[i]), f32x2);
      s += v.x + v.y;
    } else {
      s += __builtin_bit_cast(float, w[i] << 16) + __builtin_bit_cast(float, w[i] & 0xffff0000u);
    }
  }
  return s;
}

template <int PREC>
__global__ __launch_bounds__(kThreads, 2) void igemm_wgrad_split_kernel(const uint16_t* __restrict__ xp, const size_t x_plane_elems,
                                                                       const uint16_t* __restrict__ dyp, const size_t dy_plane_elems,
                                                                       float* __restrict__ out, float* __restrict__ bias_part,
                                                                       const IgemmDesc d, const int tiles_n, const int m_per_split,
                                                                       const float* __restrict__ xamax, const float* __restrict__ damax) {
  constexpr int NS = Fmt<PREC>::NS;
  constexpr bool F16 = Fmt<PREC>::F16;
  constexpr int OPB = NS * GW_PLANE;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * 2 * OPB];     // [buffer][A | dY]

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5, l15 = lane & 15;
  const int wm = wid >> 1, wn = wid & 1;
  const int tile = blockIdx.x;
  const int k0t = (tile / tiles_n) * 128, n0 = (tile % tiles_n) * 128;
  const int HoWo = d.Ho * d.Wo;
  const int p_begin = blockIdx.y * m_per_split;
  const int p_end = min(d.M, p_begin + m_per_split);
  const int tap = k0t / d.Cin, ci0 = k0t - tap * d.Cin;       // the tile lies inside one tap (Cin % 128 == 0)
  const int tr = tap / d.KW, ts = tap - tr * d.KW;
  // f16x3 scales: either operand's planes may carry one scale per sample (ladder_presplit).  The reduction runs over the pixels of ALL
  // samples, so the accumulators hold s * (partial sum) with s = cx(n) * cd(n) of the sample being reduced and are multiplied by
  // s_new / s_old (a power of two: exact) whenever a 32-pixel chunk starts in another sample.  Needs chunks inside one sample.
  // The scales of the samples this workgroup reduces over are gathered ONCE into an LDS table (vector loads, counted by vmcnt like the chunk
  // loads they precede): scalar loads between the segments made the first LDS wait of every segment stall on them (lgkmcnt counts both).
  constexpr int GW_NSC = 256;
  __shared__ float2 seg_scale[GW_NSC];                       // [sample - n_first] = {cx * cd, cd}
  float xt = 0.f, dt = 0.f, s_cur = 1.f, cd_cur = 1.f;
  bool x_ps = false, d_ps = false;
  int n_cur = 0, n_first = 0;
  if (F16) {
    xt = amax_load(xamax);
    dt = amax_load(damax);
    x_ps = planes_per_sample(xp, x_plane_elems, NS);
    d_ps = planes_per_sample(dyp, dy_plane_elems, NS);
    if ((x_ps || d_ps) && ((HoWo % 32) != 0 || (p_begin % 32) != 0)) __builtin_trap();     // the caller asked for per-sample planes on a map it must not
    n_first = n_cur = (int)fdiv((uint32_t)min(p_begin, d.M - 1), d.div_howo);
    // (one entry when both operands carry a single scale; else m_per_split / HoWo + 1 samples per workgroup: far below the table size)
    const int n_tab = (x_ps || d_ps) ? (int)fdiv((uint32_t)(max(p_end, p_begin + 1) - 1), d.div_howo) - n_first : 0;
    if (n_tab >= GW_NSC) __builtin_trap();
    if (tid <= n_tab) {
      const float cdn = scale_for_sample(damax, n_first + tid, d_ps, dt);
      seg_scale[tid] = make_float2(scale_for_sample(xamax, n_first + tid, x_ps, xt) * cdn, cdn);
    }
  }
  const bool do_bias = (bias_part != nullptr) && (tile / tiles_n == 0) && wm == 0;
  float bsum[2] = {0.f, 0.f};

  // staging units: 32 pixels x 16 channel octets per operand = 512 units = 2 per thread and operand, NS 16-byte plane loads each;
  // unit u -> pixel u >> 4, octet u & 15 (both operands arrive pre-split: ladder_presplit)
  const int s_pix = tid >> 4, s_oct = tid & 15;              // + 16 pixels for the second round
  const int s_dst = (s_oct >> 2) * GW_BLK + s_pix * 64 + (s_oct & 3) * 16;   // + round * 16 * 64
  const bool n_ok = (n0 + s_oct * 8) < d.Cout;
  const int frag_lane = (8 * lh + (l15 >> 2)) * 64 + (16 * ((lane >> 4) & 1) + 4 * (l15 & 3)) * 2;

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  uint4 ra00, ra01, ra02, ra10, ra11, ra12, rd00, rd01, rd02, rd10, rd11, rd12;     // [round][plane] (named: see igemm_fwd_split_kernel)
  auto unit_offsets = [&](int pc, int round, long& ao, long& dof) {
    const int p = pc + s_pix + round * 16;
    ao = dof = -1;
    if (p < p_end) {
      const uint32_t n_img = fdiv((uint32_t)p, d.div_howo), rem = (uint32_t)p - n_img * HoWo;
      const int ho = (int)fdiv(rem, d.div_wo), wo = (int)rem - ho * d.Wo;
      const int hi = ho * d.stride - d.pad_t + tr, wi = wo * d.stride - d.pad_l + ts;
      if (hi >= 0 && hi < d.H && wi >= 0 && wi < d.W) ao = (((long)n_img * d.H + hi) * d.W + wi) * d.Cin + ci0 + s_oct * 8;
      if (n_ok) dof = (long)p * d.Cout + n0 + s_oct * 8;
    }
  };
#define GW_LD(base_, elems_, off_, p_) *reinterpret_cast<const uint4*>((off_) >= 0 ? (const void*)((base_) + (size_t)(p_) * (elems_) + (off_)) \
                                                                                : (const void*)g_zero16)
  auto load_chunk = [&](int c) {
    const int pc = p_begin + c * 32;
    long ao, dof;
    unit_offsets(pc, 0, ao, dof);
    ra00 = GW_LD(xp, x_plane_elems, ao, 0); ra01 = GW_LD(xp, x_plane_elems, ao, 1);
    rd00 = GW_LD(dyp, dy_plane_elems, dof, 0); rd01 = GW_LD(dyp, dy_plane_elems, dof, 1);
    if (NS > 2) { ra02 = GW_LD(xp, x_plane_elems, ao, 2); rd02 = GW_LD(dyp, dy_plane_elems, dof, 2); }
    unit_offsets(pc, 1, ao, dof);
    ra10 = GW_LD(xp, x_plane_elems, ao, 0); ra11 = GW_LD(xp, x_plane_elems, ao, 1);
    rd10 = GW_LD(dyp, dy_plane_elems, dof, 0); rd11 = GW_LD(dyp, dy_plane_elems, dof, 1);
    if (NS > 2) { ra12 = GW_LD(xp, x_plane_elems, ao, 2); rd12 = GW_LD(dyp, dy_plane_elems, dof, 2); }
  };
#undef GW_LD
  auto store_chunk = [&](int buf) {
    unsigned char* Ab = lds + buf * 2 * OPB;
#define GW_ST(op_, round_, p_) *reinterpret_cast<uint4*>(Ab + (op_) * OPB + (p_) * GW_PLANE + s_dst + (round_) * 16 * 64)
    GW_ST(0, 0, 0) = ra00; GW_ST(0, 0, 1) = ra01; GW_ST(0, 1, 0) = ra10; GW_ST(0, 1, 1) = ra11;
    GW_ST(1, 0, 0) = rd00; GW_ST(1, 0, 1) = rd01; GW_ST(1, 1, 0) = rd10; GW_ST(1, 1, 1) = rd11;
    if (NS > 2) { GW_ST(0, 0, 2) = ra02; GW_ST(0, 1, 2) = ra12; GW_ST(1, 0, 2) = rd02; GW_ST(1, 1, 2) = rd12; }
#undef GW_ST
  };
  auto mma_chunk = [&](int buf) {
    const unsigned char* Ab = lds + buf * 2 * OPB + frag_lane + wm * 2 * GW_BLK;
    const unsigned char* Bb = lds + buf * 2 * OPB + OPB + frag_lane + wn * 2 * GW_BLK;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      uint4 a[2][NS], b[2][NS];
#pragma unroll
      for (int p = 0; p < NS; ++p) {
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) a[mi][p] = gw_tr_frag(Ab + p * GW_PLANE + mi * GW_BLK + ks * 16 * 64);
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) b[ni][p] = gw_tr_frag(Bb + p * GW_PLANE + ni * GW_BLK + ks * 16 * 64);
      }
#pragma unroll
      for (int sum = NS - 1; sum >= 0; --sum)
#pragma unroll
        for (int pa = 0; pa <= sum; ++pa) {
          const int pb = sum - pa;
#pragma unroll
          for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = mfma16<F16>(a[mi][pa], b[ni][pb], acc[mi][ni]);
        }
      if (do_bias) {
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
          for (int p = NS - 1; p >= 0; --p) bsum[ni] += gw_frag_sum<F16>(b[ni][p]);
      }
    }
  };

  const int nchunks = (p_end - p_begin + 31) / 32;
  if (nchunks > 0) {
    load_chunk(0);
    store_chunk(0);
  }
  __syncthreads();
  // chunk loop in SEGMENTS of chunks that share their scales (per-sample planes: the chunks of one sample; else one segment): the inner
  // loop is the plain pipelined loop, all re-scaling sits between segments (a test inside the chunk loop cost the kernel 19 %)
  if (F16) {                                                 // (after the barrier above: the table is complete)
    s_cur = seg_scale[0].x;
    cd_cur = seg_scale[0].y;
  }
  const bool any_ps = F16 && (x_ps || d_ps);
  const int cps = any_ps ? HoWo / 32 : nchunks;             // chunks per sample (HoWo % 32 == 0 and p_begin % 32 == 0 were checked)
  int c = 0;
  int seg_end = any_ps ? min(nchunks, cps - (int)((uint32_t)(p_begin / 32) - (uint32_t)n_cur * (uint32_t)cps)) : nchunks;
  while (c < nchunks) {
    // the NEXT segment's scales are fetched now and used after this segment's chunks
    float s_nxt = s_cur, cd_nxt = cd_cur;
    if (any_ps && seg_end < nchunks) {
      const float2 e = seg_scale[n_cur + 1 - n_first];
      s_nxt = e.x;
      cd_nxt = e.y;
    }
    for (; c < seg_end; ++c) {
      const int buf = c & 1;
      if (c + 1 < nchunks) load_chunk(c + 1);
      mma_chunk(buf);
      if (c + 1 < nchunks) store_chunk(buf ^ 1);
      __syncthreads();
    }
    if (c < nchunks) {                                       // entering the next sample: re-scale the accumulators (powers of two: exact)
      if (s_nxt != s_cur || cd_nxt != cd_cur) {
        const float ratio = s_nxt / s_cur, bratio = cd_nxt / cd_cur;
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mi][ni][e] *= ratio;
        bsum[0] *= bratio;
        bsum[1] *= bratio;
      }
      ++n_cur; s_cur = s_nxt; cd_cur = cd_nxt;
      seg_end = min(nchunks, seg_end + cps);
    }
  }

  const float unscale = F16 ? 1.f / s_cur : 1.f;
  const float cd = cd_cur;
  float* o = out + (size_t)blockIdx.y * d.K * d.Cout;
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int n = n0 + wn * 64 + ni * 32 + l31;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int k = k0t + wm * 64 + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (k < d.K && n < d.Cout) o[(long)k * d.Cout + n] = acc[mi][ni][e] * unscale;
      }
    }
    if (do_bias) {
      const float v = (bsum[ni] + __shfl_down(bsum[ni], 32, 64)) * (F16 ? 1.f / cd : 1.f);
      if (lh == 0 && n < d.Cout) bias_part[(size_t)blockIdx.y * d.Cout + n] = v;
    }
  }
}

// `small_ok`: a few 128x128 tiles can still fill the chip through split-K (the 8x8 ... 1x1 ends of the CelebA encoder / decoder:
// M = 128 ... 8192 pixels, K = 256 ... 8192; strided outputs -- the parity classes of a stride-2 backward-data -- go through
// splitk_epilogue_strided_kernel)
bool split_gather_ok(const IgemmDesc& d, bool small_ok = false) {
  if (!(d.ntaps > 0 && d.ntaps <= 28 && d.ups == 1 && (d.Cin % GS_BK) == 0 && d.M > 0)) return false;
  if (select_fwd_tile(d.M, d.Cout) == 128128) return true;
  return small_ok && d.M >= 128 && d.Cout >= 128;
}

// Split-K plan of the split gather kernel (32-deep chunks).  Measured at B = 128: with >= 384 tiles (two workgroups per CU, 75 % full)
// the partial traffic costs more than the idle CUs (dec.conv4, 512 tiles: 252 TF with 2 splits, 267 without; the stride-2 encoder layer
// 172 vs 218); around 256 tiles a LONG reduction still gains from 4 splits (dec.conv3, K = 4608: 237 vs 189 TF) while a short one (a
// parity class of a stride-2 backward-data, K <= 1024) does not; a split keeps at least 8 chunks (K = 256).
SplitPlan plan_splitk32(const IgemmDesc& d) {
  const int nchunks = d.ntaps * (d.Cin / GS_BK);
  const long tiles = (long)((d.M + GS_BM - 1) / GS_BM) * ((d.Cout + GS_BN - 1) / GS_BN);
  SplitPlan p{1, nchunks};
  if (tiles >= 384 || nchunks < 16 || (tiles >= 192 && nchunks < 64)) return p;
  long s = (1024 + tiles - 1) / tiles;
  if (s > nchunks / 8) s = nchunks / 8;
  if (s > 32) s = 32;
  if (s < 2) return p;
  p.cps = (int)((nchunks + s - 1) / s);
  p.splits = (nchunks + p.cps - 1) / p.cps;
  return p;
}

size_t fwd_split_ws_bytes(const IgemmDesc& d) {
  const SplitPlan sp = plan_splitk32(d);
  return sp.splits > 1 ? (size_t)sp.splits * d.M * d.Cout * sizeof(float) : 0;
}

int launch_fwd_split(const void* x, const float* xamax, const void* packed, const float* bias, float* y, const IgemmDesc& d, int prec,
                     void* ws, size_t ws_bytes, hipStream_t st, const float* gate, int gate_act, float* stats_part = nullptr) {
  // `x` = the pre-split planes of the gathered tensor (ladder_presplit), plane-major, d.N*d.H*d.W*d.Cin elements per plane
  const bool dense_out = d.out_sh == 1 && d.out_sw == 1 && d.OH == d.Ho && d.OW == d.Wo;
  if (!split_gather_ok(d, true) || !prec_ok(prec)) return LADDER_E_SHAPE;
  if (!ladder_aligned16(x) || !ladder_aligned16(packed) || !ladder_aligned16(y)) return LADDER_E_ALIGN;
  const size_t plane_elems = (size_t)d.N * d.H * d.W * d.Cin;
  if (prec == LADDER_PREC_F16X3 && xamax == nullptr) return LADDER_E_SHAPE;
  const int tiles_m = (d.M + GS_BM - 1) / GS_BM, tiles_n = (d.Cout + GS_BN - 1) / GS_BN;
  SplitPlan sp = plan_splitk32(d);
  const size_t need = (size_t)sp.splits * d.M * d.Cout * sizeof(float);
  if (sp.splits > 1 && (ws == nullptr || ws_bytes < need)) sp = SplitPlan{1, d.ntaps * (d.Cin / GS_BK)};
  float* part = sp.splits > 1 ? (float*)ws : nullptr;
  if (stats_part != nullptr && (part != nullptr || !dense_out)) return LADDER_E_SHAPE;   // statistics come from the single-pass epilogue
  const float* wamax = reinterpret_cast<const float*>(static_cast<const unsigned char*>(packed) + pack_payload_bytes(d.KH * d.KW, d.Cin, d.Cout, prec));
  const dim3 grid(tiles_m * tiles_n, sp.splits), block(kThreads);
  LADDER_PREC_SWITCH(prec, hipLaunchKernelGGL(igemm_fwd_split_kernel<PP>, grid, block, 0, st, (const uint16_t*)x, plane_elems, (const uint4*)packed, bias, y, d,
                                              tiles_n, part, sp.cps, part ? nullptr : gate, gate_act, xamax, wamax, stats_part));
  if (part != nullptr) launch_splitk_epilogue(part, bias, y, sp.splits, d, gate, gate_act, st);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

// ---- split filter gradient: planning shared by the workspace query and the launcher
bool wgrad_split_ok(const IgemmDesc& d) {
  if (d.ups != 1 || (d.Cin % 128) != 0 || d.Cout <= 64 || (d.Cout % 8) != 0 || d.M < 128) return false;
  const WgradPlan p = plan_wgrad(d.M, d.K, d.Cout);
  return p.bm == 128 && p.bn == 128;
}
WgradPlan plan_wgrad_split32(const IgemmDesc& d) {
  WgradPlan p = plan_wgrad(d.M, d.K, d.Cout);
  // this kernel keeps 2 workgroups per CU resident: exactly ONE full round of the chip (512) measured best on every layer (dec.conv4
  // 347 us against 377 us with the fp32 kernel's 768-slot plan, enc.conv2 186 / 223 us); at least 256 pixels per split
  {
    const long tiles = (long)p.tiles_k * p.tiles_n;
    long s = 512 / tiles;
    const long max_s = (d.M + 255) / 256;
    if (s > max_s) s = max_s;
    if (s < 1) s = 1;
    p.m_per_split = (int)((d.M + s - 1) / s);
  }
  long mps = (p.m_per_split + 31) / 32 * 32;           // 32-pixel chunks
  p.m_per_split = (int)mps;
  p.splits = (int)((d.M + mps - 1) / mps);
  return p;
}
size_t wgrad_split_ws_bytes(const IgemmDesc& d) {
  const WgradPlan p = plan_wgrad_split32(d);
  return ((size_t)p.splits * d.K * d.Cout + (size_t)p.splits * d.Cout) * sizeof(float);
}
int run_wgrad_split(const void* x, const float* xamax, const void* dy, const float* damax, float* dw, float* db, const IgemmDesc& d,
                    int prec, void* ws, size_t ws_bytes, hipStream_t st) {
  // x, dy = pre-split planes (ladder_presplit) of the layer input [N,H,W,Cin] and of the output gradient [N,Ho,Wo,Cout]
  if (!wgrad_split_ok(d) || !prec_ok(prec)) return LADDER_E_SHAPE;
  if (!ladder_aligned16(x) || !ladder_aligned16(dy) || !ladder_aligned16(dw)) return LADDER_E_ALIGN;
  if (prec == LADDER_PREC_F16X3 && (xamax == nullptr || damax == nullptr)) return LADDER_E_SHAPE;
  if (ws == nullptr || ws_bytes < wgrad_split_ws_bytes(d)) return LADDER_E_WORKSPACE;
  const WgradPlan p = plan_wgrad_split32(d);
  const WgradTail t = wgrad_tail(ws, p.splits, (size_t)d.K * d.Cout, d.Cout, dw, db);
  const dim3 grid(p.tiles_k * p.tiles_n, p.splits), block(kThreads);
  LADDER_PREC_SWITCH(prec, hipLaunchKernelGGL(igemm_wgrad_split_kernel<PP>, grid, block, 0, st, (const uint16_t*)x, (size_t)d.N * d.H * d.W * d.Cin,
                                              (const uint16_t*)dy, (size_t)d.M * d.Cout, t.part, t.bias_part, d, p.tiles_n, p.m_per_split, xamax, damax));
  return t.reduce(st);
}

}  // namespace

extern "C" {

// ---- split-precision variants of the forward-type convolution calls (gather kernel; the 3x3 halo layers have their own entry points
// in convsplit.hip).  `dry` = only report whether every launch of the call would run on the split kernel.
static int conv2d_fwd_split_impl(const void* x, const float* x_absmax, const void* packed, const float* bias, float* y, int N, int H,
                                 int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int act,
                                 int prec, void* ws, size_t ws_bytes, ladder_stream_t stream, bool dry, size_t* ws_need) {
  if (!conv_shape_ok(N, H, W, Cin, Ho, Wo, KH, KW, stride)) return LADDER_E_SHAPE;
  const IgemmDesc d = conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, 1, pad_t, pad_l, act);
  if (!split_gather_ok(d, true) || halo_eligible(d)) return LADDER_E_SHAPE;
  if (ws_need != nullptr) *ws_need = fwd_split_ws_bytes(d);
  if (dry) return LADDER_OK;
  return launch_fwd_split(x, x_absmax, packed, bias, y, d, prec, ws, ws_bytes, stream, nullptr, 0);
}

static int conv2d_bwd_data_split_impl(const void* dy, const float* dy_absmax, const void* packed, float* dx, int N, int H, int W, int Cin,
                                      int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, const float* gate_y,
                                      int gate_act, int prec, void* ws, size_t ws_bytes, ladder_stream_t stream, bool dry, size_t* ws_need) {
  if (!conv_shape_ok(N, H, W, Cin, Ho, Wo, KH, KW, stride)) return LADDER_E_SHAPE;
  const IgemmDesc d = bwd_data_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l);
  if (ws_need != nullptr) *ws_need = 0;
  if (stride == 1) {
    if (!split_gather_ok(d, true) || (gate_y == nullptr && halo_eligible(d))) return LADDER_E_SHAPE;
    if (ws_need != nullptr) *ws_need = fwd_split_ws_bytes(d);
    if (dry) return LADDER_OK;
    return launch_fwd_split(dy, dy_absmax, packed, nullptr, dx, d, prec, ws, ws_bytes, stream, gate_y, gate_act);
  }
  if (stride != 2 || KH * KW > 28) return LADDER_E_SHAPE;
  IgemmDesc cls[4];
  parity_classes(d, cls);
  for (const IgemmDesc& c : cls) {                       // every parity class must be eligible (a class without pixels or taps is not)
    if (!split_gather_ok(c, true)) return LADDER_E_SHAPE;
    if (ws_need != nullptr && fwd_split_ws_bytes(c) > *ws_need) *ws_need = fwd_split_ws_bytes(c);   // (classes run one after another)
  }
  if (dry) return LADDER_OK;
  for (const IgemmDesc& c : cls) {
    const int rc = launch_fwd_split(dy, dy_absmax, packed, nullptr, dx, c, prec, ws, ws_bytes, stream, gate_y, gate_act);
    if (rc != LADDER_OK) return rc;
  }
  return LADDER_OK;
}

int ladder_conv2d_fwd_split_eligible(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t,
                                     int pad_l) {
  return conv2d_fwd_split_impl(nullptr, nullptr, nullptr, nullptr, nullptr, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l, 0,
                               LADDER_PREC_F16X3, nullptr, 0, nullptr, true, nullptr) == LADDER_OK ? 1 : 0;
}

size_t ladder_conv2d_fwd_split_workspace_bytes(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                               int pad_t, int pad_l) {
  size_t need = 0;
  conv2d_fwd_split_impl(nullptr, nullptr, nullptr, nullptr, nullptr, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l, 0,
                        LADDER_PREC_F16X3, nullptr, 0, nullptr, true, &need);
  return need;
}

int ladder_conv2d_fwd_split(const void* x_planes, const float* x_absmax, const void* packed, const float* bias, float* y, int N, int H, int W,
                            int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int act, int prec,
                            void* ws, size_t ws_bytes, ladder_stream_t stream) {
  return conv2d_fwd_split_impl(x_planes, x_absmax, packed, bias, y, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l, act, prec, ws,
                               ws_bytes, stream, false, nullptr);
}

// Forward + the batch-norm statistics of its output (sums4 = the statistics record, minmax form: 2 Cout doubles sum | sum of squares, then min | max, as
// ladder_bn_fwd_stats_minmax computes them from a second pass over y) from the epilogue's per-tile column statistics.  Available when the
// call runs without split-K (workspace query > 0): the partial sums of a split reduction never see the finished values.
size_t ladder_conv2d_fwd_split_bnstats_workspace_bytes(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                                       int pad_t, int pad_l) {
  if (!ladder_conv2d_fwd_split_eligible(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l)) return 0;
  if (ladder_conv2d_fwd_split_workspace_bytes(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l) != 0) return 0;
  const size_t tiles_m = ((size_t)N * Ho * Wo + GS_BM - 1) / GS_BM;
  return tiles_m * 4 * (size_t)Cout * sizeof(float);
}

int ladder_conv2d_fwd_split_bnstats(const void* x_planes, const float* x_absmax, const void* packed, const float* bias, float* y, int N, int H,
                                    int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int act,
                                    int prec, float* sums4, void* stats_ws, size_t stats_ws_bytes, ladder_stream_t stream) {
  const size_t need = ladder_conv2d_fwd_split_bnstats_workspace_bytes(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l);
  if (need == 0 || sums4 == nullptr) return LADDER_E_SHAPE;
  if (stats_ws == nullptr || stats_ws_bytes < need) return LADDER_E_WORKSPACE;
  const IgemmDesc d = conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, 1, pad_t, pad_l, act);
  const int rc = launch_fwd_split(x_planes, x_absmax, packed, bias, y, d, prec, nullptr, 0, stream, nullptr, 0, (float*)stats_ws);
  if (rc != LADDER_OK) return rc;
  return ladder_bn_stats_minmax_from_partials((const float*)stats_ws, (int)(((size_t)N * Ho * Wo + GS_BM - 1) / GS_BM), sums4, Cout, stream);
}

int ladder_conv2d_bwd_data_split_eligible(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t,
                                          int pad_l, int gated) {
  static const float dummy = 0.f;
  return conv2d_bwd_data_split_impl(nullptr, nullptr, nullptr, nullptr, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l,
                                    gated ? &dummy : nullptr, 0, LADDER_PREC_F16X3, nullptr, 0, nullptr, true, nullptr) == LADDER_OK ? 1 : 0;
}

size_t ladder_conv2d_bwd_data_split_workspace_bytes(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride,
                                                    int pad_t, int pad_l) {
  size_t need = 0;
  static const float dummy = 0.f;
  conv2d_bwd_data_split_impl(nullptr, nullptr, nullptr, nullptr, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l, &dummy, 0,
                             LADDER_PREC_F16X3, nullptr, 0, nullptr, true, &need);
  return need;
}

int ladder_conv2d_bwd_data_split(const void* dy_planes, const float* dy_absmax, const void* packed_T, float* dx, int N, int H, int W, int Cin,
                                 int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, const float* gate_y,
                                 int gate_act, int prec, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  return conv2d_bwd_data_split_impl(dy_planes, dy_absmax, packed_T, dx, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l, gate_y, gate_act,
                                    prec, ws, ws_bytes, stream, false, nullptr);
}

int ladder_conv2d_bwd_filter_split_eligible(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t,
                                            int pad_l) {
  if (!conv_shape_ok(N, H, W, Cin, Ho, Wo, KH, KW, stride)) return 0;
  const IgemmDesc d = conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, 1, pad_t, pad_l, 0);
  return (wgrad_split_ok(d) && !plan_wgrad_halo(d).ok) ? 1 : 0;
}

size_t ladder_conv2d_bwd_filter_split_workspace_bytes(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW) {
  return wgrad_split_ws_bytes(conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, 1, 1, 0, 0, 0));
}

int ladder_conv2d_bwd_filter_split(const void* x_planes, const float* x_absmax, const void* dy_planes, const float* dy_absmax, float* dw, float* db,
                                   int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l,
                                   int prec, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (!conv_shape_ok(N, H, W, Cin, Ho, Wo, KH, KW, stride)) return LADDER_E_SHAPE;
  return run_wgrad_split(x_planes, x_absmax, dy_planes, dy_absmax, dw, db, conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, 1, pad_t, pad_l, LADDER_ACT_NONE),
                         prec, ws, ws_bytes, stream);
}

}  // extern "C"
