// Convolution / dense kernels for gfx950 (MI355X), fp32 in / fp32 accumulate on the matrix cores
// (v_mfma_f32_32x32x2_f32: an exact fp32 FMA chain at the fp32 vector rate, 157.3 TFLOP/s peak).  This file: the forward family
// (igemm.h has the descriptor and the helpers; the filter gradients are igemm_wgrad.hip, the split-precision forms igemm_split.hip,
// the direct kernels for tiny channel counts convdirect.hip).
//
//   conv3x3_halo_kernel     3x3 / stride 1 / SAME forward and backward-data of large maps: 8x32-pixel x 128-channel tile,
//                           the input halo of each 16-channel slab staged once in LDS for all 9 taps (dominant kernel, ~134 TF).
//   igemm_fwd_kernel<...>   everything else that is forward-shaped (conv fwd / bwd_data of any size, stride, kernel; dense):
//                           C[M x N] = A_gather[M x K] * B[K x N], M = pixels, N = Cout, K = (tap, ci).  A is gathered on the
//                           fly from the NHWC input (no im2col buffer); B is the HWIO filter bank viewed as a row-major
//                           [K x Cout] matrix -- exactly the reference's checkpoint layout.  Tap table + per-row validity
//                           bitmask on the fast path, split-K when the grid cannot fill the chip, stride-2 backward-data
//                           decomposed into its four output-parity classes.
//
// Common structure: 16-deep K chunks staged through double-buffered LDS (global -> registers issued before the MFMA block of
// the current chunk, registers -> LDS after it, one barrier per chunk); NHWC keeps ci contiguous, so every global load is a
// 16-byte access; padding lanes read a 16-byte zero buffer so loads stay unconditional.
// The small tiles of igemm_fwd_kernel (64x64, 32x128) come in variants (ladder_*_variant, LADDER_IGEMM_VARIANT; profiles/gather_small_maps.md):
// on maps of at most 16 positions the rows run position-major and a tile walks only the chunks whose tap is inside the image for one of its
// rows (on by default); the global loads can run 1 ... 4 chunks ahead in as many register sets (default 1).  Every variant gives the same bits.
#include "igemm.h"

namespace {

// D: prefetch depth = register sets of global loads in flight (the loads of chunk j + D are issued before the MFMA block of chunk j;
// D = 1 is one chunk ahead).  SKIPPABLE: the instantiation can walk a compacted chunk list (`skip`: drop the chunks whose tap lies in
// the padding for every row of the tile) over position-major rows (`posmajor`: row m = (position m / N, image m % N)).
template <int BM, int BN, int WM, int WN, bool VECA, bool VECB, int D = 1, bool SKIPPABLE = false>
__global__ __launch_bounds__(kThreads, (BM * BN >= 128 * 128) ? IGEMM_FWD_MINW : IGEMM_MINW) void igemm_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, float* __restrict__ y,
                                                             const IgemmDesc d, const int tiles_n, const bool fast,
                                                             float* __restrict__ part, const int chunks_per_split,
                                                             const float* __restrict__ gate, const int gate_act,
                                                             float* __restrict__ stats_part, const bool skip, const bool posmajor,
                                                             const FastDiv div_n, const TapTab tt) {
  constexpr int LDA = BK + 1;  // odd row stride: conflict-free ds_read_b32 of A fragments
  constexpr int TM = BM / WM, TN = BN / WN, MI = TM / 32, NI = TN / 32;
  constexpr int A_UNITS = BM * (BK / 4), B_UNITS = BK * (BN / 4);
  constexpr int AU = (A_UNITS + kThreads - 1) / kThreads, BU = (B_UNITS + kThreads - 1) / kThreads;
  static_assert(WM * WN == 4, "4 wavefronts");
  __shared__ float As[2][BM * LDA];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK * BN];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int wm = wid / WN, wn = wid % WN;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;
  const int HoWo = d.Ho * d.Wo;

  // per-thread A rows (fixed for the whole K loop): base pointer of tap (0,0) and a bitmask of the taps that
  // fall inside the image, so the K loop only adds a wave-uniform tap offset and tests one bit.
  constexpr bool FASTA = VECA;          // needs KH*KW <= 32 and ups == 1 (checked by the launcher via `fast`)
  int a_row[AU], a_kq[AU], a_bh[AU], a_bw[AU];
  long a_img[AU];
  bool a_ok[AU];
  const float* a_ptr[AU];
  uint32_t a_mask[AU];
#pragma unroll
  for (int i = 0; i < AU; ++i) {
    const int u = tid + i * kThreads;
    a_row[i] = u / (BK / 4);
    a_kq[i] = u % (BK / 4);
    const int m = m0 + a_row[i];
    a_ok[i] = (u < A_UNITS) && (m < d.M);
    const uint32_t mm = a_ok[i] ? m : 0;
    uint32_t n_img = fdiv(mm, d.div_howo), rem = mm - n_img * HoWo;
    if (SKIPPABLE && posmajor) {   // all images of one output position together: a tile's rows share their padding taps
      rem = fdiv(mm, div_n);
      n_img = mm - rem * d.N;
    }
    const uint32_t ho = fdiv(rem, d.div_wo), wo = rem - ho * d.Wo;
    a_bh[i] = (int)ho * d.stride - d.pad_t;
    a_bw[i] = (int)wo * d.stride - d.pad_l;
    a_img[i] = (long)n_img * d.H * d.W * d.Cin;
    a_ptr[i] = x + a_img[i] + ((long)a_bh[i] * d.W + a_bw[i]) * d.Cin + a_kq[i] * 4;
    uint32_t msk = 0;
    if (FASTA && fast && a_ok[i]) {
      for (int t = 0; t < d.ntaps; ++t) {
        const int nh = a_bh[i] + (tt.dhw[t] >> 16), nw = a_bw[i] + (int)(short)(tt.dhw[t] & 0xffff);
        if (nh >= 0 && nh < d.H && nw >= 0 && nw < d.W) msk |= 1u << t;
      }
    }
    a_mask[i] = msk;
  }
  int b_kr[BU], b_nq[BU];
#pragma unroll
  for (int i = 0; i < BU; ++i) {
    const int u = tid + i * kThreads;
    b_kr[i] = u / (BN / 4);
    b_nq[i] = u % (BN / 4);
  }

  float4 ra[D][AU], rb[D][BU];     // (indexed by unrolled constants only)
  // the address of the zero buffer, taken once: left to itself the compiler fetches it again from the global offset table for every chunk,
  // a scalar load and a full wait in front of each chunk's loads
  typedef const float __attribute__((address_space(1)))* global_cptr;     // (kept a global-memory pointer: a flat load would count on both wait counters)
  global_cptr zero16_g = (global_cptr)g_zero16;
  asm volatile("" : "+s"(zero16_g));
  const float* zero16 = (const float*)zero16_g;
  // chunk c = tap t of channel slab `slab` on the fast path (c = slab * ntaps + t); t_coff / t_kbase = the tap's table entries
  auto load_chunk = [&](int c, int t, int slab, int t_coff, int t_kbase, float4 (&ra)[AU], float4 (&rb)[BU]) {
    // K order on the fast path: channel slab outer, taps inner -> the taps of one 16-channel slab re-read the same cache lines
    int k0 = c * BK;     // row of the [K x Cout] filter matrix this chunk starts at
    if (VECA) {  // Cin % BK == 0: the whole chunk lies inside one filter tap (wave-uniform tap, ci0)
      if (fast) {
        const int ci0 = slab * BK;
        k0 = t_kbase + ci0;
        const long coff = (long)t_coff + ci0;
#pragma unroll
        for (int i = 0; i < AU; ++i) ra[i] = ld4(((a_mask[i] >> t) & 1u) ? a_ptr[i] + coff : zero16);
      } else {
        const int rs = k0 / d.Cin, ci0 = k0 - rs * d.Cin;
        const int r = rs / d.KW, s = rs - r * d.KW;
#pragma unroll
        for (int i = 0; i < AU; ++i) {
          long off = a_ok[i] ? gather_off(d, a_img[i], a_bh[i], a_bw[i], r, s, ci0 + a_kq[i] * 4) : -1;
          ra[i] = ld4(off >= 0 ? x + off : zero16);
        }
      }
    } else {
#pragma unroll
      for (int i = 0; i < AU; ++i) {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + a_kq[i] * 4 + j;
          v[j] = 0.f;
          if (a_ok[i] && k < d.K) {
            const int rs = k / d.Cin, ci = k - rs * d.Cin;
            const int r = rs / d.KW, s = rs - r * d.KW;
            const long off = gather_off(d, a_img[i], a_bh[i], a_bw[i], r, s, ci);
            if (off >= 0) v[j] = x[off];
          }
        }
        ra[i] = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
#pragma unroll
    for (int i = 0; i < BU; ++i) {
      const int k = k0 + b_kr[i], n = n0 + b_nq[i] * 4;
      const bool inb = (tid + i * kThreads < B_UNITS) && k < d.KH * d.KW * d.Cin;
      if (VECB) {
        rb[i] = ld4((inb && n < d.Cout) ? w + (long)k * d.Cout + n : zero16);
      } else {
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (inb && n + j < d.Cout) ? w[(long)k * d.Cout + n + j] : 0.f;
        rb[i] = make_float4(v[0], v[1], v[2], v[3]);
      }
    }
  };
  auto store_chunk = [&](int buf, const float4 (&ra)[AU], const float4 (&rb)[BU]) {
#pragma unroll
    for (int i = 0; i < AU; ++i) {
      if (A_UNITS % kThreads == 0 || tid + i * kThreads < A_UNITS) {   // (a whole number of rounds: no branch, so the wait for the loads stands on every path)
        float* p = &As[buf][a_row[i] * LDA + a_kq[i] * 4];
        p[0] = ra[i].x; p[1] = ra[i].y; p[2] = ra[i].z; p[3] = ra[i].w;
      }
    }
#pragma unroll
    for (int i = 0; i < BU; ++i) {
      if (B_UNITS % kThreads == 0 || tid + i * kThreads < B_UNITS)
        *reinterpret_cast<float4*>(&Bs[buf][b_kr[i] * BN + b_nq[i] * 4]) = rb[i];
    }
  };

  f32x16 acc[MI][NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  // split-K: blockIdx.y owns the chunk range [c_begin, nchunks)
  const int c_begin = blockIdx.y * chunks_per_split;
  const int nchunks = min((d.K + BK - 1) / BK, c_begin + chunks_per_split);

  auto mma_chunk = [&](int buf) {
    const float* Ab = &As[buf][(wm * TM + l31) * LDA + lh];
    const float* Bb = &Bs[buf][lh * BN + wn * TN + l31];
    // all fragment reads of the chunk are issued before the MFMA block (one LDS round trip per chunk, not per k-step)
    float af[BK / 2][MI], bf[BK / 2][NI];
#pragma unroll
    for (int ks = 0; ks < BK / 2; ++ks) {
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) af[ks][mi] = Ab[mi * 32 * LDA + 2 * ks];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) bf[ks][ni] = Bb[2 * ks * BN + ni * 32];
    }
#pragma unroll
    for (int ks = 0; ks < BK / 2; ++ks)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[ks][mi], bf[ks][ni], acc[mi][ni], 0, 0, 0);
  };

  // the taps some row of this tile reads inside the image; a chunk of any other tap multiplies zeros and is not walked
  uint32_t tmask = 0xffffffffu;
  if (SKIPPABLE && FASTA && skip) {
    uint32_t wmask = 0;
    for (int t = 0; t < d.ntaps; ++t) {
      bool any = false;
#pragma unroll
      for (int i = 0; i < AU; ++i) any |= ((a_mask[i] >> t) & 1u) != 0;
      if (__ballot(any) != 0) wmask |= 1u << t;
    }
    uint32_t* wm4 = reinterpret_cast<uint32_t*>(&As[0][0]);
    if (lane == 0) wm4[wid] = wmask;
    __syncthreads();
    tmask = __builtin_amdgcn_readfirstlane(wm4[0] | wm4[1] | wm4[2] | wm4[3]);
    __syncthreads();
  }
  const bool walk = SKIPPABLE && FASTA && skip;
  // live chunks of [c_begin, nchunks): the pipeline below runs over this compacted list, split ranges keep the original numbering
  int nlive = nchunks - c_begin;
  // load cursor: the next chunk to fetch, its tap and channel slab, and the tap's table entries.  The entries come from 32-bit tables (a byte
  // of the descriptor indexed by the tap is a vector load, and waiting for it would drain every prefetch in flight), and the cursor moves
  // right after a chunk's loads are issued, so these scalar loads are back long before the next chunk needs them.
  int lc = c_begin, lt = 0, ls = 0, lcoff = 0, lkb = 0;
  if (VECA && fast) { ls = c_begin / d.ntaps; lt = c_begin - ls * d.ntaps; }
  if (walk) {
    const int pc = __popc(tmask), se = nchunks / d.ntaps, te = nchunks - se * d.ntaps;
    nlive = (se * pc + __popc(tmask & ((1u << te) - 1u))) - (ls * pc + __popc(tmask & ((1u << lt) - 1u)));
  }
  auto next_chunk = [&]() {
    do {
      ++lc;
      if (++lt == d.ntaps) { lt = 0; ++ls; }
    } while (walk && ((tmask >> lt) & 1u) == 0);
    if (VECA && fast) { lcoff = tt.coff[lt]; lkb = tt.kbase[lt]; }
  };
  // Every step issues its loads unconditionally (past the end it fetches the last chunk once more, into a register set nobody stores), and
  // the loop leaves through its one exit: the count of loads in flight is then the same on every path, and the wait before a
  // registers -> LDS store lets the D - 1 younger chunks stay in flight.
  if (nlive > 0) {
    if (walk && ((tmask >> lt) & 1u) == 0) next_chunk();
    else if (VECA && fast) { lcoff = tt.coff[lt]; lkb = tt.kbase[lt]; }
    // (the cursor stands at live chunk min(j + D, nlive - 1) when step j issues its loads)
#pragma unroll
    for (int r = 0; r < D; ++r) {
      load_chunk(lc, lt, ls, lcoff, lkb, ra[r], rb[r]);
      if (r + 1 < nlive) next_chunk();
    }
    store_chunk(0, ra[0], rb[0]);
    __syncthreads();
    for (int j0 = 0;; j0 += D) {
#pragma unroll
      for (int r = 0; r < D; ++r) {
        const int j = j0 + r;
        load_chunk(lc, lt, ls, lcoff, lkb, ra[r], rb[r]);
        if (j + D + 1 < nlive) next_chunk();
        mma_chunk(j & 1);
        if (j + 1 >= nlive) goto k_done;
        store_chunk((j + 1) & 1, ra[(r + 1) % D], rb[(r + 1) % D]);
        __syncthreads();
      }
    }
  }
k_done:

  if (part != nullptr) {   // split-K partial: raw accumulators, bias/activation applied by splitk_epilogue_kernel
    float* o = part + (size_t)blockIdx.y * d.M * d.Cout;
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int n = n0 + wn * TN + ni * 32 + l31;
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int m = m0 + wm * TM + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
          if (m < d.M && n < d.Cout) o[(long)m * d.Cout + n] = acc[mi][ni][e];
        }
    }
    return;
  }
  // epilogue: bias + activation, 128-byte row segments per half-wave
  const bool dense_out = d.out_sh == 1 && d.out_sw == 1 && d.OH == d.Ho && d.OW == d.Wo;
  // batch-norm statistics of what is written (128x128 tiles only; lane = output channel: the column sums are local):
  // stats_part [tile_m][4][Cout] = sum | sum of squares | min | max per tile, reduced by ladder_bn_stats_minmax_from_partials
  constexpr bool STATS = (BM == 128 && BN == 128 && WM == 2);
  float st0[NI], st1[NI], smn[NI], smx[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) { st0[ni] = 0.f; st1[ni] = 0.f; smn[ni] = INFINITY; smx[ni] = -INFINITY; }
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int n = n0 + wn * TN + ni * 32 + l31;
    const float bv = (bias != nullptr && n < d.Cout) ? bias[n] : 0.f;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + wm * TM + mi * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (m < d.M && n < d.Cout) {
          long row = m;
          if (!dense_out || (SKIPPABLE && posmajor)) {   // phased backward-data: the M space is one parity class of the output map
            uint32_t n_img = fdiv((uint32_t)m, d.div_howo), rem = (uint32_t)m - n_img * HoWo;
            if (SKIPPABLE && posmajor) {
              rem = fdiv((uint32_t)m, div_n);
              n_img = (uint32_t)m - rem * d.N;
            }
            const uint32_t ho = fdiv(rem, d.div_wo), wo = rem - ho * d.Wo;
            row = ((long)n_img * d.OH + d.out_h0 + (long)ho * d.out_sh) * d.OW + d.out_w0 + (long)wo * d.out_sw;
          }
          float v = ladder_act_fn(acc[mi][ni][e] + bv, d.act);
          // optional gate: multiply by act'(gate) evaluated from the producer layer's activation OUTPUT at the same element
          // (fuses the previous layer's activation backward into this backward-data pass)
          if (gate != nullptr) v *= ladder_act_grad_from_out(gate[row * d.Cout + n], gate_act);
          y[row * d.Cout + n] = v;
          if (STATS && stats_part != nullptr) {        // (wave-uniform: a plain forward / backward-data launch carries no statistics work -- ADVICE r4)
            st0[ni] += v;
            st1[ni] += v * v;
            smn[ni] = fminf(smn[ni], v);
            smx[ni] = fmaxf(smx[ni], v);
          }
        }
      }
    }
  }
  if (STATS && stats_part != nullptr) {
    float* sred = &Bs[0][0];                                 // [which 4][wm 2][128 channels] (the operand tiles are dead)
    __syncthreads();
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const float a0 = st0[ni] + __shfl_xor(st0[ni], 32, 64), a1 = st1[ni] + __shfl_xor(st1[ni], 32, 64);
      const float a2 = fminf(smn[ni], __shfl_xor(smn[ni], 32, 64)), a3 = fmaxf(smx[ni], __shfl_xor(smx[ni], 32, 64));
      if (lh == 0) {
        const int cc = wn * TN + ni * 32 + l31;
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

__global__ void splitk_epilogue_kernel(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ y,
                                       int S, size_t MN, int N, int act, const float* __restrict__ gate, int gate_act) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= MN) return;
  float s = 0.f;
  for (int z = 0; z < S; ++z) s += part[(size_t)z * MN + i];   // fixed order
  if (bias != nullptr) s += bias[i % N];
  s = ladder_act_fn(s, act);
  if (gate != nullptr) s *= ladder_act_grad_from_out(gate[i], gate_act);
  y[i] = s;
}

// The same second pass for a call whose M space is a strided subset of the output map (one parity class of a stride-2 backward-data):
// partials are dense in the class-local pixel index m, the result goes to y[n, out_h0 + ho*out_sh, out_w0 + wo*out_sw, :].
__global__ void splitk_epilogue_strided_kernel(const float* __restrict__ part, const float* __restrict__ bias, float* __restrict__ y,
                                               int S, size_t MN, int act, const float* __restrict__ gate, int gate_act, const IgemmDesc d,
                                               const bool posmajor, const FastDiv div_n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= MN) return;
  float s = 0.f;
  for (int z = 0; z < S; ++z) s += part[(size_t)z * MN + i];   // fixed order
  const uint32_t m = (uint32_t)(i / d.Cout), n = (uint32_t)(i - (size_t)m * d.Cout);
  uint32_t n_img = fdiv(m, d.div_howo), rem = m - n_img * (uint32_t)(d.Ho * d.Wo);
  if (posmajor) {   // the partials keep the first pass's row order: row m = (position m / N, image m % N)
    rem = fdiv(m, div_n);
    n_img = m - rem * (uint32_t)d.N;
  }
  const uint32_t ho = fdiv(rem, d.div_wo), wo = rem - ho * d.Wo;
  const size_t o = ((((size_t)n_img * d.OH + d.out_h0 + (size_t)ho * d.out_sh) * d.OW + d.out_w0 + (size_t)wo * d.out_sw)) * d.Cout + n;
  if (bias != nullptr) s += bias[n];
  s = ladder_act_fn(s, act);
  if (gate != nullptr) s *= ladder_act_grad_from_out(gate[o], gate_act);
  y[o] = s;
}

__global__ void flip_transpose_kernel(const float* __restrict__ w, float* __restrict__ wT, int KH, int KW, int Cin, int Cout) {
  // wT[KH-1-r][KW-1-s][co][ci] = w[r][s][ci][co]; 32x32 LDS tile transpose per tap
  __shared__ float t[32][33];
  const int tap = blockIdx.z, r = tap / KW, s = tap % KW;
  const int ci0 = blockIdx.y * 32, co0 = blockIdx.x * 32;
  const float* src = w + (size_t)tap * Cin * Cout;
  float* dst = wT + (size_t)((KH - 1 - r) * KW + (KW - 1 - s)) * Cin * Cout;
  for (int i = threadIdx.y; i < 32; i += blockDim.y) {
    const int ci = ci0 + i, co = co0 + threadIdx.x;
    t[i][threadIdx.x] = (ci < Cin && co < Cout) ? src[(size_t)ci * Cout + co] : 0.f;
  }
  __syncthreads();
  for (int i = threadIdx.y; i < 32; i += blockDim.y) {
    const int co = co0 + i, ci = ci0 + threadIdx.x;
    if (co < Cout && ci < Cin) dst[(size_t)co * Cin + ci] = t[threadIdx.x][i];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// 3x3 / stride 1 / SAME convolution with an LDS-staged INPUT HALO tile (the decoder's dominant layers and their
// backward-data passes).  One workgroup = 8 wavefronts = an 8x32-pixel output patch x 128 output channels.
// For every 16-channel input slab the (8+2)x(32+2) halo patch is fetched from HBM/L2 ONCE and serves all 9 filter
// taps straight out of LDS (the gather kernel above re-fetches it per tap); the filter slab [16 x 128] of each tap is
// double-buffered.  Per 9 K-chunks a thread issues 12 global loads instead of 36, and the 256-pixel patch halves the
// filter bytes per MFMA.  Wavefront (wm, wn) owns patch rows {2wm, 2wm+1} x channels [64wn, 64wn+64): an MFMA A
// fragment is 32 consecutive pixels of one patch row, i.e. consecutive LDS rows of odd stride 17 -> conflict-free.
constexpr int HT_H = 8, HT_W = 32, HT_PW = HT_W + 2, HT_PH = HT_H + 2, HT_LDA = BK + 1;
constexpr int HT_THREADS = 512, HT_BN = 128;
constexpr int HT_HALO_UNITS = HT_PH * HT_PW * (BK / 4);                      // float4 units per slab (1360)
constexpr int HT_AU = (HT_HALO_UNITS + HT_THREADS - 1) / HT_THREADS;         // 3

__global__ __launch_bounds__(HT_THREADS, 2) void conv3x3_halo_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, float* __restrict__ y,
                                                                     const int N, const int H, const int W, const int Cin,
                                                                     const int Cout, const int act, const int tiles_n) {
  static_assert(BK == 16, "halo kernel is written for 16-channel slabs");
  __shared__ float Ah[2][HT_PH * HT_PW * HT_LDA];
  __shared__ __attribute__((aligned(16))) float Bh[2][BK * HT_BN];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  const int l31 = lane & 31, lh = lane >> 5;
  const int wm = wid >> 1, wn = wid & 1;
  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = tile / tiles_n, n0 = (tile % tiles_n) * HT_BN;
  const int tw_n = W / HT_W, th_n = H / HT_H;
  const int img = mt / (tw_n * th_n), rem = mt - img * (tw_n * th_n);
  const int h0 = (rem / tw_n) * HT_H, w0 = (rem % tw_n) * HT_W;

  // halo load units (fixed per workgroup): source pointer at channel 0 of the slab, or the zero buffer
  const float* hsrc[HT_AU];
  int hdst[HT_AU];
#pragma unroll
  for (int i = 0; i < HT_AU; ++i) {
    const int u = tid + i * HT_THREADS;
    const int pix = u >> 2, kq = u & 3;
    const int hr = pix / HT_PW, hc = pix - hr * HT_PW;
    const int hi = h0 - 1 + hr, wi = w0 - 1 + hc;
    const bool ok = (u < HT_HALO_UNITS) && hi >= 0 && hi < H && wi >= 0 && wi < W;
    hsrc[i] = ok ? x + (((long)img * H + hi) * W + wi) * Cin + kq * 4 : nullptr;
    hdst[i] = pix * HT_LDA + kq * 4;
  }
  const int b_kr = tid >> 5, b_nq = tid & 31;                                // 16 rows x 32 float4 = 512 units
  const bool b_ok = (n0 + b_nq * 4) < Cout;
  const float* bsrc = w + (long)b_kr * Cout + n0 + b_nq * 4;

  f32x16 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[mi][ni][e] = 0.f;

  float4 ha[HT_AU], rb;
  auto load_halo = [&](int slab) {
#pragma unroll
    for (int i = 0; i < HT_AU; ++i) ha[i] = ld4(hsrc[i] != nullptr ? hsrc[i] + slab * BK : g_zero16);
  };
  auto store_halo = [&](int buf) {
#pragma unroll
    for (int i = 0; i < HT_AU; ++i)
      if (tid + i * HT_THREADS < HT_HALO_UNITS) {
        float* p = &Ah[buf][hdst[i]];
        p[0] = ha[i].x; p[1] = ha[i].y; p[2] = ha[i].z; p[3] = ha[i].w;
      }
  };
  auto load_b = [&](int slab, int tap) { rb = ld4(b_ok ? bsrc + ((long)tap * Cin + slab * BK) * Cout : g_zero16); };
  auto store_b = [&](int buf) { *reinterpret_cast<float4*>(&Bh[buf][b_kr * HT_BN + b_nq * 4]) = rb; };

  const int nslabs = Cin / BK;
  load_halo(0);
  load_b(0, 0);
  store_halo(0);
  store_b(0);
  __syncthreads();
  int bbuf = 0;
  for (int slab = 0; slab < nslabs; ++slab) {
    const int hb = slab & 1;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      // prefetch: next filter slab every tap; next input halo once per slab (issued at tap 0, written at tap 4)
      const bool last = (slab + 1 == nslabs) && (tap == 8);
      if (!last) load_b(tap == 8 ? slab + 1 : slab, tap == 8 ? 0 : tap + 1);
      if (tap == 0 && slab + 1 < nslabs) load_halo(slab + 1);
      const int r = tap / 3, sft = tap - 3 * r;
      const float* Ab = &Ah[hb][((2 * wm + r) * HT_PW + sft + l31) * HT_LDA + lh];
      const float* Bb = &Bh[bbuf][lh * HT_BN + wn * 64 + l31];
#pragma unroll
      for (int ks = 0; ks < BK / 2; ++ks) {
        float a[2], b[2];
        a[0] = Ab[2 * ks];
        a[1] = Ab[HT_PW * HT_LDA + 2 * ks];
        b[0] = Bb[2 * ks * HT_BN];
        b[1] = Bb[2 * ks * HT_BN + 32];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
          for (int ni = 0; ni < 2; ++ni)
            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
      }
      if (tap == 4 && slab + 1 < nslabs) store_halo(hb ^ 1);
      if (!last) store_b(bbuf ^ 1);
      __syncthreads();
      bbuf ^= 1;
    }
  }

#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int n = n0 + wn * 64 + ni * 32 + l31;
    const float bv = (bias != nullptr && n < Cout) ? bias[n] : 0.f;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const long rowbase = (((long)img * H + h0 + 2 * wm + mi) * W + w0) * Cout;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int px = (e & 3) + 8 * (e >> 2) + 4 * lh;
        if (n < Cout) y[rowbase + (long)px * Cout + n] = ladder_act_fn(acc[mi][ni][e] + bv, act);
      }
    }
  }
}

}  // namespace

bool halo_eligible(const IgemmDesc& d) {
  if (halo_disabled()) return false;
#if IGEMM_HALO
  return d.KH == 3 && d.KW == 3 && d.stride == 1 && d.ups == 1 && d.pad_t == 1 && d.pad_l == 1 && d.Ho == d.H && d.Wo == d.W &&
         (d.Cin % BK) == 0 && (d.Cout % 4) == 0 && (d.W % HT_W) == 0 && (d.H % HT_H) == 0 && d.Cout >= 64 &&
         (long)d.N * (d.H / HT_H) * (d.W / HT_W) * ((d.Cout + HT_BN - 1) / HT_BN) >= 512;
#else
  return false;
#endif
}

static int launch_halo(const float* x, const float* w, const float* bias, float* y, const IgemmDesc& d, hipStream_t st) {
  const int tiles_n = (d.Cout + HT_BN - 1) / HT_BN;
  const int tiles_m = d.N * (d.H / HT_H) * (d.W / HT_W);
  hipLaunchKernelGGL(conv3x3_halo_kernel, dim3(tiles_m * tiles_n), dim3(HT_THREADS), 0, st, x, w, bias, y, d.N, d.H, d.W, d.Cin,
                     d.Cout, d.act, tiles_n);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

// split-K only when the output tiling cannot fill the chip and K is long enough to amortise the second pass
SplitPlan plan_splitk(long M, int K, int Cout, int bm, int bn) {
  const long tiles = ((M + bm - 1) / bm) * ((Cout + bn - 1) / bn);
  const int nchunks = (K + BK - 1) / BK;
  SplitPlan p{1, nchunks};
  if (tiles >= 640 || nchunks < 16) return p;
  long s = tiles < 128 ? (384 + tiles - 1) / tiles : 1024 / tiles;   // small grids: >=1.5 wg/CU; mid grids: one full round of 4 wg/CU
  if (s > nchunks / 8) s = nchunks / 8;
  if (tiles < 128 && s < nchunks / 4 && s * tiles < 256) s = nchunks / 4;
  if (s > 32) s = 32;
  if (s < 2) return p;
  p.cps = (int)((nchunks + s - 1) / s);
  p.splits = (nchunks + p.cps - 1) / p.cps;
  return p;
}

void launch_splitk_epilogue(const float* part, const float* bias, float* y, int splits, const IgemmDesc& d, const float* gate, int gate_act,
                            hipStream_t st, bool posmajor) {
  const size_t mn = (size_t)d.M * d.Cout;
  if (!posmajor && d.out_sh == 1 && d.out_sw == 1 && d.OH == d.Ho && d.OW == d.Wo)
    hipLaunchKernelGGL(splitk_epilogue_kernel, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, st, part, bias, y, splits, mn, d.Cout, d.act,
                       gate, gate_act);
  else
    hipLaunchKernelGGL(splitk_epilogue_strided_kernel, dim3((unsigned)((mn + 255) / 256)), dim3(256), 0, st, part, bias, y, splits, mn, d.act,
                       gate, gate_act, d, posmajor, make_fastdiv((uint32_t)d.N));
}

// Small maps (at most 16 output positions, more than one tap): a tile of the small-tile kernels walks only the chunks whose tap is inside the
// image for one of its rows; with at least a tile of images the rows run position-major, so a tile's rows share their padding taps.
// Geometry only, never data.  (variant bit 0)
struct SmallMapMode { bool skip, posmajor; };
static SmallMapMode small_map_mode(const IgemmDesc& d, int bm, int bn, int variant) {
  const bool small_tile = (bm == 64 && bn == 64) || (bm == 32 && bn == 128);
  const bool skip = (variant & 1) != 0 && small_tile && (d.Cin % BK) == 0 && d.ntaps > 1 && d.Ho * d.Wo <= 16;
  return SmallMapMode{skip, skip && d.N >= bm};
}

int igemm_default_variant() {
  static const int variant = getenv("LADDER_IGEMM_VARIANT") != nullptr ? atoi(getenv("LADDER_IGEMM_VARIANT")) & 7 : IGEMM_VARIANT_DEFAULT;
  return variant;
}

struct FwdArgs {
  const float *x, *w, *bias;
  float* y;
  const IgemmDesc& d;
  int tiles_n;
  bool fast;
  float* part;
  int cps;
  const float* gate;
  int gate_act;
  float* stats_part;
  SmallMapMode mode;
};

template <int BM, int BN, int WM, int WN, int D, bool SK>
static void launch_fwd_vec(dim3 grid, hipStream_t st, const FwdArgs& a) {
  const bool veca = (a.d.Cin % BK) == 0, vecb = (a.d.Cout % 4) == 0;
  const FastDiv div_n = make_fastdiv((uint32_t)a.d.N);
  const TapTab tt = make_taptab(a.d);
  const dim3 block(kThreads);
#define LADDER_FWD_GO(VA, VB)                                                                                                                  \
  hipLaunchKernelGGL((igemm_fwd_kernel<BM, BN, WM, WN, VA, VB, D, SK>), grid, block, 0, st, a.x, a.w, a.bias, a.y, a.d, a.tiles_n, a.fast, a.part, \
                     a.cps, a.gate, a.gate_act, a.stats_part, a.mode.skip, a.mode.posmajor, div_n, tt)
  if (veca && vecb) LADDER_FWD_GO(true, true);
  else if (veca) LADDER_FWD_GO(true, false);
  else if (vecb) LADDER_FWD_GO(false, true);
  else LADDER_FWD_GO(false, false);
#undef LADDER_FWD_GO
}

template <int BM, int BN, int WM, int WN>
static int launch_fwd(const float* x, const float* w, const float* bias, float* y, const IgemmDesc& d, void* ws, size_t ws_bytes,
               hipStream_t st, const float* gate = nullptr, int gate_act = 0, float* stats_part = nullptr, int variant = 0) {
  const int tiles_m = (d.M + BM - 1) / BM, tiles_n = (d.Cout + BN - 1) / BN;
  const bool fast = d.ntaps > 0;
  const bool dense_out = d.out_sh == 1 && d.out_sw == 1 && d.OH == d.Ho && d.OW == d.Wo;
  // (round 4: also the parity classes of a stride-2 backward-data -- a quarter of the pixels, 1 ... 4 of the 9 taps: 32 tiles on 256 CUs
  // for the 8x8 <- 4x4 layer -- through splitk_epilogue_strided_kernel: 241 -> 96 us for its four launches)
  // (only the small ones: at 512 tiles the strided second pass costs more than the idle CUs -- 16x16 <- 8x8: 174 us single pass, 195 split)
  SplitPlan sp = (dense_out || (long)tiles_m * tiles_n <= 256) ? plan_splitk(d.M, d.K, d.Cout, BM, BN) : SplitPlan{1, (d.K + BK - 1) / BK};
  const size_t need = (size_t)sp.splits * d.M * d.Cout * sizeof(float);
  if (sp.splits > 1 && (ws == nullptr || ws_bytes < need)) sp = SplitPlan{1, (d.K + BK - 1) / BK};
  float* part = sp.splits > 1 ? (float*)ws : nullptr;
  if (stats_part != nullptr && (part != nullptr || !dense_out || BM != 128 || BN != 128)) return LADDER_E_SHAPE;   // statistics come from the single-pass 128x128 epilogue
  const dim3 grid(tiles_m * tiles_n, sp.splits);
  const FwdArgs a{x, w, bias, y, d, tiles_n, fast, part, sp.cps, part ? nullptr : gate, gate_act, stats_part, small_map_mode(d, BM, BN, variant)};
  // the prefetch depth (variant bits 1-2) exists for the small tiles; the large ones stay one chunk ahead
  constexpr bool SMALL = (BM == 64 && BN == 64) || (BM == 32 && BN == 128);
  if constexpr (SMALL) {
    switch ((variant >> 1) & 3) {
      case 0: launch_fwd_vec<BM, BN, WM, WN, 1, true>(grid, st, a); break;
      case 1: launch_fwd_vec<BM, BN, WM, WN, 2, true>(grid, st, a); break;
      case 2: launch_fwd_vec<BM, BN, WM, WN, 3, true>(grid, st, a); break;
      default: launch_fwd_vec<BM, BN, WM, WN, 4, true>(grid, st, a); break;
    }
  } else {
    launch_fwd_vec<BM, BN, WM, WN, 1, false>(grid, st, a);
  }
  if (part != nullptr) launch_splitk_epilogue(part, bias, y, sp.splits, d, gate, gate_act, st, a.mode.posmajor);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

// tile selection: BM*1000 + BN
int select_fwd_tile(long M, int Cout) {
  const long big_tiles = ((M + 127) / 128) * ((Cout + 127) / 128);
  if (Cout > 64) {
    if (big_tiles >= 192) return 128128;
    if (M > 32) return 64064;
    return 32128;
  }
  if (Cout > 32) return ((M + 127) / 128 >= 192) ? 128064 : 64064;
  return 128032;
}

int dispatch_fwd(const float* x, const float* w, const float* bias, float* y, const IgemmDesc& d, void* ws, size_t ws_bytes,
                 hipStream_t st, const float* gate, int gate_act, int variant) {
  if (d.M <= 0 || d.K <= 0 || d.Cout <= 0) return LADDER_E_SHAPE;
  if (!ladder_aligned16(x) || !ladder_aligned16(w) || !ladder_aligned16(y)) return LADDER_E_ALIGN;
  if (gate == nullptr && halo_eligible(d)) return launch_halo(x, w, bias, y, d, st);
  switch (select_fwd_tile(d.M, d.Cout)) {
    case 128128: return launch_fwd<128, 128, 2, 2>(x, w, bias, y, d, ws, ws_bytes, st, gate, gate_act, nullptr, variant);
    case 64064: return launch_fwd<64, 64, 2, 2>(x, w, bias, y, d, ws, ws_bytes, st, gate, gate_act, nullptr, variant);
    case 32128: return launch_fwd<32, 128, 1, 4>(x, w, bias, y, d, ws, ws_bytes, st, gate, gate_act, nullptr, variant);
    case 128064: return launch_fwd<128, 64, 4, 1>(x, w, bias, y, d, ws, ws_bytes, st, gate, gate_act, nullptr, variant);
    default: return launch_fwd<128, 32, 4, 1>(x, w, bias, y, d, ws, ws_bytes, st, gate, gate_act, nullptr, variant);
  }
}

int dispatch_fwd(const float* x, const float* w, const float* bias, float* y, const IgemmDesc& d, void* ws, size_t ws_bytes,
                 hipStream_t st, const float* gate, int gate_act) {
  return dispatch_fwd(x, w, bias, y, d, ws, ws_bytes, st, gate, gate_act, igemm_default_variant());
}

static size_t fwd_ws_bytes(long M, int K, int Cout) {
  const int t = select_fwd_tile(M, Cout);
  const SplitPlan sp = plan_splitk(M, K, Cout, t / 1000, t % 1000);
  size_t need = sp.splits > 1 ? (size_t)sp.splits * M * Cout * sizeof(float) : 0;
  // the call may be a stride-2 backward-data: its parity classes (a quarter of the pixels, at most 4 of 9 taps) split on their own
  if ((K % 9) == 0 && M >= 4) {
    const long Mc = (M + 3) / 4;
    const int Kc = K / 9 * 4, tc = select_fwd_tile(Mc, Cout);
    const SplitPlan sc = plan_splitk(Mc, Kc, Cout, tc / 1000, tc % 1000);
    const size_t nc = sc.splits > 1 ? (size_t)sc.splits * Mc * Cout * sizeof(float) : 0;
    if (nc > need) need = nc;
  }
  return need;
}

extern "C" {

int ladder_abi_version(void) { return 2; }   // == LADDER_ABI_VERSION (include/ladder_hip.h)

int ladder_dense_fwd_is_persistent(long M, int K, int N) { return dense_f32_big_ok(M, K, N) ? 1 : 0; }
int ladder_dense_bwd_weight_is_persistent(long M, int K, int N) { return dense_wgrad_f32_ok(M, K, N) ? 1 : 0; }

int ladder_igemm_fwd_tile(long M, int Cin, int Cout) {
  // BM*1000+BN of the kernel instantiation ladder_conv2d_fwd / _bwd_data / ladder_dense_* dispatch to; negative when the
  // vectorised (Cin%16==0 && Cout%4==0) instantiation is not used.  Lets a profiler attribute a launch to a kernel name.
  const int t = select_fwd_tile(M, Cout);
  return ((Cin % BK) == 0 && (Cout % 4) == 0) ? t : -t;   // (the 3x3 halo kernel is reported by ladder_conv3x3_uses_halo)
}

// The *_variant entry points run one form of igemm_fwd_kernel (bit 0: position-major rows and padding-tap skipping on small maps; bits 1-2:
// prefetch depth - 1); every variant gives the same bits, variant 0 is the first form of the kernel.  The plain entry points run
// IGEMM_VARIANT_DEFAULT, or LADDER_IGEMM_VARIANT (read once) for whole-process comparisons.
int ladder_conv2d_fwd_variant(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin,
                              int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int act,
                              void* ws, size_t ws_bytes, int variant, ladder_stream_t stream) {
  if (variant < 0 || variant > 7) return LADDER_E_SHAPE;
  if (!conv_shape_ok(N, H, W, Cin, Ho, Wo, KH, KW, stride)) return LADDER_E_SHAPE;
  if (smallcout_eligible(Cin, Cout, KH, KW, stride, (long)N * Ho * Wo) && ladder_aligned16(x)) {
    const int M = N * Ho * Wo;
    launch_smallcout(x, w, bias, y, nullptr, nullptr, nullptr, Cin, Cout, act, M, nullptr, 0, smallcout_blocks(M, Cin), stream);
    LADDER_CHECK_LAUNCH();
    return LADDER_OK;
  }
  if (cout1_eligible(Cin, Cout, KH, KW, stride, pad_t, pad_l, H, W, Ho, Wo)) {
    launch_cout1(x, w, bias, y, nullptr, nullptr, nullptr, nullptr, N, H, W, Cin, Ho, Wo, act, stream);
    LADDER_CHECK_LAUNCH();
    return LADDER_OK;
  }
  return dispatch_fwd(x, w, bias, y, conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, 1, pad_t, pad_l, act), ws, ws_bytes, stream, nullptr, 0, variant);
}

int ladder_conv2d_fwd(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin,
                      int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int act,
                      void* ws, size_t ws_bytes, ladder_stream_t stream) {
  return ladder_conv2d_fwd_variant(x, w, bias, y, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l, act, ws, ws_bytes, igemm_default_variant(), stream);
}

size_t ladder_igemm_fwd_workspace_bytes(long M, int K, int Cout) { return fwd_ws_bytes(M, K, Cout); }

int ladder_igemm_fwd_splits(long M, int K, int Cout) {
  const int t = select_fwd_tile(M, Cout);
  return plan_splitk(M, K, Cout, t / 1000, t % 1000).splits;
}

// ---- strict-fp32 convolution whose epilogue also emits the batch-norm statistics of its output (round 4: the fp32 form of
// ladder_conv2d_fwd_split_bnstats): 128x128-tile gather launches without split-K.  0 bytes = not available for this geometry.
static bool fwd_bnstats_ok(const IgemmDesc& d) {
  if (getenv("LADDER_DISABLE_BNSTATS") != nullptr) return false;       // (test-only switch: the statistics then come from the separate pass)
  // (Cin % 16: the image-side conv, Cin = 3, is bound by writing its output -- the statistics epilogue costs it the 90 us the separate pass takes: measured, no gain)
  return (d.Cin % BK) == 0 && (d.Cout % 4) == 0 && d.ntaps > 0 && !halo_eligible(d) && select_fwd_tile(d.M, d.Cout) == 128128 &&
         plan_splitk(d.M, d.K, d.Cout, 128, 128).splits == 1 && !smallcout_eligible(d.Cin, d.Cout, d.KH, d.KW, d.stride, d.M);
}

size_t ladder_conv2d_fwd_bnstats_workspace_bytes(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t,
                                                 int pad_l) {
  if (!conv_shape_ok(N, H, W, Cin, Ho, Wo, KH, KW, stride)) return 0;
  const IgemmDesc d = conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, 1, pad_t, pad_l, 0);
  if (!fwd_bnstats_ok(d)) return 0;
  return (((size_t)d.M + 127) / 128) * 4 * (size_t)Cout * sizeof(float);
}

int ladder_conv2d_fwd_bnstats(const float* x, const float* w, const float* bias, float* y, int N, int H, int W, int Cin, int Ho, int Wo, int Cout,
                              int KH, int KW, int stride, int pad_t, int pad_l, int act, float* sums4, void* stats_ws, size_t stats_ws_bytes,
                              ladder_stream_t stream) {
  const size_t need = ladder_conv2d_fwd_bnstats_workspace_bytes(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l);
  if (need == 0 || sums4 == nullptr) return LADDER_E_SHAPE;
  if (stats_ws == nullptr || stats_ws_bytes < need) return LADDER_E_WORKSPACE;
  if (!ladder_aligned16(x) || !ladder_aligned16(w) || !ladder_aligned16(y)) return LADDER_E_ALIGN;
  const IgemmDesc d = conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, 1, pad_t, pad_l, act);
  const int rc = launch_fwd<128, 128, 2, 2>(x, w, bias, y, d, nullptr, 0, stream, nullptr, 0, (float*)stats_ws);
  if (rc != LADDER_OK) return rc;
  return ladder_bn_stats_minmax_from_partials((const float*)stats_ws, (int)(((size_t)d.M + 127) / 128), sums4, Cout, stream);
}

int ladder_conv2d_fwd_kernel_id(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int ups,
                                int pad_t, int pad_l) {
  // 256128 = conv3x3_halo_kernel (8x32-pixel x 128-channel LDS-halo tile); otherwise the code of ladder_igemm_fwd_tile
  const IgemmDesc d = conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, ups, pad_t, pad_l, 0);
  if (halo_eligible(d)) return 256128;
  if (ups == 1 && stride == 1 && smallcin_eligible(Cin, Cout, KH, KW)) return 9003;     // conv_smallcin_kernel (direct, output-write bound)
  return ladder_igemm_fwd_tile(d.M, Cin, Cout);
}

int ladder_filter_flip_transpose(const float* w, float* wT, int KH, int KW, int Cin, int Cout, ladder_stream_t stream) {
  if (KH <= 0 || KW <= 0 || Cin <= 0 || Cout <= 0) return LADDER_E_SHAPE;
  dim3 grid((Cout + 31) / 32, (Cin + 31) / 32, KH * KW), block(32, 8);
  hipLaunchKernelGGL(flip_transpose_kernel, grid, block, 0, stream, w, wT, KH, KW, Cin, Cout);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_conv2d_bwd_data_variant(const float* dy, const float* wT, float* dx, int N, int H, int W, int Cin, int Ho, int Wo,
                                   int Cout, int KH, int KW, int stride, int pad_t, int pad_l, const float* gate_y, int gate_act,
                                   void* ws, size_t ws_bytes, int variant, ladder_stream_t stream) {
  if (variant < 0 || variant > 7) return LADDER_E_SHAPE;
  if (!conv_shape_ok(N, H, W, Cin, Ho, Wo, KH, KW, stride)) return LADDER_E_SHAPE;
  const IgemmDesc d = bwd_data_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l);
  if (stride == 1 && smallcin_eligible(Cout, Cin, KH, KW))             // 1x1 from a 3-channel dy (CelebA output conv), gate fused
    return launch_smallcin(dy, wT, nullptr, dx, gate_y, N, Ho, Wo, Cout, H, W, Cin, KH, 1, 0, 0, gate_y != nullptr ? gate_act : 0, stream);
  if (stride == 1) return dispatch_fwd(dy, wT, nullptr, dx, d, ws, ws_bytes, stream, gate_y, gate_act, variant);
  if (stride == 2 && (Cout % BK) == 0 && KH * KW <= 28) {
    IgemmDesc cls[4];
    parity_classes(d, cls);
    for (const IgemmDesc& c : cls) {
      if (c.M == 0) continue;
      if (c.ntaps == 0) return dispatch_fwd(dy, wT, nullptr, dx, d, ws, ws_bytes, stream, gate_y, gate_act, variant);   // degenerate: legacy path writes the zeros
      const int rc = dispatch_fwd(dy, wT, nullptr, dx, c, ws, ws_bytes, stream, gate_y, gate_act, variant);   // (the classes run one after another: one workspace)
      if (rc != LADDER_OK) return rc;
    }
    return LADDER_OK;
  }
  return dispatch_fwd(dy, wT, nullptr, dx, d, ws, ws_bytes, stream, gate_y, gate_act, variant);   // generic strided gather (ups > 1)
}

int ladder_conv2d_bwd_data(const float* dy, const float* wT, float* dx, int N, int H, int W, int Cin, int Ho, int Wo,
                           int Cout, int KH, int KW, int stride, int pad_t, int pad_l, const float* gate_y, int gate_act,
                           void* ws, size_t ws_bytes, ladder_stream_t stream) {
  return ladder_conv2d_bwd_data_variant(dy, wT, dx, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l, gate_y, gate_act, ws, ws_bytes,
                                        igemm_default_variant(), stream);
}

int ladder_dense_fwd_variant(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int act,
                             void* ws, size_t ws_bytes, int variant, ladder_stream_t stream) {
  if (variant < 0 || variant > 7) return LADDER_E_SHAPE;
  if (dense_f32_big_ok(M, K, N)) return dense_f32_big_launch(x, w, bias, y, nullptr, 0, M, K, N, act, stream);     // (csrc/densef32.hip)
  return dispatch_fwd(x, w, bias, y, dense_desc(M, K, N, act), ws, ws_bytes, stream, nullptr, 0, variant);
}

int ladder_dense_fwd(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, int act,
                     void* ws, size_t ws_bytes, ladder_stream_t stream) {
  return ladder_dense_fwd_variant(x, w, bias, y, M, K, N, act, ws, ws_bytes, igemm_default_variant(), stream);
}

// Chunks (16-deep K steps of one output tile) that the gather kernel issues for a convolution forward (bwd_data == 0) or its backward-data
// (bwd_data != 0, same geometry arguments as ladder_conv2d_bwd_data), summed over all tiles and launches, under `variant` (-1: the default).
// variant 0 gives the chunks of the full tap walk.  -1 when the call does not run igemm_fwd_kernel.  Pure host arithmetic.
static long desc_live_chunks(const IgemmDesc& d, int variant) {
  const int t = select_fwd_tile(d.M, d.Cout), bm = t / 1000, bn = t % 1000;
  const long tiles_m = (d.M + bm - 1) / bm, tiles_n = (d.Cout + bn - 1) / bn;
  const int nchunks = (d.K + BK - 1) / BK;
  const SmallMapMode mode = small_map_mode(d, bm, bn, variant);
  if (!mode.skip) return tiles_m * tiles_n * nchunks;
  const int howo = d.Ho * d.Wo, slabs = d.Cin / BK;
  long live = 0;
  for (long tm = 0; tm < tiles_m; ++tm) {
    uint32_t mask = 0;
    for (long m = tm * bm; m < (tm + 1) * bm && m < d.M; ++m) {
      const int rem = (int)(mode.posmajor ? m / d.N : m % howo);
      const int bh = (rem / d.Wo) * d.stride - d.pad_t, bw = (rem % d.Wo) * d.stride - d.pad_l;
      for (int tp = 0; tp < d.ntaps; ++tp) {
        const int nh = bh + d.tap_dh[tp], nw = bw + d.tap_dw[tp];
        if (nh >= 0 && nh < d.H && nw >= 0 && nw < d.W) mask |= 1u << tp;
      }
    }
    live += (long)__builtin_popcount(mask) * slabs;
  }
  return live * tiles_n;
}

long ladder_igemm_fwd_live_chunks(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l,
                                  int bwd_data, int variant) {
  if (!conv_shape_ok(N, H, W, Cin, Ho, Wo, KH, KW, stride) || variant > 7) return -1;
  if (variant < 0) variant = igemm_default_variant();
  if (bwd_data == 0) {
    const IgemmDesc d = conv_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, 1, pad_t, pad_l, 0);
    if (smallcout_eligible(Cin, Cout, KH, KW, stride, (long)N * Ho * Wo) || cout1_eligible(Cin, Cout, KH, KW, stride, pad_t, pad_l, H, W, Ho, Wo) ||
        halo_eligible(d))
      return -1;
    return desc_live_chunks(d, variant);
  }
  const IgemmDesc d = bwd_data_desc(N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad_t, pad_l);
  if (stride == 1) return (smallcin_eligible(Cout, Cin, KH, KW) || halo_eligible(d)) ? -1 : desc_live_chunks(d, variant);
  if (stride == 2 && (Cout % BK) == 0 && KH * KW <= 28) {
    IgemmDesc cls[4];
    parity_classes(d, cls);
    long live = 0;
    for (const IgemmDesc& c : cls) {
      if (c.M == 0) continue;
      if (c.ntaps == 0) return desc_live_chunks(d, variant);
      live += desc_live_chunks(c, variant);
    }
    return live;
  }
  return desc_live_chunks(d, variant);
}

int ladder_dense_fwd_nt(const float* x, const float* wT, const float* bias, float* y, int M, int K, int N, int act, ladder_stream_t stream) {
  return dense_f32_nt_launch(x, wT, bias, y, nullptr, 0, M, K, N, act, stream);                    // (csrc/densef32.hip; LADDER_E_SHAPE when not eligible)
}

int ladder_dense_bwd_data_nt(const float* dy, const float* w, float* dx, int M, int K, int N, const float* gate_y, int gate_act, ladder_stream_t stream) {
  return dense_f32_nt_launch(dy, w, nullptr, dx, gate_y, gate_act, M, N, K, LADDER_ACT_NONE, stream);
}

int ladder_dense_bwd_data(const float* dy, const float* wT, float* dx, int M, int K, int N, const float* gate_y, int gate_act,
                          void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (dense_f32_big_ok(M, N, K)) return dense_f32_big_launch(dy, wT, nullptr, dx, gate_y, gate_act, M, N, K, LADDER_ACT_NONE, stream);
  return dispatch_fwd(dy, wT, nullptr, dx, dense_desc(M, N, K, LADDER_ACT_NONE), ws, ws_bytes, stream, gate_y, gate_act);
}

}  // extern "C"
