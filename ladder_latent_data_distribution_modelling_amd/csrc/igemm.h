// Internal interface of the implicit-GEMM convolution files (igemm.hip, igemm_wgrad.hip, igemm_split.hip, convdirect.hip): the by-value kernel
// descriptor with its builders, the device helpers every gather kernel uses, and the host functions that cross those files.
#pragma once
#include <cstdlib>
#include "split16.h"
#include "convf32.h"

struct FastDiv {   // exact unsigned 32-bit division by a runtime constant (Granlund-Montgomery round-up method)
  uint32_t m, s1, s2;
};
struct IgemmDesc {
  int N, H, W, Cin;      // gathered tensor
  int Ho, Wo, Cout;      // GEMM-M spatial extent and GEMM-N
  int KH, KW, stride, ups, pad_t, pad_l;
  int M, K;
  int act;
  FastDiv div_howo, div_wo;
  // fast path (Cin % 16 == 0): explicit tap table.  K order = channel slab outer, taps inner; tap t reads the input at
  // (base_h + tap_dh[t], base_w + tap_dw[t]) and the filter tap tap_w[t] (= r*KW + s of the HWIO bank).
  int ntaps;
  signed char tap_dh[28], tap_dw[28], tap_w[28];
  // output pixel (ho, wo) of the M space is stored at y[n, out_h0 + ho*out_sh, out_w0 + wo*out_sw, :] of an OH x OW map
  int out_sh, out_sw, out_h0, out_w0, OH, OW;
};

// Fills the tap table / output mapping of an ordinary convolution (all KH*KW taps, dense output).
inline bool set_conv_taps(IgemmDesc& d) {
  d.out_sh = d.out_sw = 1;
  d.out_h0 = d.out_w0 = 0;
  d.OH = d.Ho;
  d.OW = d.Wo;
  d.ntaps = 0;
  if (d.ups != 1 || d.KH * d.KW > 28) return false;
  for (int r = 0; r < d.KH; ++r)
    for (int sx = 0; sx < d.KW; ++sx) {
      d.tap_dh[d.ntaps] = (signed char)r;
      d.tap_dw[d.ntaps] = (signed char)sx;
      d.tap_w[d.ntaps] = (signed char)(r * d.KW + sx);
      ++d.ntaps;
    }
  return true;
}

// The tap table of a descriptor as the gather kernel's K loop reads it: 32-bit entries, so that a wave-uniform tap index is a scalar load.
// coff = element offset of the tap's input pixel from the row's base, kbase = first row of the tap in the [K x Cout] filter matrix,
// dhw = (tap_dh << 16) | (tap_dw & 0xffff).
struct TapTab {
  int coff[28], kbase[28], dhw[28];
};
inline TapTab make_taptab(const IgemmDesc& d) {
  TapTab t{};
  for (int i = 0; i < d.ntaps; ++i) {
    t.coff[i] = (d.tap_dh[i] * d.W + d.tap_dw[i]) * d.Cin;
    t.kbase[i] = d.tap_w[i] * d.Cin;
    t.dhw[i] = (int)(((unsigned)(int)d.tap_dh[i] << 16) | ((unsigned)(int)d.tap_dw[i] & 0xffffu));
  }
  return t;
}

namespace {

constexpr int kThreads = 256;
#ifndef IGEMM_BK
#define IGEMM_BK 16
#endif
#ifndef IGEMM_MINW
#define IGEMM_MINW 1
#endif
#ifndef IGEMM_HALO
#define IGEMM_HALO 1
#endif
#ifndef IGEMM_WH_BLOCKS     // workgroups per CU (x rounds) the halo filter-gradient plan aims for
#define IGEMM_WH_BLOCKS 2
#endif
#ifndef IGEMM_FWD_MINW
#define IGEMM_FWD_MINW 4
#endif
constexpr int BK = IGEMM_BK;

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// Source of out-of-image / out-of-range operands: loads stay unconditional (no exec-mask branches around VMEM in the
// K loop); lanes that would read padding fetch these 16 zero bytes instead.
__device__ __attribute__((aligned(16))) float g_zero16[4] = {0.f, 0.f, 0.f, 0.f};
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv& f) {
  const uint32_t t = __umulhi(f.m, n);
  return (t + ((n - t) >> f.s1)) >> f.s2;
}
inline FastDiv make_fastdiv(uint32_t d) {
  uint32_t l = 0;
  while ((1ull << l) < d) ++l;
  FastDiv f;
  f.m = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
  f.s1 = l < 1 ? l : 1;
  f.s2 = l > 1 ? l - 1 : 0;
  return f;
}

// One gathered element of A: returns pointer offset or -1 when the tap falls outside / between samples.
__device__ __forceinline__ long gather_off(const IgemmDesc& d, long img, int bh, int bw, int r, int s, int ci) {
  int nh = bh + r, nw = bw + s;
  if (nh < 0 || nw < 0) return -1;
  if (d.ups > 1) {
    if ((nh % d.ups) | (nw % d.ups)) return -1;
    nh /= d.ups;
    nw /= d.ups;
  }
  if (nh >= d.H || nw >= d.W) return -1;
  return img + ((long)nh * d.W + nw) * d.Cin + ci;
}

// ---- descriptor builders (host) ---------------------------------------------------------------------------------------------------
inline bool conv_shape_ok(int N, int H, int W, int Cin, int Ho, int Wo, int KH, int KW, int stride) {
  return N > 0 && H > 0 && W > 0 && Cin > 0 && Ho > 0 && Wo > 0 && KH > 0 && KW > 0 && stride > 0;
}

// Descriptor of a forward-shaped convolution with its tap table (ups != 1 or more than 28 taps: no table, the kernels gather generically).
// The filter-gradient kernels take the same descriptor: they read the geometry fields only, never ntaps / tap_* / out_* / OH / OW.
inline IgemmDesc conv_desc(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int ups, int pad_t, int pad_l,
                           int act) {
  const int howo = Ho * Wo;                                   // (queries may carry an empty map: no division by zero on their way to a refusal)
  IgemmDesc d{N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, ups, pad_t, pad_l, N * Ho * Wo, KH * KW * Cin, act,
              make_fastdiv(howo != 0 ? howo : 1), make_fastdiv(Wo != 0 ? Wo : 1)};
  set_conv_taps(d);
  return d;
}

// Backward-data of the convolution [N,H,W,Cin] -> [N,Ho,Wo,Cout] as a forward-shaped gather over dy with the flipped, transposed bank:
// dx[hi] gathers dy[(hi + pad_t - r)/stride] = dy[(hi + r' - (KH-1-pad_t))/stride] with the flipped tap r'.
// (stride 1: full tap table; stride > 1: dense output mapping only, ntaps = 0 -> generic gather or the parity classes below)
inline IgemmDesc bwd_data_desc(int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int KH, int KW, int stride, int pad_t, int pad_l) {
  return conv_desc(N, Ho, Wo, Cout, H, W, Cin, KH, KW, 1, stride, KH - 1 - pad_t, KW - 1 - pad_l, LADDER_ACT_NONE);
}

// y [M][N] = x [M][K] . w [K][N]: a 1x1 convolution of M one-pixel samples
inline IgemmDesc dense_desc(int M, int K, int N, int act) { return conv_desc(M, 1, 1, K, 1, 1, N, 1, 1, 1, 1, 0, 0, act); }

// Parity-class decomposition of a stride-2 backward-data `d` (bwd_data_desc, KH * KW <= 28): output pixels with (hi, wi) parity (ch, cw)
// only ever see the flipped taps r' = (pad' + ch) mod 2 (+2), so each class is a dense stride-1 gather over ~1/4 of the taps written to
// every other output pixel -- no zero taps enter the MFMA pipeline.  cls[2 * ch + cw] = the descriptor of the class; M == 0 when the map
// has no pixel of that parity, ntaps == 0 when no tap lands on it.
inline void parity_classes(const IgemmDesc& d, IgemmDesc (&cls)[4]) {
  for (int ch = 0; ch < 2; ++ch)
    for (int cw = 0; cw < 2; ++cw) {
      IgemmDesc& c = cls[2 * ch + cw];
      c = d;
      c.Ho = (d.Ho - ch + 1) / 2; c.Wo = (d.Wo - cw + 1) / 2; c.stride = 1; c.ups = 1; c.pad_t = 0; c.pad_l = 0;
      c.M = d.N * c.Ho * c.Wo;
      c.ntaps = 0;
      if (c.M <= 0) { c.M = 0; continue; }
      c.div_howo = make_fastdiv(c.Ho * c.Wo);
      c.div_wo = make_fastdiv(c.Wo);
      c.out_sh = c.out_sw = 2; c.out_h0 = ch; c.out_w0 = cw; c.OH = d.Ho; c.OW = d.Wo;
      for (int r = 0; r < d.KH; ++r) {
        if (((r + d.pad_t + ch) & 1) != 0) continue;
        for (int sx = 0; sx < d.KW; ++sx) {
          if (((sx + d.pad_l + cw) & 1) != 0) continue;
          c.tap_dh[c.ntaps] = (signed char)((ch + r - d.pad_t) / 2);     // exact: numerator is even
          c.tap_dw[c.ntaps] = (signed char)((cw + sx - d.pad_l) / 2);
          c.tap_w[c.ntaps] = (signed char)(r * d.KW + sx);
          ++c.ntaps;
        }
      }
      c.K = c.ntaps * d.Cin;
    }
}

}  // namespace

static_assert(sizeof(IgemmDesc) == 200, "IgemmDesc is a by-value kernel argument: its layout is fixed");

// Debug / validation switch: LADDER_DISABLE_HALO=1 in the environment routes every convolution through the generic gather
// kernels (used by the tests to cross-check the halo kernels in situ at full size).  Read on every call: no cached state.
inline bool halo_disabled() {
  const char* e = getenv("LADDER_DISABLE_HALO");
  return e != nullptr && e[0] == '1';
}

// ---- host functions that cross files ----------------------------------------------------------------------------------------------
// igemm.hip: the fp32 forward family
struct SplitPlan { int splits, cps; };
int select_fwd_tile(long M, int Cout);                       // BM*1000 + BN
SplitPlan plan_splitk(long M, int K, int Cout, int bm, int bn);
bool halo_eligible(const IgemmDesc& d);
int dispatch_fwd(const float* x, const float* w, const float* bias, float* y, const IgemmDesc& d, void* ws, size_t ws_bytes, hipStream_t st,
                 const float* gate = nullptr, int gate_act = 0);
// igemm_fwd_kernel variants: bit 0 = position-major rows and padding-tap skipping on small maps, bits 1-2 = prefetch depth - 1; -1 = the default
// (default: the skipping on, one chunk ahead -- deeper prefetch measured within the run-to-run spread of the step, profiles/gather_small_maps.md)
constexpr int IGEMM_VARIANT_DEFAULT = 1;
int igemm_default_variant();                                 // IGEMM_VARIANT_DEFAULT, or LADDER_IGEMM_VARIANT from the environment (read once)
int dispatch_fwd(const float* x, const float* w, const float* bias, float* y, const IgemmDesc& d, void* ws, size_t ws_bytes, hipStream_t st,
                 const float* gate, int gate_act, int variant);
// second pass of a split-K launch: y = act(sum of the `splits` partials [M][Cout] + bias) (* act'(gate)), dense or through d's output mapping
// (posmajor: the partial rows are ordered (position, image) -- the first pass ran over position-major rows)
void launch_splitk_epilogue(const float* part, const float* bias, float* y, int splits, const IgemmDesc& d, const float* gate, int gate_act,
                            hipStream_t st, bool posmajor = false);

// igemm_wgrad.hip: the fp32 filter gradients
struct WgradPlan { int bm, bn, tiles_k, tiles_n, splits, m_per_split; };
struct WgradHaloPlan { bool ok; int tiles_ci, tiles_co, splits, pps, pw, stride; };    // pw: patch width 32 / 16 / 8 (patch = 32 / pw rows)
WgradPlan plan_wgrad(long M, int K, int Cout);
WgradHaloPlan plan_wgrad_halo(const IgemmDesc& d);
void launch_reduce_splits(const float* ws, float* out, int S, size_t n, hipStream_t st);

// The tail of a filter gradient.  The workspace holds the partials [splits][kn], then the bias partials [splits][Cout] (db != NULL); reduce()
// sums both in a fixed order into dw / db.  `direct`: a single split writes dw itself, and the bias partials then start the workspace.
struct WgradTail {
  float *part, *bias_part, *dw, *db;
  int splits, Cout;
  size_t kn;
  int reduce(hipStream_t st) const {
    if (part != dw) launch_reduce_splits(part, dw, splits, kn, st);
    if (db != nullptr) launch_reduce_splits(bias_part, db, splits, (size_t)Cout, st);
    LADDER_CHECK_LAUNCH();
    return LADDER_OK;
  }
};
inline WgradTail wgrad_tail(void* ws, int splits, size_t kn, int Cout, float* dw, float* db, bool direct = false) {
  float* part = (direct && splits == 1) ? dw : (float*)ws;
  return WgradTail{part, db != nullptr ? (float*)ws + (part != dw ? (size_t)splits * kn : 0) : nullptr, dw, db, splits, Cout, kn};
}

// convdirect.hip: the direct kernels for tiny channel counts
bool smallcin_eligible(int Cin, int Cout, int KH, int KW);
int launch_smallcin(const float* x, const float* w, const float* bias, float* y, const float* gate, int N, int H, int W, int Cin, int Ho,
                    int Wo, int Cout, int KH, int stride, int pad_t, int pad_l, int act, hipStream_t st);
bool cout1_eligible(int Cin, int Cout, int KH, int KW, int stride, int pad_t, int pad_l, int H, int W, int Ho, int Wo);
size_t cout1_wgrad_ws_bytes(int N, int Ho, int Cin);
// forward (dy == NULL: y = act(conv(x, w) + bias)) or filter gradient (dy != NULL: block partials in `part`, cout1_wgrad_ws_bytes, summed into dw / db)
void launch_cout1(const float* x, const float* w, const float* bias, float* y, const float* dy, float* part, float* dw, float* db, int N,
                  int H, int W, int Cin, int Ho, int Wo, int act, hipStream_t st);
bool smallcout_eligible(int Cin, int Cout, int KH, int KW, int stride, long M);
int smallcout_blocks(long M, int Cin);
// forward (dy == NULL) or the one-pass backward (dy != NULL: dx, block partials of dw | db, optional absmax record of dx)
void launch_smallcout(const float* x, const float* w, const float* bias, float* y, const float* dy, float* dx, float* part, int Cin, int Cout,
                      int act, int M, float* dxamax, int rows_per_sample, int blocks, hipStream_t st);
