// The fitted full-covariance mixture on a WIDE latent, 64 < R <= 256, R % 16 == 0, 1 <= K <= 1024 (include/ladder_hip.h, section N21): the
// third form beside the packed one (R <= 8) and the whitening-GEMM one (R <= 64) of csrc/mixture.hip.  Strict fp32 on v_mfma_f32_16x16x4_f32;
// the whitened product Y [S, K*R] never exists: the squared norms are formed from the accumulators, only q [S, K] leaves the forward kernel.
//
// Parameter buffer (ladder_gmm_wide_param_bytes(K, R) bytes, 16-byte aligned; nb = R / 16):
//   bytes [0, 16)                      int32 status | int32 K | int32 R | int32 0
//                                      status: -1 = usable; k >= 0 = first component whose factorisation met a non-positive (or NaN) pivot;
//                                      -2 = the weights have no positive finite sum
//   then 4 ceil(K / 4) float32         logc[k] = log w_k - log sum w - sum log diag L_k - R/2 log 2 pi
//   then K * R float32                 means[k][j]
//   then K * nb(nb+1)/2 * 256 float32  Linv_k = L_k^-1 as 16 x 16 blocks (ib, jb <= ib) in the order ib(ib+1)/2 + jb, each block in the OPERAND ORDER of
//                                      the matrix instruction: float 4 lane + s of a block = Linv_k[16 ib + (lane & 15)][16 jb + 4 (lane >> 4) + s],
//                                      so a lane's four B operands of a block are one 16-byte load and a wavefront's load is 1 KB contiguous
//   then K * nb*nb * 256 float32       P_k = Linv_k^T Linv_k (the precision), all blocks (jb, ib) in the order jb nb + ib, float 4 lane + s =
//                                      P_k[16 jb + 4 (lane >> 4) + s][16 ib + (lane & 15)]
// every value the float64 result rounded to fp32.  The blocks above the diagonal of Linv_k are all zero and are neither stored nor multiplied:
// R = 256 keeps 136 of 256.
//
// The term (ladder_gmm_wide_logprob_fwd_bwd), S = L*B samples in tiles of 64 (4 wavefronts x 16 rows), t = mu + sd * eps formed in registers:
//   gmmw_q_kernel     grid (tiles, KS): per component of the workgroup's K range d = t - m_k, y = Linv_k d block row by block row, q[s][k] = |y|^2
//   gmmw_lse_kernel   a thread per sample: lp_k = logc_k - q_k / 2, max-subtracted logsumexp, q <- responsibilities, a double partial per workgroup
//   sum_doubles_kernel   (common.h) the partials in a fixed order -> sum_logp
//   gmmw_g_kernel     grid (tiles, KS): acc = sum_k (r_sk d_sk) P_k over the K range with the scaled operand formed in registers, g[ks][s][:] = -acc;
//                     a component whose responsibilities are exactly zero on all 16 samples of a wavefront's rows is skipped (it adds +-0)
//   gmmw_reduce_kernel dmu[b] = sum_l sum_ks g[ks][l,b], dsd[b] = sum_l (sum_ks g[ks][l,b]) eps[l,b], l ascending, ks ascending inside
// KS splits K over workgroups so that they fill the chip in whole rounds (gw_best_split; at most 16 for q, at most 5 partial g, whose number the
// workspace is sized for from S alone).  No atomics on floating-point data, no
// grid-wide synchronisation, one fixed order for every sum.  Every kernel compares the header with its own (K, R) before it reads anything
// else; an unusable or foreign buffer gives NaN outputs.
#include "chol_wide.h"
#include "gmm_packed.h"

namespace {

typedef float f32x4w __attribute__((ext_vector_type(4)));

constexpr int GW_MAXK = 1024, GW_TILE = 64, GW_MAXNB = CW_MAXR / 16;

__host__ __device__ inline bool gw_shape_ok(int K, int R) { return K >= 1 && K <= GW_MAXK && cw_width_ok(R); }
__host__ __device__ inline size_t gw_kpad(int K) { return ((size_t)K + 3) & ~(size_t)3; }
__host__ __device__ inline size_t gw_tri_blocks(int R) { return (size_t)(R / 16) * (R / 16 + 1) / 2; }
__host__ __device__ inline size_t gw_off_means(int K) { return 16 + gw_kpad(K) * 4; }
__host__ __device__ inline size_t gw_off_linv(int K, int R) { return gw_off_means(K) + (size_t)K * R * 4; }
__host__ __device__ inline size_t gw_off_prec(int K, int R) { return gw_off_linv(K, R) + (size_t)K * gw_tri_blocks(R) * 1024; }
__host__ __device__ inline size_t gw_bytes(int K, int R) { return gw_off_prec(K, R) + (size_t)K * (R / 16) * (R / 16) * 1024; }

__device__ __forceinline__ bool gw_header_ok(const unsigned char* params, int K, int R) {
  const int4 head = *reinterpret_cast<const int4*>(params);
  return head.x == -1 && head.y == K && head.z == R;
}
__device__ __forceinline__ float gw_nan() { return __int_as_float(0x7fc00000); }

// ----------------------------------------------------------------------------------------------------------------- prepare
__global__ void gmmw_header_kernel(const float* __restrict__ w, const float* __restrict__ means, int K, int R, unsigned char* params) {
  int* head = reinterpret_cast<int*>(params);
  float* m = reinterpret_cast<float*>(params + gw_off_means(K));
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int k = 0; k < K; ++k) total += (double)w[k];
    head[0] = (total > 0.0 && total <= 1.7e308) ? -1 : -2;
    head[1] = K;
    head[2] = R;
    head[3] = 0;
  }
  for (int i = threadIdx.x; i < K * R; i += blockDim.x) m[i] = means[i];
}

// Workgroup b factors the components b, b + gridDim.x, ... in its slot of the workspace (chol_wide.h), then packs Linv_k and P_k.
__global__ __launch_bounds__(CW_THREADS) void gmmw_prepare_kernel(const float* __restrict__ w, const float* __restrict__ covs, int K, int R,
                                                                   unsigned char* params, double* ws) {
  __shared__ CwShared sh;
  __shared__ double s_logw;
  const int tid = threadIdx.x, nb = R / 16;
  double* W = ws + (size_t)blockIdx.x * R * R;
  float* logc = reinterpret_cast<float*>(params + 16);
  for (int k = blockIdx.x; k < K; k += gridDim.x) {
    __syncthreads();                                     // (the previous component's W and LDS are no longer read)
    const bool failed = chol_wide_factor<true>(covs + (size_t)k * R * R, R, W, sh);
    if (failed) {
      if (tid == 0) atomicMin(reinterpret_cast<unsigned*>(params), (unsigned)k);     // (-1 and -2 are the largest unsigned values)
      continue;
    }
    if (tid == 0) {
      double total = 0.0;
      for (int q = 0; q < K; ++q) total += (double)w[q];
      s_logw = log((double)w[k]) - log(total);
    }
    const double ld = cw_log_diag_sum(W, R, sh.panel);   // (its barriers also publish s_logw)
    if (tid == 0) logc[k] = (float)(s_logw - ld - 0.5 * R * kLog2Pi);
    // Linv_k: element e of the component's packed region -> (block, lane, s)
    float* lp = reinterpret_cast<float*>(params + gw_off_linv(K, R)) + (size_t)k * gw_tri_blocks(R) * 256;
    for (int ib = 0; ib < nb; ++ib)
      for (int jb = 0; jb <= ib; ++jb) {
        float* blk = lp + ((size_t)ib * (ib + 1) / 2 + jb) * 256;
        const int lane = tid >> 2, s = tid & 3;
        const int i = 16 * ib + (lane & 15), j = 16 * jb + 4 * (lane >> 4) + s;
        blk[tid] = i >= j ? (float)cw_linv(W, R, i, j) : 0.f;
      }
    // P_k[i][j] = sum_{r >= i} Linv[r][i] Linv[r][j] for i >= j: thread j walks down its column; both mirror elements are written
    float* pp = reinterpret_cast<float*>(params + gw_off_prec(K, R)) + (size_t)k * nb * nb * 256;
    if (tid < R) {
      const int j = tid;
      const double* wj = W + (size_t)j * R;
      for (int i = j; i < R; ++i) {
        const double* wi = W + (size_t)i * R;
        const double ii = 1.0 / wi[i];
        double a = ii * (i == j ? ii : wj[i]);
        for (int r = i + 1; r < R; ++r) a += wi[r] * wj[r];
        const float v = (float)a;
        // element [row][col] of P sits in block (row / 16) nb + col / 16 at float 4 ((row % 16) / 4 * 16 + col % 16) + row % 4
        pp[((size_t)(i >> 4) * nb + (j >> 4)) * 256 + 4 * ((((i & 15) >> 2) << 4) + (j & 15)) + (i & 3)] = v;
        pp[((size_t)(j >> 4) * nb + (i >> 4)) * 256 + 4 * ((((j & 15) >> 2) << 4) + (i & 15)) + (j & 3)] = v;
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------------------------- the term
// This lane's A operands of tile row m = lane & 15: t[s][16 jb + 4 kq + 0..3] for every block jb, kq = lane >> 4; zero past S.
// ROWS: `mu` is t itself [S, R]; else t = mu[b] + sd[b] * eps[s] with b = s % B.
template <bool ROWS>
__device__ __forceinline__ void gw_load_rows(const float* __restrict__ mu, const float* __restrict__ sd, const float* __restrict__ eps, int S, int B,
                                             int R, int nb, int s, int kq, float (&ta)[4 * GW_MAXNB]) {
  const bool ok = s < S;
  const size_t so = (size_t)(ok ? s : 0) * R, bo = ROWS ? so : (size_t)((ok ? s : 0) % B) * R;
#pragma unroll
  for (int jb = 0; jb < GW_MAXNB; ++jb) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (jb < nb && ok) {
      const int c = 16 * jb + 4 * kq;
      v = *reinterpret_cast<const float4*>(mu + bo + c);
      if (!ROWS) {
        const float4 sg = *reinterpret_cast<const float4*>(sd + bo + c), e = *reinterpret_cast<const float4*>(eps + so + c);
        v = make_float4(fmaf(sg.x, e.x, v.x), fmaf(sg.y, e.y, v.y), fmaf(sg.z, e.z, v.z), fmaf(sg.w, e.w, v.w));
      }
    }
    ta[4 * jb] = v.x; ta[4 * jb + 1] = v.y; ta[4 * jb + 2] = v.z; ta[4 * jb + 3] = v.w;
  }
}

// d = scale * (ta - m_k) on this lane's operand columns
__device__ __forceinline__ void gw_centre(const float (&ta)[4 * GW_MAXNB], const float* __restrict__ mean, int nb, int kq, float scale,
                                          float (&d)[4 * GW_MAXNB]) {
#pragma unroll
  for (int jb = 0; jb < GW_MAXNB; ++jb) {
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (jb < nb) m = *reinterpret_cast<const float4*>(mean + 16 * jb + 4 * kq);
    d[4 * jb] = scale * (ta[4 * jb] - m.x); d[4 * jb + 1] = scale * (ta[4 * jb + 1] - m.y);
    d[4 * jb + 2] = scale * (ta[4 * jb + 2] - m.z); d[4 * jb + 3] = scale * (ta[4 * jb + 3] - m.w);
  }
}

// the four matrix instructions of input block jb: contraction index 16 jb + 4 (lane >> 4) + s, s = 0..3
__device__ __forceinline__ f32x4w gw_mma4(const float (&d)[4 * GW_MAXNB], int jb, const float4 b, f32x4w acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(d[4 * jb], b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(d[4 * jb + 1], b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(d[4 * jb + 2], b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(d[4 * jb + 3], b.w, acc, 0, 0, 0);
  return acc;
}

// the K range of split ks
__device__ __forceinline__ void gw_krange(int K, int KS, int ks, int& k0, int& k1) {
  k0 = (int)((long long)K * ks / KS);
  k1 = (int)((long long)K * (ks + 1) / KS);
}

template <bool ROWS>
__global__ __launch_bounds__(256) void gmmw_q_kernel(const float* __restrict__ mu, const float* __restrict__ sd, const float* __restrict__ eps,
                                                     const unsigned char* __restrict__ params, int S, int B, int R, int K, float* __restrict__ q) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
  const int nb = R / 16, KS = gridDim.y;
  const int row0 = blockIdx.x * GW_TILE + wave * 16;     // first sample of this wavefront's 16 rows
  int k0, k1;
  gw_krange(K, KS, blockIdx.y, k0, k1);
  if (!gw_header_ok(params, K, R)) {                     // (uniform over the grid)
    for (int k = k0; k < k1; ++k)
      if (lane < 16 && row0 + lane < S) q[(size_t)(row0 + lane) * K + k] = gw_nan();
    return;
  }
  const float* means = reinterpret_cast<const float*>(params + gw_off_means(K));
  const float4* linv = reinterpret_cast<const float4*>(params + gw_off_linv(K, R));
  const size_t tri = gw_tri_blocks(R);
  float ta[4 * GW_MAXNB], d[4 * GW_MAXNB];
  gw_load_rows<ROWS>(mu, sd, eps, S, B, R, nb, row0 + m, kq, ta);
  for (int k = k0; k < k1; ++k) {
    gw_centre(ta, means + (size_t)k * R, nb, kq, 1.f, d);
    const float4* lk = linv + (size_t)k * tri * 64 + lane;
    float qs[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ib = 0; ib < GW_MAXNB; ++ib) {
      if (ib < nb) {                                     // Linv_k is lower triangular: the blocks right of the diagonal are skipped
        f32x4w a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};       // two chains: even and odd input blocks
#pragma unroll
        for (int jb = 0; jb <= ib; ++jb) {
          const float4 b = lk[(size_t)(ib * (ib + 1) / 2 + jb) * 64];
          if (jb & 1) a1 = gw_mma4(d, jb, b, a1); else a0 = gw_mma4(d, jb, b, a0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float y = a0[r] + a1[r];
          qs[r] = fmaf(y, y, qs[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) qs[r] += __shfl_xor(qs[r], o, 64);     // over the 16 output columns of the lane group
      const int s = row0 + 4 * kq + r;                   // accumulator register r: tile row 4 (lane >> 4) + r
      if (m == 0 && s < S) q[(size_t)s * K + k] = qs[r];
    }
  }
}

// a thread per sample.  write_r: q[s][k] <- responsibilities.  row_lse (may be NULL): the per-sample values.
__global__ __launch_bounds__(256) void gmmw_lse_kernel(float* __restrict__ q, const unsigned char* __restrict__ params, int S, int K, int R,
                                                       int write_r, double* __restrict__ part, float* __restrict__ row_lse) {
  __shared__ double blk[4];
  const int s = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool ok = gw_header_ok(params, K, R);
  const float* logc = reinterpret_cast<const float*>(params + 16);
  double lse_d = 0.0;
  if (s < S) {
    float* row = q + (size_t)s * K;
    float lse = gw_nan();
    if (ok) {
      float mx = -INFINITY;
      for (int k = 0; k < K; ++k) mx = fmaxf(mx, logc[k] - 0.5f * row[k]);
      float se = 0.f;
      for (int k = 0; k < K; ++k) se += expf((logc[k] - 0.5f * row[k]) - mx);
      lse = mx + logf(se);
      if (write_r)
        for (int k = 0; k < K; ++k) row[k] = expf((logc[k] - 0.5f * row[k]) - lse);
    } else if (write_r) {
      for (int k = 0; k < K; ++k) row[k] = gw_nan();
    }
    if (row_lse != nullptr) row_lse[s] = lse;
    lse_d = (double)lse;
  }
  lse_d = wave_sum_d(lse_d);
  if (lane == 0) blk[wave] = lse_d;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (blk[0] + blk[1]) + (blk[2] + blk[3]);
}

__global__ __launch_bounds__(256) void gmmw_g_kernel(const float* __restrict__ mu, const float* __restrict__ sd, const float* __restrict__ eps,
                                                     const unsigned char* __restrict__ params, const float* __restrict__ resp, int S, int B, int R,
                                                     int K, float* __restrict__ g) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
  const int nb = R / 16, KS = gridDim.y;
  const int row0 = blockIdx.x * GW_TILE + wave * 16;
  float* gk = g + (size_t)blockIdx.y * S * R;
  if (!gw_header_ok(params, K, R)) {
    for (int r = 0; r < 16; ++r)
      if (row0 + r < S)
        for (int c = lane; c < R; c += 64) gk[(size_t)(row0 + r) * R + c] = gw_nan();
    return;
  }
  int k0, k1;
  gw_krange(K, KS, blockIdx.y, k0, k1);
  const float* means = reinterpret_cast<const float*>(params + gw_off_means(K));
  const float4* prec = reinterpret_cast<const float4*>(params + gw_off_prec(K, R));
  float ta[4 * GW_MAXNB], d[4 * GW_MAXNB];
  const int s_a = row0 + m;                              // the sample of this lane's A operands
  gw_load_rows<false>(mu, sd, eps, S, B, R, nb, s_a, kq, ta);
  f32x4w acc[GW_MAXNB];
#pragma unroll
  for (int ib = 0; ib < GW_MAXNB; ++ib) acc[ib] = f32x4w{0.f, 0.f, 0.f, 0.f};
  for (int k = k0; k < k1; ++k) {
    const float r = s_a < S ? resp[(size_t)s_a * K + k] : 0.f;
    if (!__any(r != 0.f)) continue;                      // (wavefront-uniform; a NaN responsibility is not skipped)
    gw_centre(ta, means + (size_t)k * R, nb, kq, r, d);
    const float4* pk = prec + (size_t)k * nb * nb * 64 + lane;
#pragma unroll
    for (int jb = 0; jb < GW_MAXNB; ++jb) {
      if (jb < nb) {
#pragma unroll
        for (int ib = 0; ib < GW_MAXNB; ++ib) {
          if (ib < nb) {
            const float4 b = *pk;                        // block jb nb + ib: the blocks are visited in storage order
            pk += 64;
            acc[ib] = gw_mma4(d, jb, b, acc[ib]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int ib = 0; ib < GW_MAXNB; ++ib) {
    if (ib < nb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int s = row0 + 4 * kq + r;
        if (s < S) gk[(size_t)s * R + 16 * ib + m] = -acc[ib][r];
      }
    }
  }
}

// dmu[b,j] = sum_l G[l,b,j], dsd[b,j] = sum_l G[l,b,j] eps[l,b,j] with G = the KS partials added in index order; l ascending
__global__ void gmmw_reduce_kernel(const float* __restrict__ g, const float* __restrict__ eps, float* __restrict__ dmu, float* __restrict__ dsd,
                                   int L, int BR, int KS) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BR) return;
  const size_t SR = (size_t)L * BR;
  float a = 0.f, b = 0.f;
#pragma unroll 4
  for (int l = 0; l < L; ++l) {                          // (the loads of four steps in flight; the additions keep their order)
    float v = g[(size_t)l * BR + i];
    for (int ks = 1; ks < KS; ++ks) v += g[ks * SR + (size_t)l * BR + i];
    a += v;
    b += v * eps[(size_t)l * BR + i];
  }
  dmu[i] = a;
  dsd[i] = b;
}

// ----------------------------------------------------------------------------------------------------------------- host side
int gw_tiles(size_t S) { return (int)((S + GW_TILE - 1) / GW_TILE); }
// K is split over gridDim.y workgroups per tile to fill the chip.  The matrix kernels run two workgroups per CU (two wavefronts per SIMD), 512 at
// a time on the 256 CUs this library is built for; with equal workgroups a launch takes ceil(workgroups / 512) rounds of ceil(K / KS) components, and
// the split with the smallest product wins (the smaller KS on a tie): 200 tiles, K = 50 -> KS = 5, 1000 workgroups of 10 components in two rounds,
// where KS = 3 is 600 workgroups of 17 in two rounds, the second round nearly empty.
constexpr int GW_RESIDENT = 512, GW_QSPLITS = 16, GW_GSPLITS = 5;
// partial gradients the workspace is sized for: a function of S alone
int gw_gsplits_max(size_t S) {
  const int t = gw_tiles(S), ks = (2 * GW_RESIDENT + t - 1) / t;
  return ks < 1 ? 1 : (ks > GW_GSPLITS ? GW_GSPLITS : ks);
}
int gw_best_split(int tiles, int K, int ksmax) {
  int best = 1;
  long long best_cost = -1;
  for (int ks = 1; ks <= ksmax && ks <= K; ++ks) {
    const long long cost = (((long long)tiles * ks + GW_RESIDENT - 1) / GW_RESIDENT) * ((K + ks - 1) / ks);
    if (best_cost < 0 || cost < best_cost) {
      best = ks;
      best_cost = cost;
    }
  }
  return best;
}
bool gw_samples_ok(long long L, long long B) { return L >= 1 && B >= 1 && L * B <= (1ll << 30); }

struct GwWorkspace {
  float* q;
  double* part;
  float* g;
};
// byte offsets of q | part | g behind the 256-byte aligned base, and the total (with the slack of the alignment)
struct GwLayout {
  size_t part, g, total;
};
GwLayout gw_layout(size_t S, int R, int K) {
  GwLayout l;
  l.part = ladder_round256(S * K * 4);
  l.g = l.part + ladder_round256(((S + 255) / 256) * 8);
  l.total = l.g + ladder_round256((size_t)gw_gsplits_max(S) * S * R * 4) + 256;
  return l;
}
GwWorkspace gw_workspace(size_t S, int R, int K, void* ws) {
  char* p = ladder_align256(ws);
  const GwLayout l = gw_layout(S, R, K);
  return GwWorkspace{(float*)p, (double*)(p + l.part), (float*)(p + l.g)};
}

}  // namespace

extern "C" {

size_t ladder_gmm_wide_param_bytes(int K, int R) { return gw_shape_ok(K, R) ? gw_bytes(K, R) : 0; }

size_t ladder_gmm_wide_prepare_workspace_bytes(int K, int R) { return gw_shape_ok(K, R) ? cw_workspace_bytes(K, R) : 0; }

int ladder_gmm_wide_prepare(const float* weights, const float* means, const float* covs, int K, int R, void* params, void* ws, size_t ws_bytes,
                            ladder_stream_t stream) {
  if (!gw_shape_ok(K, R) || weights == nullptr || means == nullptr || covs == nullptr || params == nullptr) return LADDER_E_SHAPE;
  if (!ladder_aligned16(params)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < cw_workspace_bytes(K, R)) return LADDER_E_WORKSPACE;
  hipLaunchKernelGGL(gmmw_header_kernel, dim3(1), dim3(256), 0, stream, weights, means, K, R, (unsigned char*)params);
  hipLaunchKernelGGL(gmmw_prepare_kernel, dim3(cw_slots(K)), dim3(CW_THREADS), 0, stream, weights, covs, K, R, (unsigned char*)params,
                     cw_workspace_base(ws));
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

size_t ladder_gmm_wide_workspace_bytes(int L, int B, int R, int K) {
  if (!gw_shape_ok(K, R) || !gw_samples_ok(L, B)) return 0;
  return gw_layout((size_t)L * B, R, K).total;
}

int ladder_gmm_wide_logprob_fwd_bwd(const float* mu, const float* sd, const float* eps, const void* params, int L, int B, int R, int K,
                                    float* sum_logp, float* dmu, float* dsd, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (!gw_shape_ok(K, R) || !gw_samples_ok(L, B) || (dmu == nullptr) != (dsd == nullptr)) return LADDER_E_SHAPE;
  if (mu == nullptr || sd == nullptr || eps == nullptr || params == nullptr || sum_logp == nullptr) return LADDER_E_SHAPE;
  if (!ladder_aligned16(mu) || !ladder_aligned16(sd) || !ladder_aligned16(eps) || !ladder_aligned16(params)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_gmm_wide_workspace_bytes(L, B, R, K)) return LADDER_E_WORKSPACE;
  const size_t S = (size_t)L * B;
  const GwWorkspace w = gw_workspace(S, R, K, ws);
  const unsigned char* p = (const unsigned char*)params;
  const int tiles = gw_tiles(S), nblk = (int)((S + 255) / 256);
  const int KSq = gw_best_split(tiles, K, GW_QSPLITS), KS = gw_best_split(tiles, K, gw_gsplits_max(S));
  const int train = dmu != nullptr ? 1 : 0;
  hipLaunchKernelGGL(gmmw_q_kernel<false>, dim3(tiles, KSq), dim3(256), 0, stream, mu, sd, eps, p, (int)S, B, R, K, w.q);
  hipLaunchKernelGGL(gmmw_lse_kernel, dim3(nblk), dim3(256), 0, stream, w.q, p, (int)S, K, R, train, w.part, (float*)nullptr);
  hipLaunchKernelGGL(sum_doubles_kernel<float>, dim3(1), dim3(64), 0, stream, (const double*)w.part, nblk, sum_logp);
  if (train) {
    hipLaunchKernelGGL(gmmw_g_kernel, dim3(tiles, KS), dim3(256), 0, stream, mu, sd, eps, p, (const float*)w.q, (int)S, B, R, K, w.g);
    hipLaunchKernelGGL(gmmw_reduce_kernel, dim3((B * R + 63) / 64), dim3(64), 0, stream, (const float*)w.g, eps, dmu, dsd, L, B * R, KS);
  }
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_gmm_wide_logprob_rows(const float* t, const void* params, int n, int R, int K, float* logp, void* ws, size_t ws_bytes,
                                 ladder_stream_t stream) {
  if (!gw_shape_ok(K, R) || !gw_samples_ok(1, n) || t == nullptr || params == nullptr || logp == nullptr) return LADDER_E_SHAPE;
  if (!ladder_aligned16(t) || !ladder_aligned16(params)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_gmm_wide_workspace_bytes(1, n, R, K)) return LADDER_E_WORKSPACE;
  const size_t S = (size_t)n;
  const GwWorkspace w = gw_workspace(S, R, K, ws);
  const unsigned char* p = (const unsigned char*)params;
  const int tiles = gw_tiles(S), KS = gw_best_split(tiles, K, GW_QSPLITS), nblk = (int)((S + 255) / 256);
  hipLaunchKernelGGL(gmmw_q_kernel<true>, dim3(tiles, KS), dim3(256), 0, stream, t, (const float*)nullptr, (const float*)nullptr, p, (int)S, n, R, K,
                     w.q);
  hipLaunchKernelGGL(gmmw_lse_kernel, dim3(nblk), dim3(256), 0, stream, w.q, p, (int)S, K, R, 0, w.part, logp);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
