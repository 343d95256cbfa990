// Mixture-prior kernels of the LaDDer path for gfx950: the packed full-covariance mixture on narrow latents (R <= 8: preparation,
// log-prob + responsibilities-weighted gradient with wavefront-shuffle logsumexp, log-prob of separate points; per-component arithmetic
// in gmm_packed.h), and the same mixture on wide latents with the whitening as a GEMM on the dense kernel (prior "GMM").
#include "common.h"
#include "gmm_packed.h"

namespace {

// ----------------------------------------------------------------------------- mixture hyper-prior (packed layout: gmm_packed.h)
template <int R>
__global__ void gmm_prepare_kernel(const float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ cov, int K,
                                   float* __restrict__ packed) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  using P = GmmPacked<R>;
  float wsum = 0.f;
  for (int j = 0; j < K; ++j) wsum += w[j];
  float Lm[R][R], Li[R][R];
  const float* c = cov + (size_t)k * R * R;
  float logdet = 0.f;
#pragma unroll
  for (int i = 0; i < R; ++i) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      Lm[i][j] = 0.f;
      Li[i][j] = 0.f;
    }
  }
#pragma unroll
  for (int j = 0; j < R; ++j) {       // Cholesky-Banachiewicz, fp32 like tf.linalg.cholesky on the fp32 feed
    float s = c[j * R + j];
#pragma unroll
    for (int p = 0; p < R; ++p)
      if (p < j) s -= Lm[j][p] * Lm[j][p];
    const float djj = sqrtf(s);
    Lm[j][j] = djj;
    logdet += logf(djj);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i > j) {
        float t = c[i * R + j];
#pragma unroll
        for (int p = 0; p < R; ++p)
          if (p < j) t -= Lm[i][p] * Lm[j][p];
        Lm[i][j] = t / djj;
      }
    }
  }
#pragma unroll
  for (int col = 0; col < R; ++col) {  // Linv by forward substitution on the identity
#pragma unroll
    for (int i = 0; i < R; ++i) {
      if (i >= col) {
        float t = (i == col) ? 1.f : 0.f;
#pragma unroll
        for (int p = 0; p < R; ++p)
          if (p >= col && p < i) t -= Lm[i][p] * Li[p][col];
        Li[i][col] = t / Lm[i][i];
      }
    }
  }
  float* o = packed + (size_t)k * P::STRIDE;
  o[0] = logf(w[k]) - logf(wsum) - logdet - 0.5f * (float)R * (float)kLog2Pi;
#pragma unroll
  for (int j = 0; j < R; ++j) o[P::MEAN + j] = m[(size_t)k * R + j];
  GMM_TRI_EACH(R, i, j, q, o[P::TRI + q] = Li[i][j]);
}

// One workgroup (4 wavefronts) per batch row b; wavefront w handles MC samples l = w, w+4, ...; lane = component.
// Per sample: lp_k in-lane, logsumexp and the R gradient components reduced with wave shuffles.
template <int R>
__global__ __launch_bounds__(256) void gmm_logprob_kernel(const float* __restrict__ mu, const float* __restrict__ sd,
                                                          const float* __restrict__ eps, const float* __restrict__ packed, int L,
                                                          int B, int K, float* __restrict__ dmu, float* __restrict__ dsd,
                                                          double* __restrict__ ws_logp) {
  constexpr int STRIDE = GmmPacked<R>::STRIDE, MEAN = GmmPacked<R>::MEAN, TRI = GmmPacked<R>::TRI;
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nchunk = (K + 63) / 64;
  float m_[R], s_[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    m_[j] = mu[(size_t)b * R + j];
    s_[j] = sd[(size_t)b * R + j];
  }
  double acc_lp = 0.0;
  float acc_mu[R], acc_sd[R];
#pragma unroll
  for (int j = 0; j < R; ++j) acc_mu[j] = acc_sd[j] = 0.f;

  for (int l = wv; l < L; l += 4) {
    float e_[R], t_[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      e_[j] = eps[((size_t)l * B + b) * R + j];
      t_[j] = m_[j] + s_[j] * e_[j];
    }
    // pass 1: log-prob per component, running max
    float mx = -INFINITY;
    for (int ch = 0; ch < nchunk; ++ch) {
      const int k = ch * 64 + lane;
      float lp = -INFINITY;
      if (k < K) {
        const float* prm = packed + (size_t)k * STRIDE;
        GMM_WHITEN(R, q, prm[TRI + q], j, t_[j] - prm[MEAN + j], y_, maha);
        lp = prm[0] - 0.5f * maha;
      }
      mx = fmaxf(mx, lp);
    }
    mx = wave_max(mx);
    // pass 2: sum exp, gradient numerators
    float se = 0.f, g_[R];
#pragma unroll
    for (int j = 0; j < R; ++j) g_[j] = 0.f;
    for (int ch = 0; ch < nchunk; ++ch) {
      const int k = ch * 64 + lane;
      if (k < K) {
        const float* prm = packed + (size_t)k * STRIDE;
        GMM_WHITEN(R, q, prm[TRI + q], j, t_[j] - prm[MEAN + j], y_, maha);
        const float ex = __expf(prm[0] - 0.5f * maha - mx);
        se += ex;
        // -exp(.) * (Linv^T y)_j, accumulated entry by entry as (ex * Linv_ij) * y_i: this kernel's own order of the back-projection
        GMM_TRI_EACH(R, i, j, q, g_[j] -= ex * prm[TRI + q] * y_[i]);
      }
    }
    se = wave_sum(se);
    acc_lp += (double)(mx + logf(se));
    const float inv = 1.f / se;
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const float G = wave_sum(g_[j]) * inv;   // d lp / d t_j = -sum_k r_k (Sigma_k^-1 (t-m_k))_j
      acc_mu[j] += G;
      acc_sd[j] += G * e_[j];
    }
  }
  __shared__ float sm_mu[4][R], sm_sd[4][R];
  __shared__ double sm_lp[4];
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
      sm_mu[wv][j] = acc_mu[j];
      sm_sd[wv][j] = acc_sd[j];
    }
    sm_lp[wv] = acc_lp;
  }
  __syncthreads();
  if (threadIdx.x < R) {
    const int j = threadIdx.x;
    dmu[(size_t)b * R + j] = (sm_mu[0][j] + sm_mu[1][j]) + (sm_mu[2][j] + sm_mu[3][j]);
    dsd[(size_t)b * R + j] = (sm_sd[0][j] + sm_sd[1][j]) + (sm_sd[2][j] + sm_sd[3][j]);
  }
  if (threadIdx.x == 0) ws_logp[b] = (sm_lp[0] + sm_lp[1]) + (sm_lp[2] + sm_lp[3]);
}
// ---- the same reduction with the mixture held in REGISTERS (K <= 64; round 3) ------------------------------------------------------
// The kernel above re-reads the 1 + R + R(R+1)/2 packed floats of its component from global memory for every MC sample, twice (it makes
// two passes: maximum, then exponentials), and runs 4 wavefronts on each of only B workgroups -- half the chip idle at B = 128, every
// wavefront a serial chain of L1 round trips: 116 us for L*B*K = 640 000 evaluations at R = 8 (BASELINE configs[4]).  Here lane k loads
// its component ONCE (45 registers at R = 8), keeps the whitened residual y = Linv (t - m_k) of the single pass for the gradient
// (d lp / d t = -sum_k r_k Linv_k^T y_k), and accumulates r_k-weighted gradient terms PER LANE across its samples, so that a sample costs
// two wave reductions (max, sum of exponentials) instead of 2 + R; the R + R gradient reductions happen once per wavefront.  The L
// samples of a batch row are spread over S = 4 gridDim.y wavefronts (workgroup (b, g), wavefront w takes l = 4g + w, + S, ...): B * S
// ~ 2048 wavefronts fill the chip; their partials are summed in a fixed order by gmm_finish_kernel.
template <int R>
__global__ __launch_bounds__(256) void gmm_logprob_reg_kernel(const float* __restrict__ mu, const float* __restrict__ sd,
                                                              const float* __restrict__ eps, const float* __restrict__ packed, int L,
                                                              int B, int K, double* __restrict__ ws_lp, float* __restrict__ ws_g) {
  const int b = blockIdx.x, lane = threadIdx.x & 63;
  const int S = 4 * gridDim.y, sidx = 4 * blockIdx.y + (threadIdx.x >> 6);
  using P = GmmPacked<R>;
  float c0 = -INFINITY, mk[R], Li[P::NT];                  // this lane's component; an idle lane (K < 64) contributes nothing
#pragma unroll
  for (int j = 0; j < R; ++j) mk[j] = 0.f;
#pragma unroll
  for (int q = 0; q < P::NT; ++q) Li[q] = 0.f;
  if (lane < K) {
    const float* prm = packed + (size_t)lane * P::STRIDE;
    c0 = prm[0];
#pragma unroll
    for (int j = 0; j < R; ++j) mk[j] = prm[P::MEAN + j];
#pragma unroll
    for (int q = 0; q < P::NT; ++q) Li[q] = prm[P::TRI + q];
  }
  float m_[R], s_[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    m_[j] = mu[(size_t)b * R + j];
    s_[j] = sd[(size_t)b * R + j];
  }
  double acc_lp = 0.0;
  float gm[R], gs[R];
#pragma unroll
  for (int j = 0; j < R; ++j) gm[j] = gs[j] = 0.f;
  for (int l = sidx; l < L; l += S) {
    float e_[R], d_[R];
#pragma unroll
    for (int j = 0; j < R; ++j) {
      e_[j] = eps[((size_t)l * B + b) * R + j];
      d_[j] = (m_[j] + s_[j] * e_[j]) - mk[j];
    }
    GMM_WHITEN(R, q, Li[q], j, d_[j], y_, maha);
    const float lp = c0 - 0.5f * maha;                      // -inf on the idle lanes (K < 64)
    const float mx = wave_max(lp);
    const float ex = __expf(lp - mx);
    const float se = wave_sum(ex);
    acc_lp += (double)(mx + logf(se));
    const float r = ex / se;
    GMM_BACK_PROJECT(R, q, Li[q], y_, v_);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const float g = r * v_[j];
      gm[j] -= g;
      gs[j] -= g * e_[j];
    }
  }
  float* o = ws_g + ((size_t)b * S + sidx) * (2 * R);
#pragma unroll
  for (int j = 0; j < R; ++j) {
    const float a = wave_sum(gm[j]), c = wave_sum(gs[j]);
    if (lane == 0) {
      o[j] = a;
      o[R + j] = c;
    }
  }
  if (lane == 0) ws_lp[(size_t)b * S + sidx] = acc_lp;
}

// dmu[b,j] / dsd[b,j] = sum over the S wavefront partials of row b (fixed order); the last workgroup sums the B * S log-prob partials.
__global__ __launch_bounds__(256) void gmm_finish_kernel(const double* __restrict__ ws_lp, const float* __restrict__ ws_g, int B, int S,
                                                         int R, float* __restrict__ dmu, float* __restrict__ dsd,
                                                         float* __restrict__ out) {
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x < 64) {
      double s = 0.0;
      for (int i = threadIdx.x; i < B * S; i += 64) s += ws_lp[i];
      s = wave_sum_d(s);
      if (threadIdx.x == 0) out[0] = (float)s;
    }
    return;
  }
  const int i = blockIdx.x * 256 + threadIdx.x;              // (b, jj) with jj in [0, 2R)
  if (i >= B * 2 * R) return;
  const int b = i / (2 * R), jj = i - b * 2 * R;
  float a = 0.f;
  for (int s = 0; s < S; ++s) a += ws_g[((size_t)b * S + s) * (2 * R) + jj];
  if (jj < R) dmu[(size_t)b * R + jj] = a; else dsd[(size_t)b * R + jj - R] = a;
}

// log p(t_i) of n separate points (density of the fitted mixture on a grid / at embeddings: demo/demo_tools.py prior.prob, log_prob):
// one wavefront per point, lane = component (and components lane + 64, ... of a larger mixture: online logsumexp per lane).
template <int R>
__global__ __launch_bounds__(256) void gmm_rows_kernel(const float* __restrict__ t, const float* __restrict__ packed, int n, int K,
                                                       float* __restrict__ logp) {
  constexpr int STRIDE = GmmPacked<R>::STRIDE, MEAN = GmmPacked<R>::MEAN, TRI = GmmPacked<R>::TRI;
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= n) return;
  float t_[R];
#pragma unroll
  for (int j = 0; j < R; ++j) t_[j] = t[(size_t)i * R + j];
  float mx = -INFINITY, se = 0.f;                 // online logsumexp over this lane's components, then across lanes
  for (int k = lane; k < K; k += 64) {
    const float* prm = packed + (size_t)k * STRIDE;
    GMM_WHITEN(R, q, prm[TRI + q], j, t_[j] - prm[MEAN + j], y_, maha);
    const float lp = prm[0] - 0.5f * maha;
    GMM_LSE_STEP(lp, mx, sc, ex);
    se = se * sc + ex;
  }
  const float gm = wave_max(mx);
  se = (mx == -INFINITY) ? 0.f : se * __expf(mx - gm);
  se = wave_sum(se);
  if (lane == 0) logp[i] = gm + logf(se);
}

// ----------------------------------------------------------------------------- mixture log-prob for WIDE latents (prior "GMM")
// prior == "GMM" puts the K-component full-covariance mixture on z itself (R = code_size = 16 / 64; codes/base.py:101-106,
// 322-329).  At that width the whitening y_k = Linv_k (t - m_k) of all components is a GEMM:  Y[S, K*R] = T[S, R] . Bmat[R, K*R]
// + bias with S = L*B MC samples, Bmat[:, kR+i] = Linv_k[i, :], bias[kR+i] = -(Linv_k m_k)[i]  (1.6 GMAC at R = 64, K = 30,
// L*B = 12 800) -- it runs on the dense MFMA kernel, and so does its transpose for the gradient dT = dY . Bmat^T with
// dY[s, kR+i] = -resp[s,k] * Y[s, kR+i].  The kernels below are the glue: parameter preparation (float64 Cholesky in LDS),
// MC sample assembly, the per-sample logsumexp / responsibilities over the Y blocks, and the reduction of dT over the L samples.
constexpr int GD_MAXR = 64;

__global__ __launch_bounds__(64) void gmm_prepare_dense_kernel(const float* __restrict__ w, const float* __restrict__ m,
                                                               const float* __restrict__ cov, int K, int R, float* __restrict__ Bmat,
                                                               float* __restrict__ BmatT, float* __restrict__ bias,
                                                               float* __restrict__ logc) {
  __shared__ double A[GD_MAXR * GD_MAXR];      // covariance -> Cholesky factor L (lower)
  __shared__ double Li[GD_MAXR * GD_MAXR];     // L^-1 (lower)
  __shared__ double sw;
  const int k = blockIdx.x, i = threadIdx.x;
  for (int e = i; e < R * R; e += 64) A[e] = (double)cov[(size_t)k * R * R + e];
  if (i == 0) {
    double t = 0.0;
    for (int q = 0; q < K; ++q) t += (double)w[q];
    sw = t;
  }
  __syncthreads();
  for (int j = 0; j < R; ++j) {
    if (i == j) {
      double d = A[j * R + j];
      for (int p = 0; p < j; ++p) d -= A[j * R + p] * A[j * R + p];
      A[j * R + j] = sqrt(d);
    }
    __syncthreads();
    if (i > j && i < R) {
      double v = A[i * R + j];
      for (int p = 0; p < j; ++p) v -= A[i * R + p] * A[j * R + p];
      A[i * R + j] = v / A[j * R + j];
    }
    __syncthreads();
  }
  if (i < R) {                                   // column i of L^-1 by forward substitution
    for (int r = 0; r < R; ++r) {
      double v = (r == i) ? 1.0 : 0.0;
      for (int p = i; p < r; ++p) v -= A[r * R + p] * Li[p * R + i];
      Li[r * R + i] = (r < i) ? 0.0 : v / A[r * R + r];
    }
  }
  __syncthreads();
  if (i < R) {                                   // row i of L^-1: whitening direction i of this component
    double b = 0.0;
    for (int j = 0; j < R; ++j) {
      const double v = Li[i * R + j];
      Bmat[(size_t)j * K * R + (size_t)k * R + i] = (float)v;
      BmatT[((size_t)k * R + i) * R + j] = (float)v;
      b -= v * (double)m[(size_t)k * R + j];
    }
    bias[(size_t)k * R + i] = (float)b;
  }
  if (i == 0) {
    double ld = 0.0;
    for (int j = 0; j < R; ++j) ld += log(A[j * R + j]);
    logc[k] = (float)(log((double)w[k]) - log(sw) - ld - 0.5 * R * kLog2Pi);
  }
}

__global__ void mc_samples_kernel(const float* __restrict__ mu, const float* __restrict__ sd, const float* __restrict__ eps,
                                  float* __restrict__ T, size_t n, int BR) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int br = (int)(i % BR);
  T[i] = mu[br] + sd[br] * eps[i];               // eps, T: [L, B, R]; mu, sd: [B, R]
}

// one wavefront per MC sample: lp_k = logc_k - 0.5 |Y_k|^2, logsumexp over k, responsibilities; Y <- dlogp/dY = -resp_k * Y_k.
__global__ __launch_bounds__(256) void gmm_dense_resp_kernel(float* __restrict__ Y, const float* __restrict__ logc, int S, int K, int R,
                                                             int write_dy, double* __restrict__ ws_lse,
                                                             float* __restrict__ row_lse = nullptr) {
  extern __shared__ float lp_sh[];               // [4 waves][K]
  __shared__ double blk[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int s = blockIdx.x * 4 + wv;
  float* lp = lp_sh + (size_t)wv * K;
  double lse_d = 0.0;
  if (s < S) {
    float* row = Y + (size_t)s * K * R;
    float mx = -INFINITY;
    for (int k = 0; k < K; ++k) {
      float q = 0.f;
      for (int i = lane; i < R; i += 64) {
        const float y = row[(size_t)k * R + i];
        q += y * y;
      }
      q = wave_sum(q);
      const float v = logc[k] - 0.5f * q;
      lp[k] = v;                                 // every lane holds the reduced value: no cross-lane dependency
      mx = fmaxf(mx, v);
    }
    float se = 0.f;
    for (int k = lane; k < K; k += 64) se += __expf(lp[k] - mx);
    se = wave_sum(se);
    const float lse = mx + __logf(se);
    lse_d = (double)lse;
    if (row_lse != nullptr && lane == 0) row_lse[s] = lse;
    if (write_dy)
      for (int k = 0; k < K; ++k) {
        const float r = __expf(lp[k] - lse);
        for (int i = lane; i < R; i += 64) row[(size_t)k * R + i] *= -r;
      }
  }
  if (lane == 0) blk[wv] = lse_d;
  __syncthreads();
  if (threadIdx.x == 0) ws_lse[blockIdx.x] = (blk[0] + blk[1]) + (blk[2] + blk[3]);
}

// dmu[b,r] = sum_l dT[l,b,r] ; dsd[b,r] = sum_l dT[l,b,r] * eps[l,b,r]   (fixed order over l)
__global__ void gmm_dense_reduce_kernel(const float* __restrict__ dT, const float* __restrict__ eps, float* __restrict__ dmu,
                                        float* __restrict__ dsd, int L, int BR) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= BR) return;
  float a = 0.f, b = 0.f;
  for (int l = 0; l < L; ++l) {
    const float g = dT[(size_t)l * BR + i];
    a += g;
    b += g * eps[(size_t)l * BR + i];
  }
  dmu[i] = a;
  dsd[i] = b;
}
}  // namespace

extern "C" {

int ladder_gmm_packed_stride(int R) { return 1 + R + R * (R + 1) / 2; }   // GmmPacked<R>::STRIDE

int ladder_gmm_prepare(const float* weights, const float* means, const float* covs, int K, int R, float* packed, ladder_stream_t stream) {
  if (K <= 0 || K > 1024) return LADDER_E_SHAPE;
  LADDER_R_SWITCH(R, hipLaunchKernelGGL(gmm_prepare_kernel<RR>, dim3((K + 63) / 64), dim3(64), 0, stream, weights, means, covs, K, packed));
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

// wavefront groups per batch row of the register kernel: ~2048 wavefronts in total, at most one per MC sample
static int gmm_row_groups(int L, int B) {
  int g = 512 / (B > 0 ? B : 1);
  const int gmax = (L + 3) / 4;
  g = g > gmax ? gmax : g;
  return g < 1 ? 1 : g;
}

size_t ladder_gmm_workspace_bytes(int L, int B) {
  const size_t S = (size_t)4 * gmm_row_groups(L, B);
  return (size_t)B * S * sizeof(double) + (size_t)B * S * 16 * sizeof(float);     // log-prob partials + [2R <= 16] gradient partials
}

int ladder_gmm_logprob_fwd_bwd(const float* mu, const float* sd, const float* eps, const float* packed, int L, int B, int R, int K,
                               float* sum_logp, float* dmu, float* dsd, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (L <= 0 || B <= 0 || K <= 0 || K > 1024) return LADDER_E_SHAPE;
  if (ws == nullptr || ws_bytes < ladder_gmm_workspace_bytes(L, B)) return LADDER_E_WORKSPACE;
  if (K <= 64) {                                            // the mixture in registers, lane = component
    const int G = gmm_row_groups(L, B), S = 4 * G;
    double* ws_lp = (double*)ws;
    float* ws_g = (float*)(ws_lp + (size_t)B * S);
    LADDER_R_SWITCH(R, hipLaunchKernelGGL(gmm_logprob_reg_kernel<RR>, dim3(B, G), dim3(256), 0, stream, mu, sd, eps, packed, L, B, K, ws_lp, ws_g));
    hipLaunchKernelGGL(gmm_finish_kernel, dim3((B * 2 * R + 255) / 256 + 1), dim3(256), 0, stream, (const double*)ws_lp, (const float*)ws_g, B, S, R,
                       dmu, dsd, sum_logp);
    LADDER_CHECK_LAUNCH();
    return LADDER_OK;
  }
  LADDER_R_SWITCH(R, hipLaunchKernelGGL(gmm_logprob_kernel<RR>, dim3(B), dim3(256), 0, stream, mu, sd, eps, packed, L, B, K, dmu, dsd, (double*)ws));
  hipLaunchKernelGGL(sum_doubles_kernel<float>, dim3(1), dim3(64), 0, stream, (const double*)ws, B, sum_logp);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_gmm_logprob_rows(const float* t, const float* packed, int n, int R, int K, float* logp, ladder_stream_t stream) {
  if (n <= 0 || K <= 0 || K > 1024) return LADDER_E_SHAPE;
  LADDER_R_SWITCH(R, hipLaunchKernelGGL(gmm_rows_kernel<RR>, dim3((n + 3) / 4), dim3(256), 0, stream, t, packed, n, K, logp));
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

size_t ladder_gmm_dense_param_floats(int K, int R) { return (size_t)2 * K * R * R + (size_t)K * R + K; }

int ladder_gmm_prepare_dense(const float* weights, const float* means, const float* covs, int K, int R, float* params,
                             ladder_stream_t stream) {
  if (K <= 0 || K > 1024 || R <= 0 || R > GD_MAXR || (R % 4) != 0) return LADDER_E_SHAPE;
  float* Bmat = params;
  float* BmatT = Bmat + (size_t)K * R * R;
  float* bias = BmatT + (size_t)K * R * R;
  float* logc = bias + (size_t)K * R;
  hipLaunchKernelGGL(gmm_prepare_dense_kernel, dim3(K), dim3(64), 0, stream, weights, means, covs, K, R, Bmat, BmatT, bias, logc);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

size_t ladder_gmm_dense_workspace_bytes(int L, int B, int R, int K) {
  const size_t S = (size_t)L * B;
  const size_t gemm = ladder_igemm_fwd_workspace_bytes((long)S, R, K * R) > ladder_igemm_fwd_workspace_bytes((long)S, K * R, R)
                          ? ladder_igemm_fwd_workspace_bytes((long)S, R, K * R) : ladder_igemm_fwd_workspace_bytes((long)S, K * R, R);
  return ladder_round256(S * R * 4) * 2 + ladder_round256(S * K * R * 4) + ladder_round256(((S + 3) / 4) * 8) + ladder_round256(gemm) + 256;
}

int ladder_gmm_dense_logprob_fwd_bwd(const float* mu, const float* sd, const float* eps, const float* params, int L, int B, int R,
                                     int K, float* sum_logp, float* dmu, float* dsd, void* ws, size_t ws_bytes,
                                     ladder_stream_t stream) {
  if (L <= 0 || B <= 0 || K <= 0 || K > 1024 || R <= 0 || R > GD_MAXR || (R % 4) != 0) return LADDER_E_SHAPE;
  if (ws == nullptr || ws_bytes < ladder_gmm_dense_workspace_bytes(L, B, R, K)) return LADDER_E_WORKSPACE;
  const size_t S = (size_t)L * B;
  char* p = ladder_align256(ws);
  float* T = (float*)p;               p += ladder_round256(S * R * 4);
  float* dT = (float*)p;              p += ladder_round256(S * R * 4);
  float* Y = (float*)p;               p += ladder_round256(S * K * R * 4);
  double* lse = (double*)p;           p += ladder_round256(((S + 3) / 4) * 8);
  void* gws = p;
  const size_t gws_bytes = ws_bytes - (size_t)(p - (char*)ws);
  const float* Bmat = params;
  const float* BmatT = Bmat + (size_t)K * R * R;
  const float* bias = BmatT + (size_t)K * R * R;
  const float* logc = bias + (size_t)K * R;
  const size_t n = S * R;
  hipLaunchKernelGGL(mc_samples_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, mu, sd, eps, T, n, B * R);
  int rc = ladder_dense_fwd(T, Bmat, bias, Y, (int)S, R, K * R, LADDER_ACT_NONE, gws, gws_bytes, stream);
  if (rc != LADDER_OK) return rc;
  const int nblk = (int)((S + 3) / 4);
  hipLaunchKernelGGL(gmm_dense_resp_kernel, dim3(nblk), dim3(256), 4 * (size_t)K * sizeof(float), stream, Y, logc, (int)S, K, R,
                     dmu != nullptr ? 1 : 0, lse);
  hipLaunchKernelGGL(sum_doubles_kernel<float>, dim3(1), dim3(64), 0, stream, (const double*)lse, nblk, sum_logp);
  if (dmu != nullptr) {
    rc = ladder_dense_bwd_data(Y, BmatT, dT, (int)S, R, K * R, nullptr, 0, gws, gws_bytes, stream);
    if (rc != LADDER_OK) return rc;
    hipLaunchKernelGGL(gmm_dense_reduce_kernel, dim3((B * R + 255) / 256), dim3(256), 0, stream, dT, eps, dmu, dsd, L, B * R);
  }
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_gmm_dense_logprob_rows(const float* t, const float* params, int n, int R, int K, float* logp, void* ws, size_t ws_bytes,
                                  ladder_stream_t stream) {
  if (n <= 0 || K <= 0 || K > 1024 || R <= 0 || R > GD_MAXR || (R % 4) != 0) return LADDER_E_SHAPE;
  if (ws == nullptr || ws_bytes < ladder_gmm_dense_workspace_bytes(1, n, R, K)) return LADDER_E_WORKSPACE;
  const size_t S = (size_t)n;
  char* p = ladder_align256(ws);
  p += 2 * ladder_round256(S * R * 4);                                  // (T, dT of the training entry point: unused here)
  float* Y = (float*)p;               p += ladder_round256(S * K * R * 4);
  double* lse = (double*)p;           p += ladder_round256(((S + 3) / 4) * 8);
  void* gws = p;
  const size_t gws_bytes = ws_bytes - (size_t)(p - (char*)ws);
  const float* Bmat = params;
  const float* bias = Bmat + (size_t)2 * K * R * R;
  const float* logc = bias + (size_t)K * R;
  int rc = ladder_dense_fwd(t, Bmat, bias, Y, (int)S, R, K * R, LADDER_ACT_NONE, gws, gws_bytes, stream);
  if (rc != LADDER_OK) return rc;
  hipLaunchKernelGGL(gmm_dense_resp_kernel, dim3((unsigned)((S + 3) / 4)), dim3(256), 4 * (size_t)K * sizeof(float), stream, Y, logc, (int)S,
                     K, R, 0, lse, logp);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}
}  // extern "C"
