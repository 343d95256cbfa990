// Ancestral sampling of the priors on the device and byte packing of generated images (include/ladder_hip.h, section N15).
//
// Parameter buffer of a sampler (ladder_mixture_sample_param_bytes(K, R) bytes, 16-byte aligned):
//   bytes [0, 16)                       int32 status | int32 K | int32 R | int32 0
//   bytes [16, 16 + 8K)                 float64 cdf[K]: cdf_k = (w'_0 + ... + w'_k) / (w'_0 + ... + w'_{K-1}), w'_k = max((double)w_k, 0),
//                                       both sums formed sequentially in index order; padded to a multiple of 16 bytes
//   then K * R float32                  means[k][r]
//   then K * R(R+1)/2 float32           L_k, lower-triangular, row-major (row i starts at i(i+1)/2): the float64 Cholesky factor of cov_k rounded
//                                       to fp32; the whole float region padded to a multiple of 16 bytes
//   status: -1 = usable; k >= 0 = first component whose factorisation met a non-positive (or NaN) pivot; -2 = the weights have no
//   positive finite sum.
// ladder_mixture_sample compares the header with its own K and R on the device before it reads anything else: a buffer that is not
// usable, or was prepared for another (K, R), gives out = NaN and comp = -1 for every sample instead of a read through a wrong layout.
//
// Philox mode of ladder_mixture_sample (u == eps == NULL): sample index i (global: first + row) draws from generator blocks
//   counter = { lo32(i), (i >> 32) | (b << 24), lo32(offset), hi32(offset) },  key = seed,        i < 2^56
//   b = 1:            u_i = (word 0 >> 8) * 2^-24   (in [0, 1))
//   b = 2 + j / 4:    eps_i[4 (b-2) .. 4 (b-2) + 3] = the four Box-Muller normals of the block (philox.h)
// so the draws of sample i depend on (seed, offset, i) only -- not on n, first or the launch grid.  ladder_randn uses b = 0 of the same
// counter space (its block index stays below 2^56), so the two never share a block under one (seed, offset).
//
// WIDE samplers (ladder_mixture_sample_wide*: 64 < R <= 256, R % 16 == 0) keep this buffer layout, this output definition and this counter
// layout (b = 2 + j / 4 reaches 65 at R = 256, inside its 8 bits); their factorisation is the panel one of chol_wide.h in a caller-provided
// workspace, and a sample's rows r = lane, lane + 64, ... are spread over the lanes of one wavefront with eps staged in LDS.
#include "common.h"
#include "chol_wide.h"
#include "philox.h"

namespace {

constexpr int SAMPLE_MAX_R = 64;
constexpr size_t SAMPLE_LDS_LIMIT = 48 * 1024;
constexpr long long SAMPLE_MAX_INDEX = 1ll << 56;

__host__ __device__ inline size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
__host__ __device__ inline size_t sample_off_means(int K) { return 16 + align16((size_t)K * 8); }
__host__ __device__ inline size_t sample_tri(int R) { return (size_t)R * (R + 1) / 2; }
__host__ __device__ inline size_t sample_bytes(int K, int R) {
  return sample_off_means(K) + align16((size_t)K * ((size_t)R + sample_tri(R)) * 4);
}

// header, cumulative distribution and means.  weights == NULL: K equal weights; means row-major [K, R].
__global__ void sample_header_kernel(const float* __restrict__ weights, const float* __restrict__ means, int K, int R, unsigned char* params) {
  int* head = reinterpret_cast<int*>(params);
  double* cdf = reinterpret_cast<double*>(params + 16);
  float* m = reinterpret_cast<float*>(params + sample_off_means(K));
  if (threadIdx.x == 0) {
    double run = 0.0;
    for (int k = 0; k < K; ++k) {
      const double w = weights != nullptr ? (double)weights[k] : 1.0;
      run += w > 0.0 ? w : 0.0;                       // (NaN compares false: counts as 0)
      cdf[k] = run;
    }
    const double total = run;
    for (int k = 0; k < K; ++k) cdf[k] = cdf[k] / total;
    head[0] = (total > 0.0 && total <= 1.7e308) ? -1 : -2;
    head[1] = K;
    head[2] = R;
    head[3] = 0;
  }
  for (int i = threadIdx.x; i < K * R; i += blockDim.x) m[i] = means[i];
}

// One workgroup (one wavefront) per component: left-looking Cholesky in float64 on the lower triangle held in LDS; column j = the pivot by
// every lane (same sequential sum), then the rows below it one per lane.
__global__ __launch_bounds__(64) void sample_chol_kernel(const float* __restrict__ covs, int K, int R, unsigned char* params) {
  __shared__ double A[SAMPLE_MAX_R * (SAMPLE_MAX_R + 1) / 2];
  __shared__ int bad;
  const int k = blockIdx.x, lane = threadIdx.x;
  const int T = (int)sample_tri(R);
  const float* c = covs + (size_t)k * R * R;
  for (int i = lane; i < R; i += 64)
    for (int j = 0; j <= i; ++j) A[i * (i + 1) / 2 + j] = (double)c[i * R + j];
  if (lane == 0) bad = 0;
  __syncthreads();
  for (int j = 0; j < R; ++j) {
    const double* rj = A + j * (j + 1) / 2;
    double d = rj[j];
    for (int q = 0; q < j; ++q) d -= rj[q] * rj[q];
    if (!(d > 0.0)) {                                   // uniform over the wavefront
      if (lane == 0) bad = 1;
      break;
    }
    const double piv = sqrt(d);
    __syncthreads();                                    // every lane has read the old diagonal
    for (int i = j + lane; i < R; i += 64) {
      double* ri = A + i * (i + 1) / 2;
      if (i == j) {
        ri[j] = piv;
      } else {
        double s = ri[j];
        for (int q = 0; q < j; ++q) s -= ri[q] * rj[q];
        ri[j] = s / piv;
      }
    }
    __syncthreads();
  }
  __syncthreads();
  float* Lk = reinterpret_cast<float*>(params + sample_off_means(K)) + (size_t)K * R + (size_t)k * T;
  const bool failed = bad != 0;
  for (int i = lane; i < T; i += 64) Lk[i] = failed ? 0.f : (float)A[i];
  if (failed && lane == 0) atomicMin(reinterpret_cast<unsigned*>(params), (unsigned)k);      // (-1 and -2 are the largest unsigned values)
}

// diagonal components: L_k = diag(sd_k); a non-positive (or NaN) standard deviation is a non-positive pivot
__global__ void sample_diag_kernel(const float* __restrict__ sd, int K, int R, unsigned char* params) {
  const int k = blockIdx.x;
  const int T = (int)sample_tri(R);
  float* Lk = reinterpret_cast<float*>(params + sample_off_means(K)) + (size_t)K * R + (size_t)k * T;
  for (int i = threadIdx.x; i < T; i += blockDim.x) Lk[i] = 0.f;
  __syncthreads();
  bool failed = false;
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    const float s = sd[(size_t)k * R + r];
    if (!(s > 0.f)) failed = true;
    Lk[r * (r + 1) / 2 + r] = s;
  }
  if (failed) atomicMin(reinterpret_cast<unsigned*>(params), (unsigned)k);
}

// number of cdf_j <= u, clamped to K - 1 (np.searchsorted(cdf, u, side="right"))
__device__ __forceinline__ int sample_component(const double* cdf, int K, double u) {
  int lo = 0, hi = K;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cdf[mid] <= u) lo = mid + 1; else hi = mid;
  }
  return lo < K - 1 ? lo : K - 1;
}

// the buffer is usable and was prepared for this (K, R); uniform over the grid
__device__ __forceinline__ bool sample_header_ok(const unsigned char* params, int K, int R) {
  const int4 head = *reinterpret_cast<const int4*>(params);
  return head.x == -1 && head.y == K && head.z == R;
}
__device__ __forceinline__ float sample_nan() { return __int_as_float(0x7fc00000); }

__device__ __forceinline__ void sample_block(uint32_t (&c)[4], long long i, uint32_t b, uint64_t seed, uint64_t offset) {
  c[0] = (uint32_t)i;
  c[1] = (uint32_t)((unsigned long long)i >> 32) | (b << 24);
  c[2] = (uint32_t)offset;
  c[3] = (uint32_t)(offset >> 32);
  philox4x32_10(c, seed);
}
__device__ __forceinline__ float sample_uniform(long long i, uint64_t seed, uint64_t offset) {
  uint32_t c[4];
  sample_block(c, i, 1u, seed, offset);
  return (float)(c[0] >> 8) * (1.0f / 16777216.0f);
}

// R <= 8: one thread per sample, the prepared parameters staged in LDS (STAGE) or read in place when they exceed SAMPLE_LDS_LIMIT
template <int R, bool STAGE>
__global__ __launch_bounds__(256) void sample_thread_kernel(const unsigned char* __restrict__ params, int K, int n, long long first,
                                                            const float* __restrict__ u_in, const float* __restrict__ eps_in, uint64_t seed,
                                                            uint64_t offset, float* __restrict__ out, int* __restrict__ comp) {
  extern __shared__ uint4 sample_lds[];
  if (!sample_header_ok(params, K, R)) {                 // (the whole workgroup leaves: no barrier is left behind)
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row < n) {
      for (int r = 0; r < R; ++r) out[(size_t)row * R + r] = sample_nan();
      if (comp != nullptr) comp[row] = -1;
    }
    return;
  }
  const unsigned char* base = params + 16;
  if (STAGE) {
    const int words = (int)((sample_bytes(K, R) - 16) / 16);
    const uint4* src = reinterpret_cast<const uint4*>(base);
    for (int i = threadIdx.x; i < words; i += blockDim.x) sample_lds[i] = src[i];
    __syncthreads();
    base = reinterpret_cast<const unsigned char*>(sample_lds);
  }
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const double* cdf = reinterpret_cast<const double*>(base);
  const float* means = reinterpret_cast<const float*>(base + sample_off_means(K) - 16);
  constexpr int T = R * (R + 1) / 2;
  const float* Ls = means + (size_t)K * R;
  const long long i = first + row;
  float u, eps[R];
  if (u_in != nullptr) {
    u = u_in[row];
#pragma unroll
    for (int j = 0; j < R; ++j) eps[j] = eps_in[(size_t)row * R + j];
  } else {
    u = sample_uniform(i, seed, offset);
#pragma unroll
    for (int b = 0; b < (R + 3) / 4; ++b) {
      uint32_t c[4];
      float o[4];
      sample_block(c, i, 2u + b, seed, offset);
      philox_box_muller4(c, o);
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (4 * b + j < R) eps[4 * b + j] = o[j];
    }
  }
  const int k = sample_component(cdf, K, (double)u);
  const float* m = means + (size_t)k * R;
  const float* Lk = Ls + (size_t)k * T;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    float acc = m[r];
#pragma unroll
    for (int j = 0; j <= r; ++j) acc = fmaf(Lk[r * (r + 1) / 2 + j], eps[j], acc);
    out[(size_t)row * R + r] = acc;
  }
  if (comp != nullptr) comp[row] = k;
}

// 8 < R <= 64: one wavefront per sample, lane r = row r of L_k; eps_j travels from lane j by a wave shuffle
__global__ __launch_bounds__(256) void sample_wave_kernel(const unsigned char* __restrict__ params, int K, int R, int n, long long first,
                                                          const float* __restrict__ u_in, const float* __restrict__ eps_in, uint64_t seed,
                                                          uint64_t offset, float* __restrict__ out, int* __restrict__ comp) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (row >= n) return;                                  // (whole wavefronts leave together)
  if (!sample_header_ok(params, K, R)) {
    if (lane < R) out[(size_t)row * R + lane] = sample_nan();
    if (comp != nullptr && lane == 0) comp[row] = -1;
    return;
  }
  const double* cdf = reinterpret_cast<const double*>(params + 16);
  const float* means = reinterpret_cast<const float*>(params + sample_off_means(K));
  const float* Ls = means + (size_t)K * R;
  const long long i = first + row;
  const int r = lane < R ? lane : R - 1;                 // idle lanes shadow the last row (no store)
  float u, e;
  if (u_in != nullptr) {
    u = u_in[row];
    e = eps_in[(size_t)row * R + r];
  } else {
    u = sample_uniform(i, seed, offset);
    uint32_t c[4];
    float o[4];
    sample_block(c, i, 2u + (uint32_t)(r >> 2), seed, offset);
    philox_box_muller4(c, o);
    e = (r & 3) == 0 ? o[0] : (r & 3) == 1 ? o[1] : (r & 3) == 2 ? o[2] : o[3];
  }
  const int k = sample_component(cdf, K, (double)u);
  const float* Lr = Ls + (size_t)k * sample_tri(R) + (size_t)r * (r + 1) / 2;
  float acc = means[(size_t)k * R + r];
  for (int j = 0; j < R; ++j) {
    const float ej = __shfl(e, j, 64);
    if (j <= r) acc = fmaf(Lr[j], ej, acc);
  }
  if (lane < R) out[(size_t)row * R + lane] = acc;
  if (comp != nullptr && lane == 0) comp[row] = k;
}

// ---- wide samplers -------------------------------------------------------------------------------------------------------------
// Workgroup b factors the components b, b + gridDim.x, ... in its slot of the workspace and rounds the lower triangle into the buffer.
__global__ __launch_bounds__(CW_THREADS) void sample_chol_wide_kernel(const float* __restrict__ covs, int K, int R, unsigned char* params, double* ws) {
  __shared__ CwShared sh;
  const int tid = threadIdx.x;
  const int T = (int)sample_tri(R);
  double* W = ws + (size_t)blockIdx.x * R * R;
  for (int k = blockIdx.x; k < K; k += gridDim.x) {
    __syncthreads();                                     // (the previous component's W is no longer read)
    const bool failed = chol_wide_factor<false>(covs + (size_t)k * R * R, R, W, sh);
    float* Lk = reinterpret_cast<float*>(params + sample_off_means(K)) + (size_t)K * R + (size_t)k * T;
    for (int e = tid; e < R * R; e += CW_THREADS) {
      const int i = e / R, j = e - i * R;
      if (j <= i) Lk[i * (i + 1) / 2 + j] = failed ? 0.f : (float)W[e];
    }
    if (failed && tid == 0) atomicMin(reinterpret_cast<unsigned*>(params), (unsigned)k);
  }
}

// One wavefront per sample, 4 per workgroup; lane l owns the rows l, l + 64, l + 128, l + 192 below R.
__global__ __launch_bounds__(256) void sample_wide_kernel(const unsigned char* __restrict__ params, int K, int R, int n, long long first,
                                                          const float* __restrict__ u_in, const float* __restrict__ eps_in, uint64_t seed,
                                                          uint64_t offset, float* __restrict__ out, int* __restrict__ comp) {
  __shared__ float s_eps[4][CW_MAXR];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int row = blockIdx.x * 4 + wv;
  const bool live = row < n;                             // (whole wavefronts; they stay for the barrier)
  const bool ok = sample_header_ok(params, K, R);
  float u = 0.f;
  if (live && ok) {
    const long long i = first + row;
    if (u_in != nullptr) {
      u = u_in[row];
      for (int j = lane; j < R; j += 64) s_eps[wv][j] = eps_in[(size_t)row * R + j];
    } else {
      u = sample_uniform(i, seed, offset);
      if (4 * lane < R) {                                // generator block 2 + lane: eps[4 lane .. 4 lane + 3]  (R % 4 == 0)
        uint32_t c[4];
        float o[4];
        sample_block(c, i, 2u + (uint32_t)lane, seed, offset);
        philox_box_muller4(c, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) s_eps[wv][4 * lane + j] = o[j];
      }
    }
  }
  __syncthreads();
  if (!live) return;
  if (!ok) {
    for (int r = lane; r < R; r += 64) out[(size_t)row * R + r] = sample_nan();
    if (comp != nullptr && lane == 0) comp[row] = -1;
    return;
  }
  const double* cdf = reinterpret_cast<const double*>(params + 16);
  const float* means = reinterpret_cast<const float*>(params + sample_off_means(K));
  const float* Ls = means + (size_t)K * R;
  const int k = sample_component(cdf, K, (double)u);
  const float* Lk = Ls + (size_t)k * sample_tri(R);
  const float* e = s_eps[wv];
  for (int r = lane; r < R; r += 64) {
    const float* Lr = Lk + (size_t)r * (r + 1) / 2;
    float acc = means[(size_t)k * R + r];
    for (int j = 0; j <= r; ++j) acc = fmaf(Lr[j], e[j], acc);
    out[(size_t)row * R + r] = acc;
  }
  if (comp != nullptr && lane == 0) comp[row] = k;
}

int wide_prepare_checks(const void* a, const void* b, int K, int R, const void* params) {
  if (K < 1 || !cw_width_ok(R) || a == nullptr || b == nullptr || params == nullptr) return LADDER_E_SHAPE;
  if (!ladder_aligned16(a) || !ladder_aligned16(b) || !ladder_aligned16(params)) return LADDER_E_ALIGN;
  return LADDER_OK;
}

__device__ __forceinline__ unsigned u8_of(float v) { return (unsigned)rintf(255.f * fminf(fmaxf(v, 0.f), 1.f)); }   // (fmaxf(NaN, 0) = 0)
__device__ __forceinline__ unsigned u8_pack(float4 v) { return u8_of(v.x) | (u8_of(v.y) << 8) | (u8_of(v.z) << 16) | (u8_of(v.w) << 24); }

// 16 pixels per step: four 16-byte loads, one 16-byte store; the (n % 16) tail by the first threads of the grid
__global__ __launch_bounds__(256) void images_to_u8_kernel(const float* __restrict__ x, unsigned char* __restrict__ out, size_t n) {
  const size_t groups = n / 16;
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const float4* x4 = reinterpret_cast<const float4*>(x);
  uint4* o4 = reinterpret_cast<uint4*>(out);
  for (size_t g = tid; g < groups; g += stride) {
    const float4 a = x4[4 * g], b = x4[4 * g + 1], c = x4[4 * g + 2], d = x4[4 * g + 3];
    o4[g] = make_uint4(u8_pack(a), u8_pack(b), u8_pack(c), u8_pack(d));
  }
  const size_t t = groups * 16 + tid;
  if (t < n) out[t] = (unsigned char)u8_of(x[t]);
}

template <bool STAGE>
void launch_thread(int R, dim3 grid, size_t lds, hipStream_t st, const unsigned char* params, int K, int n, long long first, const float* u,
                   const float* eps, uint64_t seed, uint64_t offset, float* out, int* comp) {
#define LADDER_SAMPLE_CASE(RR)                                                                                                              \
  case RR:                                                                                                                                  \
    hipLaunchKernelGGL((sample_thread_kernel<RR, STAGE>), grid, dim3(256), lds, st, params, K, n, first, u, eps, seed, offset, out, comp); \
    break;
  switch (R) {
    LADDER_SAMPLE_CASE(1) LADDER_SAMPLE_CASE(2) LADDER_SAMPLE_CASE(3) LADDER_SAMPLE_CASE(4)
    LADDER_SAMPLE_CASE(5) LADDER_SAMPLE_CASE(6) LADDER_SAMPLE_CASE(7) LADDER_SAMPLE_CASE(8)
  }
#undef LADDER_SAMPLE_CASE
}

int prepare_checks(const void* a, const void* b, int K, int R, const void* params) {
  if (K < 1 || R < 1 || R > SAMPLE_MAX_R || a == nullptr || b == nullptr || params == nullptr) return LADDER_E_SHAPE;
  if (!ladder_aligned16(a) || !ladder_aligned16(b) || !ladder_aligned16(params)) return LADDER_E_ALIGN;
  return LADDER_OK;
}

}  // namespace

extern "C" {

size_t ladder_mixture_sample_param_bytes(int K, int R) {
  if (K < 1 || R < 1 || R > SAMPLE_MAX_R) return 0;
  return sample_bytes(K, R);
}

int ladder_mixture_sample_prepare(const float* weights, const float* means, const float* covs, int K, int R, void* params,
                                  ladder_stream_t stream) {
  if (weights == nullptr) return LADDER_E_SHAPE;
  if (const int rc = prepare_checks(means, covs, K, R, params)) return rc;
  if (!ladder_aligned16(weights)) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(sample_header_kernel, dim3(1), dim3(256), 0, stream, weights, means, K, R, (unsigned char*)params);
  hipLaunchKernelGGL(sample_chol_kernel, dim3(K), dim3(64), 0, stream, covs, K, R, (unsigned char*)params);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_mixture_sample_prepare_diag(const float* comp_mean, const float* comp_sd, int K, int R, void* params, ladder_stream_t stream) {
  if (const int rc = prepare_checks(comp_mean, comp_sd, K, R, params)) return rc;
  hipLaunchKernelGGL(sample_header_kernel, dim3(1), dim3(256), 0, stream, (const float*)nullptr, comp_mean, K, R, (unsigned char*)params);
  hipLaunchKernelGGL(sample_diag_kernel, dim3(K), dim3(64), 0, stream, comp_sd, K, R, (unsigned char*)params);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_mixture_sample(const void* params, int K, int R, int n, int64_t first, const float* u, const float* eps, uint64_t seed,
                          uint64_t offset, float* out, int* comp, ladder_stream_t stream) {
  if (K < 1 || R < 1 || R > SAMPLE_MAX_R || n < 0 || first < 0 || first > SAMPLE_MAX_INDEX - n) return LADDER_E_SHAPE;
  if ((u == nullptr) != (eps == nullptr)) return LADDER_E_SHAPE;          // both fed or both drawn
  if (n == 0) return LADDER_OK;
  if (params == nullptr || out == nullptr) return LADDER_E_SHAPE;
  if (!ladder_aligned16(params) || !ladder_aligned16(out) || !ladder_aligned16(u) || !ladder_aligned16(eps) || !ladder_aligned16(comp))
    return LADDER_E_ALIGN;
  const unsigned char* p = (const unsigned char*)params;
  if (R <= 8) {
    const size_t lds = sample_bytes(K, R) - 16;
    const dim3 grid((unsigned)(((size_t)n + 255) / 256));
    if (lds <= SAMPLE_LDS_LIMIT)
      launch_thread<true>(R, grid, lds, stream, p, K, n, first, u, eps, seed, offset, out, comp);
    else
      launch_thread<false>(R, grid, 0, stream, p, K, n, first, u, eps, seed, offset, out, comp);
  } else {
    hipLaunchKernelGGL(sample_wave_kernel, dim3((unsigned)(((size_t)n + 3) / 4)), dim3(256), 0, stream, p, K, R, n, first, u, eps, seed, offset, out,
                       comp);
  }
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

size_t ladder_mixture_sample_wide_param_bytes(int K, int R) {
  if (K < 1 || !cw_width_ok(R)) return 0;
  return sample_bytes(K, R);
}

size_t ladder_mixture_sample_wide_prepare_workspace_bytes(int K, int R) { return cw_workspace_bytes(K, R); }

int ladder_mixture_sample_wide_prepare(const float* weights, const float* means, const float* covs, int K, int R, void* params, void* ws,
                                       size_t ws_bytes, ladder_stream_t stream) {
  if (weights == nullptr) return LADDER_E_SHAPE;
  if (const int rc = wide_prepare_checks(means, covs, K, R, params)) return rc;
  if (!ladder_aligned16(weights)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < cw_workspace_bytes(K, R)) return LADDER_E_WORKSPACE;
  hipLaunchKernelGGL(sample_header_kernel, dim3(1), dim3(256), 0, stream, weights, means, K, R, (unsigned char*)params);
  hipLaunchKernelGGL(sample_chol_wide_kernel, dim3(cw_slots(K)), dim3(CW_THREADS), 0, stream, covs, K, R, (unsigned char*)params, cw_workspace_base(ws));
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_mixture_sample_wide_prepare_diag(const float* comp_mean, const float* comp_sd, int K, int R, void* params, ladder_stream_t stream) {
  if (const int rc = wide_prepare_checks(comp_mean, comp_sd, K, R, params)) return rc;
  hipLaunchKernelGGL(sample_header_kernel, dim3(1), dim3(256), 0, stream, (const float*)nullptr, comp_mean, K, R, (unsigned char*)params);
  hipLaunchKernelGGL(sample_diag_kernel, dim3(K), dim3(64), 0, stream, comp_sd, K, R, (unsigned char*)params);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_mixture_sample_wide(const void* params, int K, int R, int n, int64_t first, const float* u, const float* eps, uint64_t seed,
                               uint64_t offset, float* out, int* comp, ladder_stream_t stream) {
  if (K < 1 || !cw_width_ok(R) || n < 0 || first < 0 || first > SAMPLE_MAX_INDEX - n) return LADDER_E_SHAPE;
  if ((u == nullptr) != (eps == nullptr)) return LADDER_E_SHAPE;          // both fed or both drawn
  if (n == 0) return LADDER_OK;
  if (params == nullptr || out == nullptr) return LADDER_E_SHAPE;
  if (!ladder_aligned16(params) || !ladder_aligned16(out) || !ladder_aligned16(u) || !ladder_aligned16(eps) || !ladder_aligned16(comp))
    return LADDER_E_ALIGN;
  hipLaunchKernelGGL(sample_wide_kernel, dim3((unsigned)(((size_t)n + 3) / 4)), dim3(256), 0, stream, (const unsigned char*)params, K, R, n,
                     (long long)first, u, eps, seed, offset, out, comp);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_images_to_u8(const float* x, uint8_t* out, size_t n, ladder_stream_t stream) {
  if (n == 0) return LADDER_OK;
  if (x == nullptr || out == nullptr) return LADDER_E_SHAPE;
  if (!ladder_aligned16(x) || !ladder_aligned16(out)) return LADDER_E_ALIGN;
  size_t blocks = (n / 16 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 8192) blocks = 8192;                 // grid-stride beyond 2^21 threads x 16 pixels
  hipLaunchKernelGGL(images_to_u8_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, out, n);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
