// FID evaluation on the device (reference codes/utils.py:127-200, `compute_FID_score` with FID_network == "VGG"): the pieces that the
// convolution kernels of this library do not already cover.
//
//   fid_preprocess_kernel   preprocess_input_original / preprocess_input_generated (utils.py:127-138) + tf.image.resize_images (utils.py:156-157,
//                           TF1 legacy bilinear) in one pass over uint8 or float images
//   maxpool2x2_kernel       the MaxPooling2D((2, 2), strides (2, 2)) behind each VGG16 block (utils.py:184-188)
//   global_pool_kernel      pooling = "avg" / "max" of the same Keras model
//   moments_*_kernel        streaming float64 mean / covariance of the activations: the statistics that
//                           tf.contrib.gan.eval.frechet_classifier_distance_from_activations (utils.py:197-199) forms from the whole activation matrix
//
// Streaming moments.  The state holds n, a shift vector c [D], s = sum (x - c) and S = sum (x - c)(x - c)^T, all doubles.  The first chunk sets c to
// its own column mean rounded to fp32, so x - c is exact in float64 and the products carry no uncentred cancellation.  S is a D x D x n contraction on
// v_mfma_f64_16x16x4_f64: M and N are column indices of x, K is the row.  Only the 64 x 64 tiles on and above the diagonal are computed (the reader mirrors);
// the rows of a chunk are split over blockIdx.y into partial tiles in the workspace, and a second kernel adds the partials to S in the fixed order
// split 0, 1, ... -- no atomics, so a given sequence of chunk sizes gives the same bits every time.
//
// Operand lane maps of v_mfma_f64_16x16x4_f64 (one double of A and of B per lane, four doubles of C/D):
//   A [m = lane & 15][k = lane >> 4],  B [k = lane >> 4][n = lane & 15],  C/D reg r: row m = (lane >> 4) + 4 r, col n = lane & 15
// (the C/D map differs from the fp32 16x16x4 form, whose row is 4 (lane >> 4) + r).
#include "common.h"

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int MODE_ORIGINAL = 0, MODE_GENERATED = 1;
constexpr int POOL_AVG = 0, POOL_MAX = 1;
constexpr int MOM_TILE = 64, MOM_TILE_ELEMS = MOM_TILE * MOM_TILE, MOM_MAX_SPLITS = 16, MOM_SPLIT_ROWS = 64, MOM_MAX_PARTIAL_TILES = 1024;
constexpr int MOM_HEAD = 2;        // state[0] = rows so far, state[1] = D (written with the shift; 0 before the first chunk)

// ------------------------------------------------------------------------------------------------ preprocess + resize
template <typename T>
__device__ __forceinline__ float fid_pre(T v, int mode) {
  float f = static_cast<float>(v);
  if (mode == MODE_ORIGINAL) f = f / 255.f;                           // x /= 255.
  else f = fminf(fmaxf(f, 0.f), 1.f);                                  // np.clip(x, 0., 1.)
  return (f - 0.5f) * 2.f;                                             // x -= 0.5; x *= 2.
}

// One thread per output pixel, C channels each.  src = dst * (in / out) in double (the quotient and the product as the float64 reference forms them),
// lo = floor(src), hi = min(lo + 1, in - 1), weights rounded to fp32.  A zero weight (every pixel of an integer down-scaling such as 128 -> 64) reads
// its low tap only, on either axis independently.
template <typename T>
__global__ __launch_bounds__(256) void fid_preprocess_kernel(const T* __restrict__ x, float* __restrict__ y, int N, int H, int W, int C, int OH, int OW,
                                                             int mode) {
  const size_t total = (size_t)N * OH * OW;
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= total) return;
  const int ox = (int)(p % OW), oy = (int)((p / OW) % OH);
  const size_t n = p / ((size_t)OW * OH);
  const double sy = oy * ((double)H / (double)OH), sx = ox * ((double)W / (double)OW);
  const int y0 = (int)floor(sy), x0 = (int)floor(sx);
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const float fy = (float)(sy - (double)y0), fx = (float)(sx - (double)x0);
  const T* r0 = x + (n * H + y0) * (size_t)W * C;
  const T* r1 = x + (n * H + y1) * (size_t)W * C;
  float* o = y + p * C;
  for (int c = 0; c < C; ++c) {
    float top = fid_pre(r0[(size_t)x0 * C + c], mode);
    if (fx != 0.f) top += (fid_pre(r0[(size_t)x1 * C + c], mode) - top) * fx;
    if (fy != 0.f) {
      float bot = fid_pre(r1[(size_t)x0 * C + c], mode);
      if (fx != 0.f) bot += (fid_pre(r1[(size_t)x1 * C + c], mode) - bot) * fx;
      top += (bot - top) * fy;
    }
    o[c] = top;
  }
}

// ------------------------------------------------------------------------------------------------ pools
template <typename V>
__device__ __forceinline__ V vmax(V a, V b);
template <>
__device__ __forceinline__ float vmax<float>(float a, float b) { return fmaxf(a, b); }
template <>
__device__ __forceinline__ float4 vmax<float4>(float4 a, float4 b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}

// y [N, H/2, W/2, CV] from x [N, H, W, CV] in units of V (float, or float4 when C % 4 == 0); the odd last row / column is dropped (VALID).
template <typename V>
__global__ __launch_bounds__(256) void maxpool2x2_kernel(const V* __restrict__ x, V* __restrict__ y, size_t total, int H, int W, int CV, int OH, int OW) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % CV);
  size_t q = i / CV;
  const int ox = (int)(q % OW);
  q /= OW;
  const int oy = (int)(q % OH);
  const size_t n = q / OH;
  const V* p = x + ((n * H + 2 * oy) * (size_t)W + 2 * ox) * CV + c;
  const size_t row = (size_t)W * CV;
  y[i] = vmax(vmax(p[0], p[CV]), vmax(p[row], p[row + CV]));
}

// y [N, C] from x [N, HW, C]: one thread per (n, c), the HW terms in index order (adjacent threads read adjacent channels).
__global__ __launch_bounds__(256) void global_pool_kernel(const float* __restrict__ x, float* __restrict__ y, size_t total, int HW, int C, int kind) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t n = i / C;
  const int c = (int)(i % C);
  const float* p = x + n * HW * (size_t)C + c;
  float acc = p[0];
  if (kind == POOL_MAX) {
    for (int k = 1; k < HW; ++k) acc = fmaxf(acc, p[(size_t)k * C]);
  } else {
    for (int k = 1; k < HW; ++k) acc += p[(size_t)k * C];
    acc = acc / (float)HW;
  }
  y[i] = acc;
}

// ------------------------------------------------------------------------------------------------ streaming moments
struct MomPlan {
  int ntd, ntiles, nsplit, rows;     // tiles per dimension, upper-triangular tiles, row splits, rows per split (a multiple of 4)
};

inline MomPlan mom_plan(int n, int D) {
  MomPlan p;
  p.ntd = (D + MOM_TILE - 1) / MOM_TILE;
  p.ntiles = p.ntd * (p.ntd + 1) / 2;
  int s = (n + MOM_SPLIT_ROWS - 1) / MOM_SPLIT_ROWS;
  const int cap = (MOM_MAX_PARTIAL_TILES + p.ntiles - 1) / p.ntiles;
  s = s < 1 ? 1 : s;
  s = s > MOM_MAX_SPLITS ? MOM_MAX_SPLITS : s;
  s = s > cap ? cap : s;
  p.rows = ((n + s - 1) / s + 3) / 4 * 4;
  p.nsplit = (n + p.rows - 1) / p.rows;
  if (p.nsplit < 1) p.nsplit = 1;
  return p;
}

// A state that already holds rows was laid out for the D in state[1]: a call with another D must not touch it through the wrong layout (uniform over a launch).
__device__ __forceinline__ bool mom_foreign(const double* state, int D) { return state[0] != 0.0 && state[1] != (double)D; }

// linear index of an upper-triangular tile -> (ti, tj), ti <= tj, rows enumerated first
__device__ __forceinline__ void mom_tile(int t, int ntd, int& ti, int& tj) {
  ti = 0;
  while (t >= ntd - ti) {
    t -= ntd - ti;
    ++ti;
  }
  tj = ti + t;
}

// First chunk only (state[0] == 0): c[j] = fp32 rounding of the chunk's column mean (float64 sum over the rows in index order).
__global__ __launch_bounds__(256) void moments_shift_kernel(const float* __restrict__ x, int n, int D, double* __restrict__ state) {
  if (state[0] != 0.0) return;                                     // (uniform over the launch: nothing writes state[0] here)
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= D) return;
  double acc = 0.0;
  for (int r = 0; r < n; ++r) acc += (double)x[(size_t)r * D + j];
  state[MOM_HEAD + j] = (double)(float)(acc / (double)n);
  if (j == 0) state[1] = (double)D;
}

// Partial tile (blockIdx.x = upper tile, blockIdx.y = row split): 4 wavefronts, wavefront w owns rows 16 w .. 16 w + 15 of the 64 x 64 tile as four
// 16 x 16 MFMA accumulators.  Operands come straight from global memory (a chunk is a few hundred rows: the traffic is nothing beside the feature
// network's), centred and widened on the way; rows past the split's end and columns past D enter as exact zeros AFTER centring.
__global__ __launch_bounds__(256) void moments_partial_kernel(const float* __restrict__ x, int n, int D, const double* __restrict__ state,
                                                              double* __restrict__ part, int ntd, int ntiles, int rows) {
  if (mom_foreign(state, D)) return;                               // (the whole launch: nothing is read through a wrong layout)
  int ti, tj;
  mom_tile(blockIdx.x, ntd, ti, tj);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, k = lane >> 4;
  const double* c = state + MOM_HEAD;
  const int ia = ti * MOM_TILE + wave * 16 + m;
  const bool va = ia < D;
  const double ca = va ? c[ia] : 0.0;
  int jb[4];
  bool vb[4];
  double cb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    jb[q] = tj * MOM_TILE + 16 * q + m;
    vb[q] = jb[q] < D;
    cb[q] = vb[q] ? c[jb[q]] : 0.0;
  }
  const int r0 = blockIdx.y * rows, r1 = min(n, r0 + rows);
  double4_t acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int r = r0; r < r1; r += 4) {                               // (uniform trip count: every lane reaches every MFMA)
    const int row = r + k;
    const bool ok = row < r1;
    const float* xr = x + (size_t)(ok ? row : r0) * D;             // (r0 < n whenever the loop runs: a valid row, never dereferenced unless ok)
    const double a = (ok && va) ? (double)xr[ia] - ca : 0.0;
    double b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = (ok && vb[q]) ? (double)xr[jb[q]] - cb[q] : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[q], acc[q], 0, 0, 0);
  }
  double* out = part + ((size_t)blockIdx.y * ntiles + blockIdx.x) * MOM_TILE_ELEMS;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int rg = 0; rg < 4; ++rg) out[(wave * 16 + k + 4 * rg) * MOM_TILE + 16 * q + m] = acc[q][rg];
}

// Blocks 0 .. 16 ntiles - 1: S += partials, split 0 first (256 elements of one tile per block).  The blocks behind them: s[j] += sum_r (x[r][j] - c[j]) over
// the rows in index order, one thread per column; the thread of column 0 also adds n to the row count (nothing in this launch reads it).
__global__ __launch_bounds__(256) void moments_reduce_kernel(const float* __restrict__ x, int n, int D, double* __restrict__ state,
                                                             const double* __restrict__ part, int ntd, int ntiles, int nsplit) {
  const int tile_blocks = ntiles * (MOM_TILE_ELEMS / 256);
  if (mom_foreign(state, D)) {                                      // refused on the device: the row count becomes NaN, nothing else is written
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 255) state[0] = __builtin_nan("");
    return;
  }
  if ((int)blockIdx.x < tile_blocks) {
    const int t = blockIdx.x / (MOM_TILE_ELEMS / 256), e = (blockIdx.x % (MOM_TILE_ELEMS / 256)) * 256 + threadIdx.x;
    int ti, tj;
    mom_tile(t, ntd, ti, tj);
    const int i = ti * MOM_TILE + e / MOM_TILE, j = tj * MOM_TILE + e % MOM_TILE;
    if (i >= D || j >= D) return;
    double acc = 0.0;
    for (int s = 0; s < nsplit; ++s) acc += part[((size_t)s * ntiles + t) * MOM_TILE_ELEMS + e];
    double* S = state + MOM_HEAD + 2 * (size_t)D;
    S[(size_t)i * D + j] += acc;
    return;
  }
  const int j = (blockIdx.x - tile_blocks) * 256 + threadIdx.x;
  if (j >= D) return;
  const double cj = state[MOM_HEAD + j];
  double acc = 0.0;
  for (int r = 0; r < n; ++r) acc += (double)x[(size_t)r * D + j] - cj;
  state[MOM_HEAD + D + j] += acc;
  if (j == 0) state[0] += (double)n;
}

}  // namespace

extern "C" {

int ladder_fid_preprocess(const void* x, int x_is_u8, float* y, int N, int H, int W, int C, int OH, int OW, int mode, ladder_stream_t stream) {
  if (x == nullptr || y == nullptr || N <= 0 || H <= 0 || W <= 0 || C != 3 || OH <= 0 || OW <= 0) return LADDER_E_SHAPE;
  if (mode != MODE_ORIGINAL && mode != MODE_GENERATED) return LADDER_E_SHAPE;
  const size_t total = (size_t)N * OH * OW, blocks = (total + 255) / 256;
  if (blocks >= (1ull << 31)) return LADDER_E_SHAPE;
  if (x_is_u8)
    hipLaunchKernelGGL(fid_preprocess_kernel<uint8_t>, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<const uint8_t*>(x), y, N, H, W, C, OH, OW, mode);
  else
    hipLaunchKernelGGL(fid_preprocess_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, stream, static_cast<const float*>(x), y, N, H, W, C, OH, OW, mode);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_maxpool2x2_fwd(const float* x, float* y, int N, int H, int W, int C, ladder_stream_t stream) {
  const int OH = H / 2, OW = W / 2;
  if (x == nullptr || y == nullptr || N <= 0 || C <= 0 || OH < 1 || OW < 1) return LADDER_E_SHAPE;
  const bool v4 = (C % 4 == 0) && ladder_aligned16(x) && ladder_aligned16(y);
  const int CV = v4 ? C / 4 : C;
  const size_t total = (size_t)N * OH * OW * CV, blocks = (total + 255) / 256;
  if (blocks >= (1ull << 31)) return LADDER_E_SHAPE;
  if (v4)
    hipLaunchKernelGGL(maxpool2x2_kernel<float4>, dim3((unsigned)blocks), dim3(256), 0, stream, reinterpret_cast<const float4*>(x), reinterpret_cast<float4*>(y),
                       total, H, W, CV, OH, OW);
  else
    hipLaunchKernelGGL(maxpool2x2_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, stream, x, y, total, H, W, CV, OH, OW);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_global_pool(const float* x, float* y, int N, int HW, int C, int kind, ladder_stream_t stream) {
  if (x == nullptr || y == nullptr || N <= 0 || HW <= 0 || C <= 0 || (kind != POOL_AVG && kind != POOL_MAX)) return LADDER_E_SHAPE;
  const size_t total = (size_t)N * C, blocks = (total + 255) / 256;
  if (blocks >= (1ull << 31)) return LADDER_E_SHAPE;
  hipLaunchKernelGGL(global_pool_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, y, total, HW, C, kind);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

size_t ladder_moments_state_doubles(int D) { return D < 1 ? 0 : (size_t)MOM_HEAD + 2 * (size_t)D + (size_t)D * D; }

size_t ladder_moments_workspace_bytes(int n, int D) {
  if (n < 1 || D < 1) return 0;
  const MomPlan p = mom_plan(n, D);
  return (size_t)p.nsplit * p.ntiles * MOM_TILE_ELEMS * sizeof(double);
}

int ladder_moments_accumulate(const float* x, int n, int D, double* state, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (x == nullptr || state == nullptr || n < 0 || D < 1 || D > 32768) return LADDER_E_SHAPE;
  if (n == 0) return LADDER_OK;
  if ((reinterpret_cast<uintptr_t>(state) & 7u) || (reinterpret_cast<uintptr_t>(ws) & 7u)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_moments_workspace_bytes(n, D)) return LADDER_E_WORKSPACE;
  const MomPlan p = mom_plan(n, D);
  const int col_blocks = (D + 255) / 256;
  hipLaunchKernelGGL(moments_shift_kernel, dim3(col_blocks), dim3(256), 0, stream, x, n, D, state);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(moments_partial_kernel, dim3(p.ntiles, p.nsplit), dim3(256), 0, stream, x, n, D, state, static_cast<double*>(ws), p.ntd, p.ntiles, p.rows);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(moments_reduce_kernel, dim3(p.ntiles * (MOM_TILE_ELEMS / 256) + col_blocks), dim3(256), 0, stream, x, n, D, state,
                     static_cast<const double*>(ws), p.ntd, p.ntiles, p.nsplit);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
