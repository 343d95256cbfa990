// Importance-weighted marginal log-likelihood, log p(x) ~ log (1/S) sum_s w_s (DESIGN.md "Importance-weighted log-likelihood"): the per-ROW terms of
// the log-weights and the streaming log-sum-exp over the samples of an image.  The decoder passes that produce xhat dominate the run; these kernels only
// have to be exact.  Rows are image-major: row r = b * C + c is sample c of image b of the current chunk, `per` is the number of rows per parent row.
//
//   randn_rows      the estimator's noise: element (image, sample, j) of a level draws from its own Philox counter, whatever the chunking.
//   sample_rows     z = mu + sd * eps (the fp32 fmaf of the training path) and log q = -1/2 sum eps^2 - sum log sd - W/2 log 2pi.
//   laplace_rows    log p(x|z) = -sum_d |x_d - xhat_d| / sigma - D log(2 sigma) (define_loss, codes/base.py:383-396).  A workgroup per row when the rows fill
//                   the chip, else a (row, slice) grid whose float64 partials a second launch adds in slice order.
//   gauss_rows      -sum (a - b)^2 / (2 s^2) - W log s - W/2 log 2pi.
//   add_term        logw (+)= sign * term, term fp32 or float64.
//   accumulate / finish   per image: running maximum M, sum exp(logw - M), sum exp(2 (logw - M)), sum logw, count -> log_px, elbo_1, ess, S.
//
// Row values are float64: at 49 152 pixels log p(x|z) is of order 1e4 - 1e5 and differences of order 1 between samples decide the estimate.  Inputs are the
// engine's fp32 tensors; differences, squares and sums are formed in float64.  Every sum has one fixed order (lane-strided partial sums, a shuffle tree, the
// wavefronts of a workgroup in index order): no atomics, two calls on the same inputs give the same bits.
#include "common.h"
#include "philox.h"

namespace {
constexpr double kHalfLog2PiD = 0.918938533204672741780329736406;
constexpr int IW_CUS = 256;                    // a row per workgroup fills the chip from this many rows on
constexpr int IW_SLICE_FLOATS = 1024;          // granularity of a slice of a row: whole 16-byte groups for every thread of the workgroup
constexpr int IW_MAX_SLICES = 64;              // the second pass adds a row's partials with one wavefront
constexpr int IW_MAX_D = 1 << 22, IW_MAX_W = 1 << 16, IW_MAX_ROWS = 1 << 24;

bool iw_aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// ---------------------------------------------------------------------------------------------------------------- noise
// out[(b * C + c) * W + j]: counter = (block j / 4 | level << 28, sample, image lo, image hi) under the key `seed`.
__global__ __launch_bounds__(256) void iw_randn_rows_kernel(float* __restrict__ out, long n_rows, int C, int W, unsigned long long image0,
                                                            unsigned long long sample0, uint64_t seed, uint32_t level) {
  const int qw = (W + 3) >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rows * qw) return;
  const long r = i / qw;
  const int q = (int)(i - r * qw);
  const unsigned long long img = image0 + (unsigned long long)(r / C), smp = sample0 + (unsigned long long)(r % C);
  uint32_t c[4] = {(uint32_t)q | (level << 28), (uint32_t)smp, (uint32_t)img, (uint32_t)(img >> 32)};
  philox4x32_10(c, seed);
  float o[4];
  philox_box_muller4(c, o);
  for (int j = 0; j < 4; ++j)
    if (4 * q + j < W) out[(size_t)r * W + 4 * q + j] = o[j];
}

// ---------------------------------------------------------------------------------------------------------------- row terms
__global__ __launch_bounds__(256) void iw_sample_rows_kernel(const float* __restrict__ mu, const float* __restrict__ sd, const float* __restrict__ eps,
                                                             int n, int per, int W, float* __restrict__ sample, double* __restrict__ logq) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;                                  // wavefront-uniform
  const size_t p = (size_t)(r / per) * W, o = (size_t)r * W;
  double se = 0.0, sl = 0.0;
  for (int j = lane; j < W; j += 64) {
    const float e = eps[o + j], s = sd[p + j];
    sample[o + j] = fmaf(s, e, mu[p + j]);
    se += (double)e * (double)e;
    sl += log((double)s);
  }
  se = wave_sum_d(se);
  sl = wave_sum_d(sl);
  if (lane == 0) logq[r] = -0.5 * se - sl - (double)W * kHalfLog2PiD;
}

__global__ __launch_bounds__(256) void iw_gauss_rows_kernel(const float* __restrict__ a, const float* __restrict__ b, double s, int n, int W,
                                                            double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const size_t o = (size_t)r * W;
  double acc = 0.0;
  for (int j = lane; j < W; j += 64) {
    const double d = (double)a[o + j] - (b != nullptr ? (double)b[o + j] : 0.0);
    acc += d * d;
  }
  acc = wave_sum_d(acc);
  if (lane == 0) out[r] = -acc / (2.0 * s * s) - (double)W * log(s) - (double)W * kHalfLog2PiD;
}

// sum_d |x_d - xhat_d| over floats [d0, d1) of row r: VEC takes 16-byte groups (D % 4 == 0, both bases on 16 bytes, d0 a multiple of 4).
template <bool VEC>
__device__ __forceinline__ double iw_abs_sum(const float* __restrict__ xr, const float* __restrict__ hr, int d0, int d1) {
  double acc = 0.0;
  if (VEC) {
    const float4* x4 = reinterpret_cast<const float4*>(xr);
    const float4* h4 = reinterpret_cast<const float4*>(hr);
    for (int q = (d0 >> 2) + threadIdx.x; q < (d1 >> 2); q += 256) {
      const float4 u = x4[q], v = h4[q];
      acc += (fabs((double)u.x - (double)v.x) + fabs((double)u.y - (double)v.y)) + (fabs((double)u.z - (double)v.z) + fabs((double)u.w - (double)v.w));
    }
  } else {
    for (int d = d0 + threadIdx.x; d < d1; d += 256) acc += fabs((double)xr[d] - (double)hr[d]);
  }
  __shared__ double red[4];
  acc = wave_sum_d(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// grid (rows, slices).  slices == 1: the row's value goes to out; else the slice's sum to part[r * slices + slice].
template <bool VEC>
__global__ __launch_bounds__(256) void iw_laplace_rows_kernel(const float* __restrict__ x, const float* __restrict__ xhat, int per, int D, int chunk,
                                                              double sigma, double* __restrict__ out, double* __restrict__ part) {
  const int r = blockIdx.x, sl = blockIdx.y, slices = gridDim.y;
  const int d0 = sl * chunk, d1 = d0 + chunk < D ? d0 + chunk : D;
  const double a = iw_abs_sum<VEC>(x + (size_t)(r / per) * D, xhat + (size_t)r * D, d0, d1);
  if (threadIdx.x == 0) {
    if (slices == 1) out[r] = -a / sigma - (double)D * log(2.0 * sigma);
    else part[(size_t)r * slices + sl] = a;
  }
}
__global__ __launch_bounds__(256) void iw_laplace_finish_kernel(const double* __restrict__ part, int n, int slices, int D, double sigma,
                                                                double* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  const double a = wave_sum_d(lane < slices ? part[(size_t)r * slices + lane] : 0.0);    // slices <= 64
  if (lane == 0) out[r] = -a / sigma - (double)D * log(2.0 * sigma);
}

struct LapPlan { int slices, chunk; size_t bytes; };
LapPlan lap_plan(int n, int D) {
  LapPlan p;
  int want = n >= IW_CUS ? 1 : (IW_CUS + n - 1) / n;
  want = want > IW_MAX_SLICES ? IW_MAX_SLICES : want;
  p.chunk = ((D + want - 1) / want + IW_SLICE_FLOATS - 1) / IW_SLICE_FLOATS * IW_SLICE_FLOATS;
  p.slices = (D + p.chunk - 1) / p.chunk;                    // no empty slice
  p.bytes = p.slices == 1 ? 0 : ladder_round256((size_t)n * p.slices * sizeof(double)) + 256;
  return p;
}
bool lap_shape_ok(int n, int per, int D) { return n >= 1 && n <= IW_MAX_ROWS && per >= 1 && n % per == 0 && D >= 1 && D <= IW_MAX_D; }

__global__ __launch_bounds__(256) void iw_add_term_kernel(const void* __restrict__ term, int is_f32, double sign, int n, int init, double* __restrict__ logw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = is_f32 ? (double)reinterpret_cast<const float*>(term)[i] : reinterpret_cast<const double*>(term)[i];
  logw[i] = init ? sign * v : logw[i] + sign * v;
}

// ---------------------------------------------------------------------------------------------------------------- streaming log-sum-exp
// state[b] = { M, sum exp(logw - M), sum exp(2 (logw - M)), sum logw, count }; a row with count 0 is empty whatever else it holds.
__global__ __launch_bounds__(256) void iw_accumulate_kernel(const double* __restrict__ logw, int B, int C, double* __restrict__ state) {
  const int lane = threadIdx.x & 63;
  const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;
  double* st = state + (size_t)b * 5;
  const bool empty = st[4] == 0.0;
  const double M0 = empty ? -INFINITY : st[0], s1o = empty ? 0.0 : st[1], s2o = empty ? 0.0 : st[2], slo = empty ? 0.0 : st[3], cnt = empty ? 0.0 : st[4];
  const double* row = logw + (size_t)b * C;
  double mx = -INFINITY, sl = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double v = row[c];
    mx = fmax(mx, v);
    sl += v;
  }
  mx = wave_max_d(mx);
  sl = wave_sum_d(sl);
  const double M1 = fmax(M0, mx);
  double s1 = 0.0, s2 = 0.0, a1 = 0.0, a2 = 0.0;
  if (M1 != -INFINITY) {                               // (all rows so far -inf: both sums stay 0, no inf - inf)
    for (int c = lane; c < C; c += 64) {
      const double e = exp(row[c] - M1);               // a -inf log-weight adds 0
      a1 += e;
      a2 += e * e;
    }
    const double f = M0 == -INFINITY ? 0.0 : exp(M0 - M1);
    s1 = s1o * f;
    s2 = s2o * f * f;
  }
  a1 = wave_sum_d(a1);
  a2 = wave_sum_d(a2);
  if (lane == 0) {
    st[0] = M1;
    st[1] = s1 + a1;
    st[2] = s2 + a2;
    st[3] = slo + sl;
    st[4] = cnt + (double)C;
  }
}

__global__ __launch_bounds__(256) void iw_finish_kernel(const double* __restrict__ state, int B, double* __restrict__ out) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  const double* st = state + (size_t)b * 5;
  double* o = out + (size_t)b * 4;
  const double cnt = st[4];
  if (cnt == 0.0) {                                    // no sample: nothing was estimated
    const double qn = __longlong_as_double(0x7ff8000000000000LL);
    o[0] = qn; o[1] = qn; o[2] = qn; o[3] = 0.0;
    return;
  }
  const bool dead = st[0] == -INFINITY;                // every weight 0
  o[0] = dead ? -INFINITY : st[0] + log(st[1]) - log(cnt);
  o[1] = st[3] / cnt;
  o[2] = dead ? 0.0 : st[1] * st[1] / st[2];
  o[3] = cnt;
}
}  // namespace

extern "C" {

int ladder_iw_randn_rows(float* out, int B, int C, int W, uint64_t image0, uint64_t sample0, uint64_t seed, int level, ladder_stream_t stream) {
  if (out == nullptr || B < 1 || C < 1 || W < 1 || W > IW_MAX_W || level < 0 || level > 15 || (long)B * C > IW_MAX_ROWS) return LADDER_E_SHAPE;
  const long n_rows = (long)B * C, total = n_rows * ((W + 3) / 4);
  hipLaunchKernelGGL(iw_randn_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, out, n_rows, C, W, (unsigned long long)image0,
                     (unsigned long long)sample0, seed, (uint32_t)level);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_iw_sample_rows(const float* mu, const float* sd, const float* eps, int n, int per, int W, float* sample, double* logq, ladder_stream_t stream) {
  if (mu == nullptr || sd == nullptr || eps == nullptr || sample == nullptr || logq == nullptr) return LADDER_E_SHAPE;
  if (n < 1 || n > IW_MAX_ROWS || per < 1 || n % per != 0 || W < 1 || W > IW_MAX_W) return LADDER_E_SHAPE;
  if (!iw_aligned8(logq)) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(iw_sample_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, mu, sd, eps, n, per, W, sample, logq);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_iw_gauss_rows(const float* a, const float* b, double s, int n, int W, double* out, ladder_stream_t stream) {
  if (a == nullptr || out == nullptr || n < 1 || n > IW_MAX_ROWS || W < 1 || W > IW_MAX_W || !(s > 0.0) || !(s < INFINITY)) return LADDER_E_SHAPE;
  if (!iw_aligned8(out)) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(iw_gauss_rows_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, a, b, s, n, W, out);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

size_t ladder_iw_laplace_rows_workspace_bytes(int n, int D) { return lap_shape_ok(n, 1, D) ? lap_plan(n, D).bytes : 0; }

int ladder_iw_laplace_rows(const float* x, const float* xhat, int n, int per, int D, double sigma, double* out, void* ws, size_t ws_bytes,
                           ladder_stream_t stream) {
  if (x == nullptr || xhat == nullptr || out == nullptr || !lap_shape_ok(n, per, D) || !(sigma > 0.0) || !(sigma < INFINITY)) return LADDER_E_SHAPE;
  if (!iw_aligned8(out)) return LADDER_E_ALIGN;
  const LapPlan p = lap_plan(n, D);
  double* part = nullptr;
  if (p.slices > 1) {
    if (ws == nullptr || ws_bytes < p.bytes) return LADDER_E_WORKSPACE;
    part = (double*)ladder_align256(ws);
  }
  const bool vec = D % 4 == 0 && ladder_aligned16(x) && ladder_aligned16(xhat);
  const dim3 grid((unsigned)n, (unsigned)p.slices);
  if (vec) hipLaunchKernelGGL(iw_laplace_rows_kernel<true>, grid, dim3(256), 0, stream, x, xhat, per, D, p.chunk, sigma, out, part);
  else hipLaunchKernelGGL(iw_laplace_rows_kernel<false>, grid, dim3(256), 0, stream, x, xhat, per, D, p.chunk, sigma, out, part);
  if (p.slices > 1)
    hipLaunchKernelGGL(iw_laplace_finish_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, (const double*)part, n, p.slices, D, sigma, out);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_iw_add_term(const void* term, int term_is_f32, double sign, int n, int init, double* logw, ladder_stream_t stream) {
  if (term == nullptr || logw == nullptr || n < 1 || n > IW_MAX_ROWS) return LADDER_E_SHAPE;
  if (!iw_aligned8(logw) || (!term_is_f32 && !iw_aligned8(term))) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(iw_add_term_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, term, term_is_f32, sign, n, init, logw);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_iw_accumulate(const double* logw, int B, int C, double* state, ladder_stream_t stream) {
  if (logw == nullptr || state == nullptr || B < 1 || C < 1 || (long)B * C > IW_MAX_ROWS) return LADDER_E_SHAPE;
  if (!iw_aligned8(logw) || !iw_aligned8(state)) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(iw_accumulate_kernel, dim3((B + 3) / 4), dim3(256), 0, stream, logw, B, C, state);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_iw_finish(const double* state, int B, double* out, ladder_stream_t stream) {
  if (state == nullptr || out == nullptr || B < 1 || B > IW_MAX_ROWS) return LADDER_E_SHAPE;
  if (!iw_aligned8(state) || !iw_aligned8(out)) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(iw_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, state, B, out);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}
}  // extern "C"
