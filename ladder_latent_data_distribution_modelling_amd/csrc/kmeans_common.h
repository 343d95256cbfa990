// What csrc/kmeans.hip (1 <= R <= 64) and csrc/kmeans_wide.hip (64 < R <= 256) use unchanged: the workspace, the preparation and seeding kernels
// (a workgroup per column, a thread or 16 lanes per sample: any width up to the 256-thread block), the cluster sums over 64-column groups and the checks of the
// exported calls.  What differs by width -- the assignment and the update -- is in the two files; the header comment of csrc/kmeans.hip describes the
// algorithm and the protocol.
#pragma once
#include "fit_util.h"

#include <limits.h>

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int KM_MAXK = 64;
constexpr int KM_PANEL = 64;            // columns an assignment stages at a time, and of one group of the cluster sums: 16 MFMA k-steps / 4 column blocks
constexpr int KM_SLICE = 64;            // samples per assignment workgroup: 4 wavefronts x 16 MFMA rows
// LDS row pitch of the staged centres in doubles.  The B operand of lane (n, kq) is s_C[(16 kb + n) * pitch + 4 s + kq]; ds_read_b64 serves lanes 0-31
// and 32-63 in turn over 32 eight-byte banks, so within a half (n = 0..15, two values of kq) the index n * pitch + kq must be distinct modulo 32:
// pitch = 2 (mod 32) gives 2 n + kq, all 32 banks once.
constexpr int KM_LDC = 66;
constexpr int KM_BLOCK = 256;           // samples per block of the seeding's scan
constexpr int KM_MAXTRIALS = 6;         // 2 + int(ln 64)
// integer part of the workspace
constexpr int KI_CNT = 0, KI_CHANGED = 64, KI_PENDING = 65, KI_SEL = 66, KI_CAND = 68, KI_CHOSEN = 80, KI_TOTAL = 144;

inline int km_trials(int K) { return 2 + (int)log((double)K); }
inline int km_blocks(int N) { return (N + KM_BLOCK - 1) / KM_BLOCK; }
inline int km_slices(int N) { return (N + KM_SLICE - 1) / KM_SLICE; }

// workspace: colsum [R] | sum x~ [R] | sum x~^2 [R] | potential, 3 spare | shifted centres [K,R] | per-split cluster sums [nsplit,K,R] | squared distance
// to the own centre [N] | candidates' closest distances [6,N] | their block sums [6,nb] | offsets [nb+1] | (wide alone: cluster sums [K,R]) |
// integers [KI_TOTAL]
struct KmWs {
  double *colsum, *s1, *s2, *scal, *cs, *part, *dist, *cc, *cblk, *offs, *sum;
  int* ints;
};
inline size_t km_ws_doubles(int N, int K, int R, bool wide) {
  const size_t nb = km_blocks(N);
  return 3 * (size_t)R + 4 + (size_t)K * R * (1 + fit_split(N).nsplit + (wide ? 1 : 0)) + (size_t)N * (1 + KM_MAXTRIALS) + KM_MAXTRIALS * nb + nb + 1;
}
inline size_t km_ws_bytes(int N, int K, int R, bool wide) { return km_ws_doubles(N, K, R, wide) * sizeof(double) + KI_TOTAL * sizeof(int); }
inline KmWs km_ws(void* ws, int N, int K, int R, bool wide) {
  const size_t nb = km_blocks(N);
  KmWs W;
  W.colsum = static_cast<double*>(ws);
  W.s1 = W.colsum + R;
  W.s2 = W.s1 + R;
  W.scal = W.s2 + R;
  W.cs = W.scal + 4;
  W.part = W.cs + (size_t)K * R;
  W.dist = W.part + (size_t)K * R * fit_split(N).nsplit;
  W.cc = W.dist + N;
  W.cblk = W.cc + (size_t)KM_MAXTRIALS * N;
  W.offs = W.cblk + KM_MAXTRIALS * nb;
  W.sum = W.offs + nb + 1;
  W.ints = reinterpret_cast<int*>(W.sum + (wide ? (size_t)K * R : 0));
  return W;
}

__device__ __forceinline__ double km_shift(const KmWs& W, int N, int j) { return (double)(float)(W.colsum[j] / (double)N); }

// Inclusive scan over the 256 threads of a workgroup in ONE fixed order: shuffle scan inside a wavefront, then the wavefronts' totals in order.
// EVERY thread must call it (two barriers); s_w: 4 doubles of LDS.
__device__ __forceinline__ double km_block_scan(double v, double* s_w, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const double t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) s_w[wave] = v;
  __syncthreads();
  double off = 0.0;
  for (int w = 0; w < wave; ++w) off += s_w[w];
  __syncthreads();
  return off + v;
}

// ------------------------------------------------------------------------------------------------ preparation
__global__ __launch_bounds__(256) void kmeans_colsum_kernel(const float* __restrict__ X, int N, int R, KmWs W) {
  const int j = blockIdx.x, tid = threadIdx.x;
  __shared__ double s_w[4];
  const double a = column_sum_256(X, N, R, j, s_w, tid);
  if (tid == 0) W.colsum[j] = a;
}

__global__ __launch_bounds__(256) void kmeans_moments_kernel(const float* __restrict__ X, int N, int K, int R, double* __restrict__ state, KmWs W) {
  const int j = blockIdx.x, tid = threadIdx.x;
  __shared__ double s_w[4];
  const double c = km_shift(W, N, j);
  double a1 = 0.0, a2 = 0.0;
  for (int n = tid; n < N; n += 256) {
    const double d = (double)X[(size_t)n * R + j] - c;
    a1 += d;
    a2 += d * d;
  }
  a1 = block_sum_256(a1, s_w, tid);
  a2 = block_sum_256(a2, s_w, tid);
  if (tid == 0) {
    W.s1[j] = a1;
    W.s2[j] = a2;
  }
  if (j == 0) {                                                     // a fit starts here: counters and the state tail
    for (int i = tid; i < KI_TOTAL; i += 256) W.ints[i] = 0;
    if (tid < 4) {
      W.scal[tid] = 0.0;
      state[(size_t)K * R + tid] = 0.0;
    }
  }
}

// explicit initial centres (sklearn's init = array)
__global__ __launch_bounds__(256) void kmeans_setc_kernel(const double* __restrict__ centres, int N, int K, int R, double* __restrict__ state, KmWs W) {
  for (int e = threadIdx.x; e < K * R; e += 256) {
    const double v = centres[e];
    W.cs[e] = v - km_shift(W, N, e % R);
    state[e] = v;
  }
}

// ------------------------------------------------------------------------------------------------ seeding
__global__ __launch_bounds__(256) void kmeans_pick_kernel(const float* __restrict__ X, int N, int K, int R, int ntr, int c, const double* __restrict__ draws,
                                                          double* __restrict__ state, KmWs W) {
  const int tid = threadIdx.x, nb = (N + KM_BLOCK - 1) / KM_BLOCK;
  __shared__ double s_pot[KM_MAXTRIALS], s_w[4];
  __shared__ int s_i[2];
  if (c == 0) {                                                     // the first centre is its own only candidate
    if (tid == 0) {
      const double f = draws[0];
      W.ints[KI_CAND] = f >= 0.0 ? (f < (double)N ? (int)f : N - 1) : 0;
    }
    return;
  }
  // ---- close step c - 1
  const int np = (c == 1) ? 1 : ntr;
  if (tid < np) {
    const double* bs = W.cblk + (size_t)tid * nb;
    double a = 0.0;
    for (int b = 0; b < nb; ++b) a += bs[b];
    s_pot[tid] = a;
  }
  __syncthreads();
  int best = 0;
  for (int t = 1; t < np; ++t)
    if (s_pot[t] < s_pot[best]) best = t;                           // numpy.argmin: the lowest index among equals
  const double pot = s_pot[best];
  const int idx = W.ints[KI_CAND + best];
  __syncthreads();                                                  // (every thread has read the candidate before the list is rewritten)
  if (tid == 0) {
    W.ints[KI_SEL] = best;
    W.ints[KI_CHOSEN + c - 1] = idx;
    W.scal[0] = pot;
  }
  if (tid < R) {                                                    // (R <= 256 = the block: one thread per coordinate)
    const double xv = (double)X[(size_t)idx * R + tid];
    W.cs[(size_t)(c - 1) * R + tid] = xv - km_shift(W, N, tid);
    state[(size_t)(c - 1) * R + tid] = xv;
  }
  if (c == K) return;
  // ---- open step c: the cumulative sum of the closest distances = offsets of the blocks + the scan inside a block
  const double* closest = W.cc + (size_t)best * N;
  const double* bs = W.cblk + (size_t)best * nb;
  if (tid == 0) {
    double a = 0.0;
    W.offs[0] = 0.0;
    for (int b = 0; b < nb; ++b) {
      a += bs[b];
      W.offs[b + 1] = a;                                            // (offs[nb] has the bits of `pot`: the same sum)
    }
  }
  __syncthreads();
  const double* offs = W.offs;
  for (int t = 0; t < ntr; ++t) {
    const double target = draws[1 + (size_t)(c - 1) * ntr + t] * pot;
    if (tid == 0) {
      s_i[0] = nb;
      s_i[1] = INT_MAX;
    }
    __syncthreads();
    for (int b = tid; b < nb; b += 256)
      if (offs[b + 1] >= target) {
        atomicMin(&s_i[0], b);
        break;
      }
    __syncthreads();
    const int b0 = s_i[0];                                          // (uniform)
    int res = N - 1;                                                // past the last cumulative sum: numpy's N, clipped
    if (b0 < nb) {
      const int n = b0 * KM_BLOCK + tid;
      const double s = km_block_scan(n < N ? closest[n] : 0.0, s_w, tid);
      if (n < N && offs[b0] + s >= target) atomicMin(&s_i[1], n);
      __syncthreads();
      res = s_i[1] != INT_MAX ? s_i[1] : min(N - 1, b0 * KM_BLOCK + KM_BLOCK - 1);
    }
    __syncthreads();
    if (tid == 0) W.ints[KI_CAND + t] = res;
  }
}

// MAXR: the widest sample of the file that instantiates it = the pitch of the staged candidates (6 x 64 doubles = 3 KB, 6 x 256 = 12 KB).
// LPS: lanes per sample.  1 (R <= 64): a thread walks its own row, columns ascending.  16 (wide, R % 16 == 0): a 1 KB row walked by one thread is 256
// loads one after the other in a grid of N / 256 workgroups -- latency, whatever N (measured: 88 us a launch at 2 048 and at 20 032 samples) -- so 16
// lanes share a row (columns m, m + 16, ..., then the shuffle tree over the 16 lanes: one fixed order).  The 16 lane groups of the block take 16
// consecutive samples per round and four rounds at a time: their 64 loads per lane are issued together, and a candidate's coordinate read from LDS
// serves the four samples.  The distances pass through LDS to the thread-per-sample layout of the scan.
template <int MAXR, int LPS>
__global__ __launch_bounds__(256) void kmeans_cand_kernel(const float* __restrict__ X, int N, int R, int ntr, int c, KmWs W) {
  const int tid = threadIdx.x, b = blockIdx.x, nb = gridDim.x, n = b * KM_BLOCK + tid;
  const int nt = (c == 0) ? 1 : ntr;
  __shared__ double s_c[KM_MAXTRIALS * MAXR], s_w[4];
  for (int i = tid; i < nt * R; i += 256) {
    const int t = i / R, j = i - t * R;
    s_c[t * MAXR + j] = (double)X[(size_t)W.ints[KI_CAND + t] * R + j];
  }
  __syncthreads();
  double acc[KM_MAXTRIALS];
#pragma unroll
  for (int t = 0; t < KM_MAXTRIALS; ++t) acc[t] = 0.0;
  double old = INFINITY;
  if constexpr (LPS > 1) {
    constexpr int NG = KM_BLOCK / LPS, NJ = MAXR / LPS, RQ = 4;     // samples per round; columns per lane; rounds in flight
    static_assert(LPS % RQ == 0 && MAXR % LPS == 0, "whole groups of rounds, whole columns per lane");
    __shared__ double s_v[KM_MAXTRIALS * KM_BLOCK];
    const int g = tid / LPS, m = tid % LPS, nj = R / LPS;
    for (int r0 = 0; r0 < LPS; r0 += RQ) {                          // (uniform: every lane reaches every shuffle)
      float xv[RQ][NJ];
#pragma unroll
      for (int q = 0; q < RQ; ++q) {                                // (no branch around a load: a sample past N reads row N - 1 and a column
        const float* xr = X + (size_t)min(b * KM_BLOCK + (r0 + q) * NG + g, N - 1) * R + m;      // block past R the last one; neither is used)
#pragma unroll
        for (int i = 0; i < NJ; ++i) xv[q][i] = xr[min(i, nj - 1) * LPS];
      }
      double a[RQ][KM_MAXTRIALS];
#pragma unroll
      for (int q = 0; q < RQ; ++q)
#pragma unroll
        for (int t = 0; t < KM_MAXTRIALS; ++t) a[q][t] = 0.0;
#pragma unroll
      for (int i = 0; i < NJ; ++i)
        if (i < nj) {
#pragma unroll
          for (int t = 0; t < KM_MAXTRIALS; ++t)
            if (t < nt) {
              const double cv = s_c[t * MAXR + m + i * LPS];
#pragma unroll
              for (int q = 0; q < RQ; ++q) {
                const double d = (double)xv[q][i] - cv;
                a[q][t] += d * d;
              }
            }
        }
#pragma unroll
      for (int q = 0; q < RQ; ++q)
#pragma unroll
        for (int t = 0; t < KM_MAXTRIALS; ++t)
          if (t < nt) {
#pragma unroll
            for (int o = 1; o < LPS; o <<= 1) a[q][t] += __shfl_xor(a[q][t], o, 64);
            if (m == 0) s_v[t * KM_BLOCK + (r0 + q) * NG + g] = a[q][t];
          }
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < KM_MAXTRIALS; ++t)
      if (t < nt) acc[t] = s_v[t * KM_BLOCK + tid];
  } else if (n < N) {
    const float* xr = X + (size_t)n * R;
    for (int j = 0; j < R; ++j) {
      const double xv = (double)xr[j];
#pragma unroll
      for (int t = 0; t < KM_MAXTRIALS; ++t)
        if (t < nt) {
          const double d = xv - s_c[t * MAXR + j];
          acc[t] += d * d;
        }
    }
  }
  if (n < N) {
    if (c != 0) old = W.cc[(size_t)W.ints[KI_SEL] * N + n];         // (read before this thread overwrites plane KI_SEL below)
  }
#pragma unroll
  for (int t = 0; t < KM_MAXTRIALS; ++t)
    if (t < nt) {                                                   // (uniform: every thread reaches the scan's barriers)
      const double v = n < N ? fmin(old, acc[t]) : 0.0;
      if (n < N) W.cc[(size_t)t * N + n] = v;
      const double s = km_block_scan(v, s_w, tid);
      if (tid == KM_BLOCK - 1) W.cblk[(size_t)t * nb + b] = s;
    }
}

// ------------------------------------------------------------------------------------------------ cluster sums
// blockIdx.x = row split, blockIdx.y = group of 64 columns.  Wavefront w owns the clusters 16 w .. 16 w + 15: A = the one-hot labels, B = x~, the
// group's four column blocks as MFMA accumulators.
__global__ __launch_bounds__(256) void kmeans_sums_kernel(const float* __restrict__ X, const int* __restrict__ labels, const double* __restrict__ state, int N,
                                                          int K, int R, int rows, KmWs W) {
  if (state[(size_t)K * R + FIT_DONE] != 0.0 || W.ints[KI_PENDING] != 0) return;       // over, or only the final assignment is left
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
  const int j0 = blockIdx.y * KM_PANEL, nkb = (K + 15) / 16, nb = (min(R - j0, KM_PANEL) + 15) / 16;
  if (wave >= nkb) return;                                         // (whole wavefronts; no barrier in this kernel)
  const int ka = wave * 16 + m;
  int jb[4];
  bool vb[4];
  double cb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    jb[q] = j0 + 16 * q + m;
    vb[q] = jb[q] < R;
    cb[q] = vb[q] ? km_shift(W, N, jb[q]) : 0.0;
  }
  const int r0 = blockIdx.x * rows, r1 = min(N, r0 + rows);
  double4_t acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  // Four k-steps a trip, so that their 20 loads are in flight together (one k-step a trip waits for memory 160 times over a 626-row split) -- no branch
  // around a load: a row past the split reads the split's last row, a column past R column R - 1, and neither is used.  The MFMAs are those of one
  // k-step a trip, in the same order.
  for (int r = r0; r < r1; r += 16) {                              // (uniform trip count)
    float xv[4][4];
    int lb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int rc = min(r + 4 * u + kq, r1 - 1);
      const float* xr = X + (size_t)rc * R;
      lb[u] = labels[rc];
#pragma unroll
      for (int q = 0; q < 4; ++q) xv[u][q] = xr[min(jb[q], R - 1)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (r + 4 * u < r1) {                                        // (uniform)
        const bool ok = r + 4 * u + kq < r1;
        const double a = (ok && lb[u] == ka) ? 1.0 : 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (q < nb) {
            const double b = (ok && vb[q]) ? (double)xv[u][q] - cb[q] : 0.0;
            acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
          }
        }
      }
    }
  }
  double* out = W.part + (size_t)blockIdx.x * K * R;
#pragma unroll
  for (int rg = 0; rg < 4; ++rg) {
    const int k = wave * 16 + kq + 4 * rg;
    if (k >= K) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (q < nb && vb[q]) out[(size_t)k * R + jb[q]] = acc[q][rg];
  }
}

// ------------------------------------------------------------------------------------------------ host side
// The checks every exported call makes before it launches anything, in the order of the C ABI: shapes and NULL arrays, then the alignment of the
// double arrays, then the workspace.  bad: the file's own shape test (and it / max_iter); a, b: the double arrays besides ws (b may repeat a).
inline int km_check(bool bad, const void* X, const void* a, const void* b, const void* ws, size_t ws_bytes, size_t need) {
  if (X == nullptr || a == nullptr || b == nullptr || bad) return LADDER_E_SHAPE;
  if (fit_misaligned(a) || fit_misaligned(b) || fit_misaligned(ws)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < need) return LADDER_E_SHAPE;                          // (a workspace too short for the shape)
  return LADDER_OK;
}

inline int km_prepare(const float* X, int N, int K, int R, double* state, const KmWs& W, hipStream_t stream) {
  hipLaunchKernelGGL(kmeans_colsum_kernel, dim3(R), dim3(256), 0, stream, X, N, R, W);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(kmeans_moments_kernel, dim3(R), dim3(256), 0, stream, X, N, K, R, state, W);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

template <int MAXR, int LPS>
inline int km_seed(const float* X, int N, int K, int R, const double* draws, double* state, const KmWs& W, hipStream_t s) {
  const int rc = km_prepare(X, N, K, R, state, W, s);
  if (rc != LADDER_OK) return rc;
  const int ntr = km_trials(K), nb = km_blocks(N);
  for (int c = 0; c <= K; ++c) {
    hipLaunchKernelGGL(kmeans_pick_kernel, dim3(1), dim3(256), 0, s, X, N, K, R, ntr, c, draws, state, W);
    LADDER_CHECK_LAUNCH();
    if (c == K) break;
    hipLaunchKernelGGL((kmeans_cand_kernel<MAXR, LPS>), dim3(nb), dim3(256), 0, s, X, N, R, ntr, c, W);
    LADDER_CHECK_LAUNCH();
  }
  return LADDER_OK;
}

inline int km_set_centres(const float* X, int N, int K, int R, const double* centres, double* state, const KmWs& W, hipStream_t s) {
  const int rc = km_prepare(X, N, K, R, state, W, s);
  if (rc != LADDER_OK) return rc;
  hipLaunchKernelGGL(kmeans_setc_kernel, dim3(1), dim3(256), 0, s, centres, N, K, R, state, W);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // namespace
