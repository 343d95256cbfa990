// K-means on the device: the labels a cold mixture fit starts from (reference codes/base.py:93-106, through BaseMixture._initialize_parameters):
// sklearn.cluster.KMeans(init="k-means++" or an array, n_init=1, algorithm="lloyd") restated in float64 on fp32 samples [N, R] for 1 <= R <= 64,
// 1 <= K <= 64, N >= K -- the functions _kmeans_plusplus, lloyd_iter_chunked_dense, _relocate_empty_clusters_dense, _average_centers and the loop of
// _kmeans_single_lloyd.  The conventions are those of csrc/emgmm.hip: the samples are shifted by ONE vector c (the fp32-rounded global mean, so
// x~ = x - c is exact in float64; distances and the tolerance are translation invariant), no floating-point atomics (every sum has one fixed order:
// the same bits on every run), kernel boundaries are the only grid-wide synchronisation, and a device-side `done` flag turns every kernel of the
// iteration into a no-op, so the host may enqueue iterations ahead and read the flag every few iterations.
//
// Preparation (both entries)
//   kmeans_colsum_kernel   column sums -> the shift c
//   kmeans_moments_kernel  sum x~, sum x~^2 per column (tol_ = tol * mean_j var_j from them); clears the counters and the state tail
// Seeding, ladder_kmeans_seed: the host supplies draws = [ index of the first centre | uniforms [K-1, n_trials] ], n_trials = 2 + int(ln K); step c picks
// centre c, all steps are enqueued back to back
//   kmeans_pick_kernel     ONE workgroup.  Closes step c-1: the candidates' potentials = their block sums added in block order, argmin with the lowest
//                          index winning -> centre c-1, the current closest distances and their potential.  Opens step c: offsets = the running sum of
//                          the 256-sample block sums; per uniform u the first n with offset[block] + scan_in_block[n] >= u * potential
//                          (numpy.searchsorted, left side), clipped to N - 1
//   kmeans_cand_kernel     one thread per sample: squared distances to the n_trials candidates by direct differences (exact in float64), the minimum
//                          with the current closest distance, per candidate the block sum (the last value of the same in-block scan the search uses)
// Lloyd iteration it = 1, 2, ...: ladder_kmeans_assign, then ladder_kmeans_update
//   kmeans_assign_kernel   a workgroup owns 64 samples: the shifted centres (zero-padded to multiples of 16 x 4) and their squared norms are staged in
//                          LDS, |c_k|^2 - 2 x~.c_k comes from v_mfma_f64_16x16x4_f64, row argmin with the lowest index winning (numpy.argmin); the
//                          label, the squared distance to the own centre by direct differences, integer counters: samples per cluster, changed labels
//   kmeans_sums_kernel     onehot(labels)^T x~ over row splits on the same MFMA (fit_stats_kernel at it == 0); partials per split
//   kmeans_update_kernel   ONE workgroup: partials added in split order, empty-cluster relocation, new centres, sum |c_new - c_old|^2, the convergence
//                          test of _kmeans_single_lloyd: labels unchanged -> strict convergence, the labels stand; else shift <= tol_ or it == max_iter
//                          -> ONE more assignment against the final centres (the next assign / update pair, which only sums inertia_ and sets `done`).
//                          The host therefore enqueues up to max_iter + 1 pairs.
// Relocation: empty clusters in ascending index receive the samples farthest from their own centres, in descending distance with the lowest index
// winning; each donor is subtracted from its old cluster's sum and count.  For ONE empty cluster that is sklearn's result; for several, sklearn's order
// comes from numpy.argpartition and is unspecified.
//
// state (doubles): centres [K,R] (unshifted) | inertia_, n_iter_, status (1 = shift <= tol_, 2 = labels unchanged, 3 = max_iter), done
//
// Operand lane maps of v_mfma_f64_16x16x4_f64: head of csrc/fid.hip (A [m = lane & 15][k = lane >> 4], B [k][n = lane & 15],
// C/D reg r: row (lane >> 4) + 4 r, col lane & 15).
#include "fit_util.h"

#include <limits.h>

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int KM_MAXR = 64, KM_MAXK = 64;
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
// to the own centre [N] | candidates' closest distances [6,N] | their block sums [6,nb] | offsets [nb+1] | integers [KI_TOTAL]
struct KmWs {
  double *colsum, *s1, *s2, *scal, *cs, *part, *dist, *cc, *cblk, *offs;
  int* ints;
};
inline size_t km_ws_doubles(int N, int K, int R) {
  const size_t nb = km_blocks(N);
  return 3 * (size_t)R + 4 + (size_t)K * R * (1 + fit_split(N).nsplit) + (size_t)N * (1 + KM_MAXTRIALS) + KM_MAXTRIALS * nb + nb + 1;
}
inline KmWs km_ws(void* ws, int N, int K, int R) {
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
  W.ints = reinterpret_cast<int*>(W.offs + nb + 1);
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
  if (tid < R) {
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

__global__ __launch_bounds__(256) void kmeans_cand_kernel(const float* __restrict__ X, int N, int R, int ntr, int c, KmWs W) {
  const int tid = threadIdx.x, b = blockIdx.x, nb = gridDim.x, n = b * KM_BLOCK + tid;
  const int nt = (c == 0) ? 1 : ntr;
  __shared__ double s_c[KM_MAXTRIALS * KM_MAXR], s_w[4];
  for (int i = tid; i < nt * R; i += 256) {
    const int t = i / R, j = i - t * R;
    s_c[t * KM_MAXR + j] = (double)X[(size_t)W.ints[KI_CAND + t] * R + j];
  }
  __syncthreads();
  double acc[KM_MAXTRIALS];
#pragma unroll
  for (int t = 0; t < KM_MAXTRIALS; ++t) acc[t] = 0.0;
  double old = INFINITY;
  if (n < N) {
    const float* xr = X + (size_t)n * R;
    for (int j = 0; j < R; ++j) {
      const double xv = (double)xr[j];
#pragma unroll
      for (int t = 0; t < KM_MAXTRIALS; ++t)
        if (t < nt) {
          const double d = xv - s_c[t * KM_MAXR + j];
          acc[t] += d * d;
        }
    }
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

// ------------------------------------------------------------------------------------------------ assignment
__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ X, int N, int K, int R, int it, const double* __restrict__ state,
                                                            int* __restrict__ labels, KmWs W) {
  if (state[(size_t)K * R + FIT_DONE] != 0.0) return;              // the fit is over: iterations enqueued past the end are no-ops
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * KM_SLICE, rows = min(KM_SLICE, N - n0);
  __shared__ double s_C[KM_MAXK * KM_LDC], s_cn[KM_MAXK], s_sh[KM_MAXR];
  __shared__ int s_cnt[KM_MAXK], s_chg;
  const int nkb = (K + 15) / 16, Kp = nkb * 16, nsteps = (R + 3) / 4, Rp = nsteps * 4;
  for (int idx = tid; idx < Kp * Rp; idx += 256) {
    const int i = idx / Rp, j = idx - i * Rp;
    s_C[i * KM_LDC + j] = (i < K && j < R) ? W.cs[(size_t)i * R + j] : 0.0;
  }
  if (tid < KM_MAXK) {
    double a = INFINITY;                                            // a padded centre never wins
    if (tid < K) {
      a = 0.0;
      for (int j = 0; j < R; ++j) {
        const double v = W.cs[(size_t)tid * R + j];
        a += v * v;
      }
    }
    s_cn[tid] = a;
    s_cnt[tid] = 0;
    s_sh[tid] = tid < R ? km_shift(W, N, tid) : 0.0;
  }
  if (tid == 0) s_chg = 0;
  __syncthreads();
  const int row = wave * 16 + m;
  const bool rv = row < rows;
  const float* xr = X + (size_t)(n0 + (rv ? row : 0)) * R;         // (row n0 exists: never dereferenced unless rv)
  double xa[16];                                                   // this lane's A operands: x~[row][4 s + kq], zero past R
#pragma unroll
  for (int s = 0; s < 16; ++s) {
    const int i = 4 * s + kq;
    xa[s] = (rv && i < R) ? (double)xr[i] - s_sh[i] : 0.0;
  }
  double bv[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  int bi[4] = {0, 0, 0, 0};
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    if (kb < nkb) {                                                // (uniform: every lane reaches every MFMA)
      double4_t acc = double4_t{0.0, 0.0, 0.0, 0.0};
      const double* cr = s_C + (16 * kb + m) * KM_LDC + kq;
#pragma unroll
      for (int s = 0; s < 16; ++s)
        if (s < nsteps) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[s], cr[4 * s], acc, 0, 0, 0);
      const double cn = s_cn[16 * kb + m];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double sc = cn - 2.0 * acc[r];
        if (sc < bv[r]) {                                          // ascending kb: the lowest index among equals stays
          bv[r] = sc;
          bi[r] = 16 * kb + m;
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {                             // over the 16 centres of the lane group: the same pair in every lane
      const double ov = __shfl_xor(bv[r], o, 64);
      const int oi = __shfl_xor(bi[r], o, 64);
      if (ov < bv[r] || (ov == bv[r] && oi < bi[r])) {
        bv[r] = ov;
        bi[r] = oi;
      }
    }
    const int rr = wave * 16 + kq + 4 * r;
    const bool ok = rr < rows;
    const int k = bi[r];
    double p = 0.0;                                                // |x~ - c_k|^2 by direct differences: columns m, m + 16, ..., then the 16 lanes
    if (ok) {
      const float* xq = X + (size_t)(n0 + rr) * R;
      for (int j = m; j < R; j += 16) {
        const double d = ((double)xq[j] - s_sh[j]) - s_C[k * KM_LDC + j];
        p += d * d;
      }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) p += __shfl_xor(p, o, 64);
    if (ok && m == 0) {
      const int n = n0 + rr;
      const int old = it <= 1 ? -1 : labels[n];
      labels[n] = k;
      W.dist[n] = p;
      if (old != k) atomicAdd(&s_chg, 1);
      atomicAdd(&s_cnt[k], 1);
    }
  }
  __syncthreads();
  if (tid < K && s_cnt[tid] != 0) atomicAdd(&W.ints[KI_CNT + tid], s_cnt[tid]);
  if (tid == 0 && s_chg != 0) atomicAdd(&W.ints[KI_CHANGED], s_chg);
}

// ------------------------------------------------------------------------------------------------ cluster sums
// blockIdx.x = row split.  Wavefront w owns the clusters 16 w .. 16 w + 15: A = the one-hot labels, B = x~, four column blocks as MFMA accumulators.
__global__ __launch_bounds__(256) void kmeans_sums_kernel(const float* __restrict__ X, const int* __restrict__ labels, const double* __restrict__ state, int N,
                                                          int K, int R, int rows, KmWs W) {
  if (state[(size_t)K * R + FIT_DONE] != 0.0 || W.ints[KI_PENDING] != 0) return;       // over, or only the final assignment is left
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
  const int nkb = (K + 15) / 16, nb = (R + 15) / 16;
  if (wave >= nkb) return;                                         // (whole wavefronts; no barrier in this kernel)
  const int ka = wave * 16 + m;
  int jb[4];
  bool vb[4];
  double cb[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    jb[q] = 16 * q + m;
    vb[q] = jb[q] < R;
    cb[q] = vb[q] ? km_shift(W, N, jb[q]) : 0.0;
  }
  const int r0 = blockIdx.x * rows, r1 = min(N, r0 + rows);
  double4_t acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int r = r0; r < r1; r += 4) {                               // (uniform trip count)
    const int row = r + kq;
    const bool ok = row < r1;
    const float* xr = X + (size_t)(ok ? row : r0) * R;
    const double a = (ok && labels[row] == ka) ? 1.0 : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q < nb) {
        const double b = (ok && vb[q]) ? (double)xr[jb[q]] - cb[q] : 0.0;
        acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[q], 0, 0, 0);
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

// ------------------------------------------------------------------------------------------------ update
__global__ __launch_bounds__(256) void kmeans_update_kernel(const float* __restrict__ X, const int* __restrict__ labels, int N, int K, int R, int nsplit,
                                                            double tol, int max_iter, int it, double* __restrict__ state, KmWs W) {
  double* tail = state + (size_t)K * R;
  if (tail[FIT_DONE] != 0.0) return;
  const int tid = threadIdx.x;
  __shared__ double s_sum[KM_MAXK * KM_MAXR], s_sh[KM_MAXR], s_sq[KM_MAXK], s_rd[256], s_w[4];
  __shared__ int s_cnt[KM_MAXK], s_el[KM_MAXK], s_taken[KM_MAXK], s_rn[256], s_ne, s_far, s_old, s_fin;
  bool finish = W.ints[KI_PENDING] != 0;                            // the final assignment has run: only inertia_ is left
  if (!finish) {
    const int changed = W.ints[KI_CHANGED];
    if (tid < KM_MAXK) {
      s_cnt[tid] = tid < K ? W.ints[KI_CNT + tid] : 0;
      s_sh[tid] = tid < R ? km_shift(W, N, tid) : 0.0;
    }
    if (tid == 0) s_fin = 0;
    for (int e = tid; e < K * R; e += 256) {
      double a = 0.0;
      for (int s = 0; s < nsplit; ++s) a += W.part[(size_t)s * K * R + e];
      s_sum[e] = a;
    }
    __syncthreads();
    if (tid == 0) {
      int ne = 0;
      for (int k = 0; k < K; ++k)
        if (s_cnt[k] == 0) s_el[ne++] = k;
      s_ne = ne;
    }
    __syncthreads();
    const int ne = s_ne;
    for (int e = 0; e < ne; ++e) {                                  // relocation: the e-th farthest sample goes to the e-th empty cluster
      double bd = -1.0;
      int bn = INT_MAX;
      for (int n = tid; n < N; n += 256) {
        bool taken = false;
        for (int q = 0; q < e; ++q) taken = taken || (s_taken[q] == n);
        const double d = W.dist[n];
        if (!taken && d > bd) {                                     // ascending n: the lowest index among equals stays
          bd = d;
          bn = n;
        }
      }
      s_rd[tid] = bd;
      s_rn[tid] = bn;
      __syncthreads();
      for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
          const double od = s_rd[tid + o];
          const int on = s_rn[tid + o];
          if (od > s_rd[tid] || (od == s_rd[tid] && on < s_rn[tid])) {
            s_rd[tid] = od;
            s_rn[tid] = on;
          }
        }
        __syncthreads();
      }
      if (tid == 0) {
        const int far = s_rn[0], nw = s_el[e];
        const int old = far < N ? labels[far] : -1;                 // (no donor: every distance is NaN, or labels no assignment wrote)
        const bool ok = old >= 0 && old < K;
        s_taken[e] = far;
        s_far = ok ? far : -1;
        s_old = old;
        if (ok) {
          s_cnt[nw] = 1;
          s_cnt[old] -= 1;
        }
      }
      __syncthreads();
      if (tid < R && s_far >= 0) {
        const double xt = (double)X[(size_t)s_far * R + tid] - s_sh[tid];
        s_sum[s_old * R + tid] -= xt;
        s_sum[s_el[e] * R + tid] = xt;
      }
      __syncthreads();
    }
    for (int e = tid; e < K * R; e += 256) {                        // _average_centers: centre *= 1 / weight where the weight is positive
      const int cnt = s_cnt[e / R];
      if (cnt > 0) s_sum[e] *= 1.0 / (double)cnt;
    }
    __syncthreads();
    if (tid < K) {
      double a = 0.0;
      for (int j = 0; j < R; ++j) {
        const double d = s_sum[tid * R + j] - W.cs[(size_t)tid * R + j];
        a += d * d;
      }
      s_sq[tid] = a;
    }
    __syncthreads();
    for (int e = tid; e < K * R; e += 256) {
      W.cs[e] = s_sum[e];
      state[e] = s_sum[e] + s_sh[e % R];
    }
    if (tid == 0) {
      double shift = 0.0, mv = 0.0;
      for (int k = 0; k < K; ++k) shift += s_sq[k];
      for (int j = 0; j < R; ++j) {                                 // tol_ = tol * mean(var(X, axis=0)), from the shifted moments
        const double mu = W.s1[j] / (double)N;
        mv += W.s2[j] / (double)N - mu * mu;
      }
      const double tol_ = tol * (mv / (double)R);
      W.scal[1] = shift;
      W.scal[2] = tol_;
      if (changed == 0) {                                           // strict convergence: the labels stand
        tail[FIT_NITER] = (double)it;
        tail[2] = 2.0;
        s_fin = 1;
      } else if (shift <= tol_ || it >= max_iter) {                 // one more assignment against the final centres
        tail[FIT_NITER] = (double)it;
        tail[2] = shift <= tol_ ? 1.0 : 3.0;
        W.ints[KI_PENDING] = 1;
      }
      W.ints[KI_CHANGED] = 0;
    }
    if (tid < K) W.ints[KI_CNT + tid] = 0;
    __syncthreads();
    finish = s_fin != 0;
  }
  if (finish) {                                                     // (uniform) inertia_ = sum of the squared distances to the own centres
    double a = 0.0;
    for (int n = tid; n < N; n += 256) a += W.dist[n];
    a = block_sum_256(a, s_w, tid);
    if (tid == 0) {
      tail[0] = a;
      tail[FIT_DONE] = 1.0;
    }
  }
}

inline bool km_bad_shape(int N, int K, int R) { return K < 1 || K > KM_MAXK || R < 1 || R > KM_MAXR || N < K; }

int km_prepare(const float* X, int N, int K, int R, double* state, const KmWs& W, hipStream_t stream) {
  hipLaunchKernelGGL(kmeans_colsum_kernel, dim3(R), dim3(256), 0, stream, X, N, R, W);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(kmeans_moments_kernel, dim3(R), dim3(256), 0, stream, X, N, K, R, state, W);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // namespace

extern "C" {

size_t ladder_kmeans_state_doubles(int K, int R) { return (K < 1 || K > KM_MAXK || R < 1 || R > KM_MAXR) ? 0 : (size_t)K * R + 4; }

size_t ladder_kmeans_draws_doubles(int K) { return (K < 1 || K > KM_MAXK) ? 0 : 1 + (size_t)(K - 1) * km_trials(K); }

size_t ladder_kmeans_workspace_bytes(int N, int K, int R) {
  if (km_bad_shape(N, K, R)) return 0;
  return km_ws_doubles(N, K, R) * sizeof(double) + KI_TOTAL * sizeof(int);
}

int ladder_kmeans_seed(const float* X, int N, int K, int R, const double* draws, double* state, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (X == nullptr || draws == nullptr || state == nullptr || km_bad_shape(N, K, R)) return LADDER_E_SHAPE;
  if (fit_misaligned(draws) || fit_misaligned(state) || fit_misaligned(ws)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_kmeans_workspace_bytes(N, K, R)) return LADDER_E_SHAPE;                // (a workspace too short for the shape)
  const KmWs W = km_ws(ws, N, K, R);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = km_prepare(X, N, K, R, state, W, s);
  if (rc != LADDER_OK) return rc;
  const int ntr = km_trials(K), nb = km_blocks(N);
  for (int c = 0; c <= K; ++c) {
    hipLaunchKernelGGL(kmeans_pick_kernel, dim3(1), dim3(256), 0, s, X, N, K, R, ntr, c, draws, state, W);
    LADDER_CHECK_LAUNCH();
    if (c == K) break;
    hipLaunchKernelGGL(kmeans_cand_kernel, dim3(nb), dim3(256), 0, s, X, N, R, ntr, c, W);
    LADDER_CHECK_LAUNCH();
  }
  return LADDER_OK;
}

int ladder_kmeans_set_centres(const float* X, int N, int K, int R, const double* centres, double* state, void* ws, size_t ws_bytes,
                              ladder_stream_t stream) {
  if (X == nullptr || centres == nullptr || state == nullptr || km_bad_shape(N, K, R)) return LADDER_E_SHAPE;
  if (fit_misaligned(centres) || fit_misaligned(state) || fit_misaligned(ws)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_kmeans_workspace_bytes(N, K, R)) return LADDER_E_SHAPE;                // (a workspace too short for the shape)
  const KmWs W = km_ws(ws, N, K, R);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = km_prepare(X, N, K, R, state, W, s);
  if (rc != LADDER_OK) return rc;
  hipLaunchKernelGGL(kmeans_setc_kernel, dim3(1), dim3(256), 0, s, centres, N, K, R, state, W);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_kmeans_assign(const float* X, int N, int K, int R, int it, const double* state, int* labels, void* ws, size_t ws_bytes,
                         ladder_stream_t stream) {
  if (X == nullptr || state == nullptr || labels == nullptr || km_bad_shape(N, K, R) || it < 1) return LADDER_E_SHAPE;
  if (fit_misaligned(state) || fit_misaligned(ws)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_kmeans_workspace_bytes(N, K, R)) return LADDER_E_SHAPE;                // (a workspace too short for the shape)
  const KmWs W = km_ws(ws, N, K, R);
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3(km_slices(N)), dim3(256), 0, static_cast<hipStream_t>(stream), X, N, K, R, it, state, labels, W);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_kmeans_update(const float* X, int N, int K, int R, const int* labels, double* state, double tol, int max_iter, int it, void* ws,
                         size_t ws_bytes, ladder_stream_t stream) {
  if (X == nullptr || state == nullptr || labels == nullptr || km_bad_shape(N, K, R) || max_iter < 1 || it < 1) return LADDER_E_SHAPE;
  if (fit_misaligned(state) || fit_misaligned(ws)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_kmeans_workspace_bytes(N, K, R)) return LADDER_E_SHAPE;                // (a workspace too short for the shape)
  const KmWs W = km_ws(ws, N, K, R);
  const FitSplit sp = fit_split(N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kmeans_sums_kernel, dim3(sp.nsplit), dim3(256), 0, s, X, labels, (const double*)state, N, K, R, sp.rows, W);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(1), dim3(256), 0, s, X, labels, N, K, R, sp.nsplit, tol, max_iter, it, state, W);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
