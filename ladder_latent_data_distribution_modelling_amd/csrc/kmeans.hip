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
//
// The workspace, the preparation, seeding and cluster-sum kernels and the checks of the exported calls are in csrc/kmeans_common.h, shared with
// csrc/kmeans_wide.hip (64 < R <= 256); this file has the assignment and the update for R <= 64 and the ladder_kmeans_* entries.
#include "kmeans_common.h"

namespace {

constexpr int KM_MAXR = 64;

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

}  // namespace

extern "C" {

size_t ladder_kmeans_state_doubles(int K, int R) { return (K < 1 || K > KM_MAXK || R < 1 || R > KM_MAXR) ? 0 : (size_t)K * R + 4; }

size_t ladder_kmeans_draws_doubles(int K) { return (K < 1 || K > KM_MAXK) ? 0 : 1 + (size_t)(K - 1) * km_trials(K); }

size_t ladder_kmeans_workspace_bytes(int N, int K, int R) { return km_bad_shape(N, K, R) ? 0 : km_ws_bytes(N, K, R, false); }

int ladder_kmeans_seed(const float* X, int N, int K, int R, const double* draws, double* state, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  const int rc = km_check(km_bad_shape(N, K, R), X, draws, state, ws, ws_bytes, ladder_kmeans_workspace_bytes(N, K, R));
  if (rc != LADDER_OK) return rc;
  return km_seed<KM_MAXR, 1>(X, N, K, R, draws, state, km_ws(ws, N, K, R, false), static_cast<hipStream_t>(stream));
}

int ladder_kmeans_set_centres(const float* X, int N, int K, int R, const double* centres, double* state, void* ws, size_t ws_bytes,
                              ladder_stream_t stream) {
  const int rc = km_check(km_bad_shape(N, K, R), X, centres, state, ws, ws_bytes, ladder_kmeans_workspace_bytes(N, K, R));
  if (rc != LADDER_OK) return rc;
  return km_set_centres(X, N, K, R, centres, state, km_ws(ws, N, K, R, false), static_cast<hipStream_t>(stream));
}

int ladder_kmeans_assign(const float* X, int N, int K, int R, int it, const double* state, int* labels, void* ws, size_t ws_bytes,
                         ladder_stream_t stream) {
  const int rc = km_check(km_bad_shape(N, K, R) || labels == nullptr || it < 1, X, state, state, ws, ws_bytes, ladder_kmeans_workspace_bytes(N, K, R));
  if (rc != LADDER_OK) return rc;
  const KmWs W = km_ws(ws, N, K, R, false);
  hipLaunchKernelGGL(kmeans_assign_kernel, dim3(km_slices(N)), dim3(256), 0, static_cast<hipStream_t>(stream), X, N, K, R, it, state, labels, W);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_kmeans_update(const float* X, int N, int K, int R, const int* labels, double* state, double tol, int max_iter, int it, void* ws,
                         size_t ws_bytes, ladder_stream_t stream) {
  const int rc = km_check(km_bad_shape(N, K, R) || labels == nullptr || max_iter < 1 || it < 1, X, state, state, ws, ws_bytes,
                          ladder_kmeans_workspace_bytes(N, K, R));
  if (rc != LADDER_OK) return rc;
  const KmWs W = km_ws(ws, N, K, R, false);
  const FitSplit sp = fit_split(N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kmeans_sums_kernel, dim3(sp.nsplit, 1), dim3(256), 0, s, X, labels, (const double*)state, N, K, R, sp.rows, W);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(kmeans_update_kernel, dim3(1), dim3(256), 0, s, X, labels, N, K, R, sp.nsplit, tol, max_iter, it, state, W);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
