// K-means on the device for WIDE samples: the algorithm, conventions, state, draws and protocol of csrc/kmeans.hip (read its header comment first) for the
// widths of the wide EM fit (csrc/emgmm_wide.hip): fp32 samples [N, R], 64 < R <= 256, R % 16 == 0, 1 <= K <= 64, N >= K.  Preparation, seeding and the
// per-split cluster sums are the kernels of csrc/kmeans_common.h (the seeding's candidate distances with 16 lanes per sample instead of one thread
// walking a 1 KB row); what 64 x 256 doubles of centres (128 KB) do not allow to carry over is here:
//   kmwide_assign_kernel   a workgroup owns 64 samples and walks the columns in panels of 64: per panel it stages that panel of the shifted centres in LDS
//                          (pitch 66, 33 KB) and the lane's 16 A operands, and carries the x~.c accumulators of the (up to four) centre tiles across
//                          the panels on v_mfma_f64_16x16x4_f64.  |c_k|^2 is formed once, a lane per centre adding its panel from LDS in column order.
//                          After the last panel: |c|^2 - 2 x~.c, argmin with the lowest index winning, then the squared distance to the own centre by
//                          direct differences against the centres in global memory.  Trip counts are uniform: every lane reaches every MFMA and barrier.
//   kmeans_sums_kernel     (common) with a grid dimension over the 64-column groups; partials [nsplit, K, R]
//   kmwide_reduce_kernel   grid-wide: the partials added in split order, per element -> cluster sums [K, R] in the workspace
//   kmwide_update_kernel   ONE workgroup, on those sums in global memory, only what is serial: empty-cluster relocation, averaging, the centre shift
//                          (per cluster: a wavefront's lanes over the columns, then the shuffle tree; then k ascending), tol_, the convergence test
//                          and the final inertia -- the rules of kmeans_update_kernel.
#include "kmeans_common.h"

namespace {

constexpr int KW_MINR = 64, KW_MAXR = 256, KW_STEP = 16;           // exclusive minimum: R <= 64 is csrc/kmeans.hip's
constexpr int KW_SEED_LANES = 16;                                  // kmeans_cand_kernel: lanes that share one sample's row (R % 16 == 0)

// v, or +0.0: the bits of v under a mask
__device__ __forceinline__ double kw_keep(double v, bool keep) { return __longlong_as_double(__double_as_longlong(v) & -(long long)keep); }

// ------------------------------------------------------------------------------------------------ assignment
__global__ __launch_bounds__(256) void kmwide_assign_kernel(const float* __restrict__ X, int N, int K, int R, int it, const double* __restrict__ state,
                                                            int* __restrict__ labels, KmWs W) {
  if (state[(size_t)K * R + FIT_DONE] != 0.0) return;              // the fit is over: iterations enqueued past the end are no-ops
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, kq = lane >> 4;
  const int n0 = blockIdx.x * KM_SLICE, rows = min(KM_SLICE, N - n0);
  __shared__ double s_C[KM_MAXK * KM_LDC], s_cn[KM_MAXK], s_sh[KW_MAXR];
  __shared__ int s_cnt[KM_MAXK], s_chg;
  const int nkb = (K + 15) / 16, Kp = nkb * 16, npanel = (R + KM_PANEL - 1) / KM_PANEL;
  if (tid < R) s_sh[tid] = km_shift(W, N, tid);                     // (R <= 256 = the block)
  if (tid < KM_MAXK) s_cnt[tid] = 0;
  if (tid == 0) s_chg = 0;
  const int row = wave * 16 + m;
  const bool rv = row < rows;
  const float* xr = X + (size_t)(n0 + (rv ? row : 0)) * R;         // (row n0 exists: never dereferenced unless rv)
  double4_t acc[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) acc[kb] = double4_t{0.0, 0.0, 0.0, 0.0};
  double cn = 0.0;                                                 // tid < K: |c_tid|^2, columns ascending
  for (int p = 0; p < npanel; ++p) {                               // (uniform)
    const int j0 = p * KM_PANEL, pc = min(KM_PANEL, R - j0), nsteps = pc / 4;        // (R % 16 == 0: whole k-steps)
    for (int idx = tid; idx < Kp * KM_PANEL; idx += 256) {         // the panel of the centres, zero past K and past the panel's columns
      const int i = idx / KM_PANEL, j = idx - i * KM_PANEL;
      s_C[i * KM_LDC + j] = (i < K && j < pc) ? W.cs[(size_t)i * R + j0 + j] : 0.0;
    }
    __syncthreads();                                               // (p == 0: also s_sh)
    if (tid < K)
      for (int j = 0; j < pc; ++j) {
        const double v = s_C[tid * KM_LDC + j];
        cn += v * v;
      }
    double xa[16];                                                 // this lane's A operands of the panel: x~[row][j0 + 4 s + kq], zero past the panel
#pragma unroll
    for (int s = 0; s < 16; ++s) {                                 // (no branch around a load, so the 16 are in flight together: past the panel
      const int i = 4 * s + kq, ic = j0 + min(i, pc - 1);          // the last column is read again, and masked by bits so that no branch comes
      xa[s] = kw_keep((double)xr[ic] - s_sh[ic], rv && i < pc);    // back: measured, a select here compiles to one and the loads queue up)
    }
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      if (kb < nkb) {                                              // (uniform: every lane reaches every MFMA)
        const double* cr = s_C + (16 * kb + m) * KM_LDC + kq;
#pragma unroll
        for (int s = 0; s < 16; ++s)
          if (s < nsteps) acc[kb] = __builtin_amdgcn_mfma_f64_16x16x4f64(xa[s], cr[4 * s], acc[kb], 0, 0, 0);
      }
    }
    __syncthreads();                                               // (every operand is read before the next panel overwrites s_C)
  }
  if (tid < KM_MAXK) s_cn[tid] = tid < K ? cn : INFINITY;           // a padded centre never wins
  __syncthreads();
  double bv[4] = {INFINITY, INFINITY, INFINITY, INFINITY};
  int bi[4] = {0, 0, 0, 0};
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    if (kb < nkb) {
      const double ck = s_cn[16 * kb + m];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double sc = ck - 2.0 * acc[kb][r];
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
    const int kc = min(bi[r], K - 1);                              // (bi < K already: a finite score beats every padded centre; K >= 1)
    double p = 0.0;                                                // |x~ - c_k|^2 by direct differences: columns m, m + 16, ..., then the 16 lanes
    {
      const float* xq = X + (size_t)(n0 + (ok ? rr : 0)) * R + m;  // (as above: row n0 exists, no branch around a load, clamped columns)
      const double* ck = W.cs + (size_t)kc * R + m;
      float xs[KW_MAXR / 16];
      double cv[KW_MAXR / 16];
#pragma unroll
      for (int i = 0; i < KW_MAXR / 16; ++i) {
        const int jj = 16 * min(i, R / 16 - 1);
        xs[i] = xq[jj];
        cv[i] = ck[jj];
      }
#pragma unroll
      for (int i = 0; i < KW_MAXR / 16; ++i)
        if (16 * i < R) {
          const double d = ((double)xs[i] - s_sh[m + 16 * i]) - cv[i];
          p += d * d;
        }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) p += __shfl_xor(p, o, 64);
    if (ok && m == 0) {
      const int n = n0 + rr;
      const int old = it <= 1 ? -1 : labels[n];
      labels[n] = kc;
      W.dist[n] = p;
      if (old != kc) atomicAdd(&s_chg, 1);
      atomicAdd(&s_cnt[kc], 1);
    }
  }
  __syncthreads();
  if (tid < K && s_cnt[tid] != 0) atomicAdd(&W.ints[KI_CNT + tid], s_cnt[tid]);
  if (tid == 0 && s_chg != 0) atomicAdd(&W.ints[KI_CHANGED], s_chg);
}

// ------------------------------------------------------------------------------------------------ cluster sums: the splits
__global__ __launch_bounds__(256) void kmwide_reduce_kernel(const double* __restrict__ state, int K, int R, int nsplit, KmWs W) {
  if (state[(size_t)K * R + FIT_DONE] != 0.0 || W.ints[KI_PENDING] != 0) return;       // over, or only the final assignment is left
  const int e = blockIdx.x * 256 + threadIdx.x, KR = K * R;
  if (e >= KR) return;
  double a = 0.0;
  for (int s = 0; s < nsplit; ++s) a += W.part[(size_t)s * KR + e];
  W.sum[e] = a;
}

// ------------------------------------------------------------------------------------------------ update
__global__ __launch_bounds__(256) void kmwide_update_kernel(const float* __restrict__ X, const int* __restrict__ labels, int N, int K, int R, double tol,
                                                            int max_iter, int it, double* __restrict__ state, KmWs W) {
  double* tail = state + (size_t)K * R;
  if (tail[FIT_DONE] != 0.0) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, KR = K * R;
  __shared__ double s_sh[KW_MAXR], s_sq[KM_MAXK], s_rd[256], s_w[4];
  __shared__ int s_cnt[KM_MAXK], s_el[KM_MAXK], s_taken[KM_MAXK], s_rn[256], s_ne, s_far, s_old, s_fin;
  double* sum = W.sum;                                              // (this workgroup alone reads and writes it: barriers order the accesses)
  bool finish = W.ints[KI_PENDING] != 0;                            // the final assignment has run: only inertia_ is left
  if (!finish) {
    const int changed = W.ints[KI_CHANGED];
    if (tid < KM_MAXK) s_cnt[tid] = tid < K ? W.ints[KI_CNT + tid] : 0;
    if (tid < R) s_sh[tid] = km_shift(W, N, tid);
    if (tid == 0) s_fin = 0;
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
        sum[s_old * R + tid] -= xt;
        sum[s_el[e] * R + tid] = xt;
      }
      __syncthreads();
    }
    for (int e = tid; e < KR; e += 256) {                           // _average_centers: centre *= 1 / weight where the weight is positive
      const int cnt = s_cnt[e / R];
      if (cnt > 0) sum[e] *= 1.0 / (double)cnt;
    }
    __syncthreads();
    for (int k = wave; k < K; k += 4) {                             // |c_new - c_old|^2 of cluster k: whole wavefronts, columns lane, lane + 64, ...
      double a = 0.0;
      for (int j = lane; j < R; j += 64) {
        const double d = sum[k * R + j] - W.cs[(size_t)k * R + j];
        a += d * d;
      }
      a = wave_sum_d(a);
      if (lane == 0) s_sq[k] = a;
    }
    double mv = 0.0;                                                // tol_ = tol * mean(var(X, axis=0)), from the shifted moments
    if (tid < R) {
      const double mu = W.s1[tid] / (double)N;
      mv = W.s2[tid] / (double)N - mu * mu;
    }
    mv = block_sum_256(mv, s_w, tid);                               // (its barriers also close s_sq and the reads of W.cs)
    for (int e = tid; e < KR; e += 256) {
      W.cs[e] = sum[e];
      state[e] = sum[e] + s_sh[e % R];
    }
    if (tid == 0) {
      double shift = 0.0;
      for (int k = 0; k < K; ++k) shift += s_sq[k];
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

inline bool kw_bad_width(int K, int R) { return K < 1 || K > KM_MAXK || R <= KW_MINR || R > KW_MAXR || R % KW_STEP != 0; }
inline bool kw_bad_shape(int N, int K, int R) { return kw_bad_width(K, R) || N < K; }

}  // namespace

extern "C" {

size_t ladder_kmeans_wide_state_doubles(int K, int R) { return kw_bad_width(K, R) ? 0 : (size_t)K * R + 4; }

size_t ladder_kmeans_wide_workspace_bytes(int N, int K, int R) { return kw_bad_shape(N, K, R) ? 0 : km_ws_bytes(N, K, R, true); }

int ladder_kmeans_wide_seed(const float* X, int N, int K, int R, const double* draws, double* state, void* ws, size_t ws_bytes,
                            ladder_stream_t stream) {
  const int rc = km_check(kw_bad_shape(N, K, R), X, draws, state, ws, ws_bytes, ladder_kmeans_wide_workspace_bytes(N, K, R));
  if (rc != LADDER_OK) return rc;
  return km_seed<KW_MAXR, KW_SEED_LANES>(X, N, K, R, draws, state, km_ws(ws, N, K, R, true), static_cast<hipStream_t>(stream));
}

int ladder_kmeans_wide_set_centres(const float* X, int N, int K, int R, const double* centres, double* state, void* ws, size_t ws_bytes,
                                   ladder_stream_t stream) {
  const int rc = km_check(kw_bad_shape(N, K, R), X, centres, state, ws, ws_bytes, ladder_kmeans_wide_workspace_bytes(N, K, R));
  if (rc != LADDER_OK) return rc;
  return km_set_centres(X, N, K, R, centres, state, km_ws(ws, N, K, R, true), static_cast<hipStream_t>(stream));
}

int ladder_kmeans_wide_assign(const float* X, int N, int K, int R, int it, const double* state, int* labels, void* ws, size_t ws_bytes,
                              ladder_stream_t stream) {
  const int rc = km_check(kw_bad_shape(N, K, R) || labels == nullptr || it < 1, X, state, state, ws, ws_bytes,
                          ladder_kmeans_wide_workspace_bytes(N, K, R));
  if (rc != LADDER_OK) return rc;
  const KmWs W = km_ws(ws, N, K, R, true);
  hipLaunchKernelGGL(kmwide_assign_kernel, dim3(km_slices(N)), dim3(256), 0, static_cast<hipStream_t>(stream), X, N, K, R, it, state, labels, W);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_kmeans_wide_update(const float* X, int N, int K, int R, const int* labels, double* state, double tol, int max_iter, int it, void* ws,
                              size_t ws_bytes, ladder_stream_t stream) {
  const int rc = km_check(kw_bad_shape(N, K, R) || labels == nullptr || max_iter < 1 || it < 1, X, state, state, ws, ws_bytes,
                          ladder_kmeans_wide_workspace_bytes(N, K, R));
  if (rc != LADDER_OK) return rc;
  const KmWs W = km_ws(ws, N, K, R, true);
  const FitSplit sp = fit_split(N);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(kmeans_sums_kernel, dim3(sp.nsplit, (R + KM_PANEL - 1) / KM_PANEL), dim3(256), 0, s, X, labels, (const double*)state, N, K, R,
                     sp.rows, W);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(kmwide_reduce_kernel, dim3((K * R + 255) / 256), dim3(256), 0, s, (const double*)state, K, R, sp.nsplit, W);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(kmwide_update_kernel, dim3(1), dim3(256), 0, s, X, labels, N, K, R, tol, max_iter, it, state, W);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
