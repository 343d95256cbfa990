// Batched shortest-likely-path interpolation for WIDE representations (8 < R <= 64, R % 4 == 0): the loop of csrc/slp.hip -- same
// objective, same float64 path algebra, clip, Adam and record (csrc/slp_common.h, one copy for both kernels) -- with the mixture term on
// the fp32 matrix cores, read from the dense buffer of ladder_gmm_prepare_dense (Bmat [R, K*R] | BmatT [K*R, R] | bias [K*R] | logc [K]),
// the buffer the engine's mixture term uses.
//
// One workgroup (4 wavefronts) per path; paths never communicate; __syncthreads() is the only synchronisation, reached by every thread
// (n_iter, n_step, K, R are uniform); no atomics; every sum has one fixed order.
//
// Phase A per iteration, for the n = n_step points T [n, R] (fp32 roundings of the float64 points, kept in LDS with a row stride that
// spreads the 16 rows of an operand read over the banks) and component k:
//     Y_k = T Linv_k^T + bias_k,   lp[i,k] = logc_k - 0.5 |Y_k[i,:]|^2,   -d log p / d t_i = sum_k r_ik Y_k[i,:] Linv_k
// COMPONENTS ARE STRIDED OVER THE WAVEFRONTS (wavefront w takes k = w, w + 4, ...), every wavefront covers all points.  Both products run
// on v_mfma_f32_16x16x4_f32 in TRANSPOSED form, so that the second needs no re-layout of the first's result:
//   product 1   Y_k^T [c, i] = sum_j Linv_k[c, j] T[i, j]:   A = Linv_k (lane l: row c = 16 ct + (l & 15), k-index j = 4 ks + (l >> 4), read
//               from Bmat, where c is the contiguous direction: 16 consecutive floats per lane group), B = T^T from LDS (k-index j, column
//               i = 16 pt + (l & 15)), accumulator preloaded with bias_k.  D: column l & 15 = point i, rows 4 (l >> 4) + r = c.
//   the lane's point i therefore owns a quarter of row i of Y_k: |Y_k[i,:]|^2 is an in-lane sum and two xor shuffles (16, 32; every lane
//   of a point gets the same bits), and the online log-sum-exp of GMM_LSE_STEP runs per lane exactly as in the narrow kernel.
//   product 2   G^T [j, i] += sum_c Linv_k[c, j] (ex_ik Y_k[i, c]):   the k-index of a step is c = 16 ct + 4 (l >> 4) + r for fixed (ct, r)
//               -- a permutation of the order of c that A and B share -- so B is the lane's OWN accumulator register r of tile ct scaled
//               by ex, and A = Linv_k[c, j = 16 jt + (l & 15)] is read from BmatT, where j is the contiguous direction.  Before the
//               step the accumulators of the point are rescaled by the log-sum-exp factor sc: no [n, K*R] intermediate exists.
// Each wavefront thus fetches each Linv_k it owns once per iteration for each product (never per point or per point tile), straight into
// the MFMA operand registers and a whole component's operands per batch (see "Operand fetch" below): with components on wavefronts no
// two wavefronts share a weight, so an LDS slab would only add a copy.
// Rows c >= R and columns j >= R of the 16-wide tiles (R = 12, 20, ...) are zero operands; point rows >= n_step are zero rows of T whose
// results are never read.
// Merge: the wavefronts publish (max, sum) per point, every wavefront forms the common maximum, rescales its gradient and the four
// partial gradients are added into s_gn in the order 0, 1, 2, 3 with a barrier between (one [n, R] fp32 buffer instead of four); the
// last one divides by the total sum.  The LAST wavefront -- the one with the fewest components when K is no multiple of 4 -- also does the
// path algebra, as in the narrow kernel.
// Phase B is slp_clip_adam_record; the thread that updates an element also refreshes its fp32 copy.
#include <mutex>
#include "common.h"
#include "gmm_packed.h"
#include "slp_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SLPW_MAX_R = 64, SLPW_MAX_ELEMS = 2048;          // n_step * R <= 2048 (codes/interpolation.py: MAX_POINTS_WIDE)
constexpr size_t SLPW_MAX_LDS = 128 * 1024;

// Row stride of the fp32 points: lane l reads word (l & 15) * TS + (l >> 4) (+ const); with TS / 4 odd the 64 words fall into 64 banks.
__host__ __device__ inline int slpw_tstride(int R) { return ((R / 4) & 1) ? R : R + 4; }

// Dynamic LDS layout: doubles first, then floats (16-byte aligned for the float4 accesses of s_gn).
struct SlpwLayout {
  int full, m, v, unit, c, scal, n_double;                       // offsets in doubles
  int gn, lp, mx, se, t32, n_float;                              // offsets in floats behind the doubles
  __host__ __device__ SlpwLayout(int n, int R, int n_pad) {
    const int ne = n * R;
    full = 0;
    m = full + (n + 2) * R;
    v = m + ne;
    unit = v + ne;
    c = unit + (n + 1) * R;
    scal = c + ((n + 2) & ~1);
    n_double = scal + 4;
    gn = 0;
    lp = gn + ne;
    mx = lp + SLP_MAX_STEP;
    se = mx + SLP_WAVES * SLP_MAX_STEP;
    t32 = se + SLP_WAVES * SLP_MAX_STEP;
    n_float = t32 + n_pad * slpw_tstride(R);
  }
  __host__ __device__ size_t bytes() const { return (size_t)n_double * sizeof(double) + (size_t)n_float * sizeof(float); }
};

// RT = ceil(R / 16) tiles over R, NT = ceil(n_step / 16) tiles over the points.
template <int RT, int NT>
__global__ __launch_bounds__(SLP_THREADS) void slp_wide_optimise_kernel(SlpArgs A, const int R) {
  extern __shared__ double slpw_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l15 = lane & 15, g = lane >> 4;
  const int n = A.n_step, ne = n * R, K = A.K, KR = K * R, TS = slpw_tstride(R);
  const size_t p = blockIdx.x;
  const SlpwLayout Lo(n, R, NT * 16);
  double *s_full = slpw_lds + Lo.full, *s_m = slpw_lds + Lo.m, *s_v = slpw_lds + Lo.v, *s_unit = slpw_lds + Lo.unit, *s_c = slpw_lds + Lo.c,
         *s_scal = slpw_lds + Lo.scal;
  float* s_f = reinterpret_cast<float*>(slpw_lds + Lo.n_double);
  float *s_gn = s_f + Lo.gn, *s_lp = s_f + Lo.lp, *s_mx = s_f + Lo.mx, *s_se = s_f + Lo.se, *s_t = s_f + Lo.t32;
  const double* s_pts = s_full + R;
  const float *Bmat = A.packed, *BmatT = Bmat + (size_t)R * KR, *bias = BmatT + (size_t)R * KR, *logc = bias + KR;

  slp_load_path(A, R, tid, p, s_full, s_m, s_v);
  for (int e = tid; e < NT * 16 * TS; e += SLP_THREADS) s_t[e] = 0.f;      // zero rows of the padded point tiles (and the stride's padding)
  __syncthreads();
  for (int e = tid; e < ne; e += SLP_THREADS) {
    const int i = e / R;
    s_t[i * TS + (e - i * R)] = (float)s_pts[e];
  }
  __syncthreads();

  for (int it = 0; it < A.n_iter; ++it) {
    // ---- phase A: this wavefront's components at all points
    float mx[NT], se[NT];
    f32x4 G[NT][RT];
#pragma unroll
    for (int pt = 0; pt < NT; ++pt) {
      mx[pt] = -INFINITY;
      se[pt] = 0.f;
#pragma unroll
      for (int jt = 0; jt < RT; ++jt) G[pt][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // Operand fetch.  KS = 4 RT k-steps cover R (steps at or past R / 4 are zero operands: R = 12, 20, ...).  All A operands of a component
    // -- KS x RT registers per product -- are requested in one batch, so a wavefront waits for the L2 once per batch and not once per
    // k-step: product 2's batch is requested before product 1's MFMAs, the NEXT component's product-1 batch before product 2's.
    constexpr int KS = 4 * RT;
    auto load_a1 = [&](int k, float (&a1)[KS][RT]) {             // a1[ks][ct] = Linv_k[c = 16 ct + l15, j = 4 ks + g], from Bmat (c contiguous)
      const float* Bk = Bmat + (size_t)min(k, K - 1) * R;        // (past the last component: a valid address, the values are not used)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int ct = 0; ct < RT; ++ct)
          a1[ks][ct] = (4 * ks < R && 16 * ct + l15 < R) ? Bk[(size_t)(4 * ks + g) * KR + 16 * ct + l15] : 0.f;
    };
    float a1[KS][RT];
    load_a1(wv, a1);
    for (int k = wv; k < K; k += SLP_WAVES) {
      const float* BTk = BmatT + (size_t)k * R * R;              // BTk[c * R + j] = Linv_k[c, j] (j contiguous)
      float a2[KS][RT];                                          // a2[4 ct + r][jt] = Linv_k[c = 16 ct + 4 g + r, j = 16 jt + l15]
#pragma unroll
      for (int ct = 0; ct < RT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int c = 16 * ct + 4 * g + r;
#pragma unroll
          for (int jt = 0; jt < RT; ++jt) a2[4 * ct + r][jt] = (c < R && 16 * jt + l15 < R) ? BTk[(size_t)c * R + 16 * jt + l15] : 0.f;
        }
      f32x4 y[NT][RT];
#pragma unroll
      for (int ct = 0; ct < RT; ++ct) {
        const int c0 = 16 * ct + 4 * g;                          // (c0 and R are multiples of 4: the four rows are inside R together)
        const f32x4 b4 = c0 < R ? *reinterpret_cast<const f32x4*>(bias + (size_t)k * R + c0) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int pt = 0; pt < NT; ++pt) y[pt][ct] = b4;
      }
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        float b[NT];
#pragma unroll
        for (int pt = 0; pt < NT; ++pt) b[pt] = (4 * ks < R) ? s_t[(16 * pt + l15) * TS + 4 * ks + g] : 0.f;
#pragma unroll
        for (int pt = 0; pt < NT; ++pt)
#pragma unroll
          for (int ct = 0; ct < RT; ++ct) y[pt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[ks][ct], b[pt], y[pt][ct], 0, 0, 0);
      }
      load_a1(k + SLP_WAVES, a1);
      const float lc = logc[k];
      float ex_[NT];
#pragma unroll
      for (int pt = 0; pt < NT; ++pt) {
        float q = 0.f;
#pragma unroll
        for (int ct = 0; ct < RT; ++ct)
#pragma unroll
          for (int r = 0; r < 4; ++r) q += y[pt][ct][r] * y[pt][ct][r];
        q += __shfl_xor(q, 16, 64);
        q += __shfl_xor(q, 32, 64);
        const float lp = lc - 0.5f * q;
        GMM_LSE_STEP(lp, mx[pt], sc, ex);
        se[pt] = se[pt] * sc + ex;
        ex_[pt] = ex;
#pragma unroll
        for (int jt = 0; jt < RT; ++jt) G[pt][jt] *= sc;
      }
#pragma unroll
      for (int ct = 0; ct < RT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int pt = 0; pt < NT; ++pt) {
            const float w = ex_[pt] * y[pt][ct][r];
#pragma unroll
            for (int jt = 0; jt < RT; ++jt) G[pt][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[4 * ct + r][jt], w, G[pt][jt], 0, 0, 0);
          }
    }
    if (g == 0) {
#pragma unroll
      for (int pt = 0; pt < NT; ++pt) {
        s_mx[wv * SLP_MAX_STEP + 16 * pt + l15] = mx[pt];
        s_se[wv * SLP_MAX_STEP + 16 * pt + l15] = se[pt];
      }
    }
    if (wv == SLP_WAVES - 1) slp_path_algebra(A, R, lane, it, s_full, s_unit, s_c, s_scal);
    __syncthreads();

    // ---- merge over the wavefronts, in the order 0, 1, 2, 3
    float f_[NT], inv_[NT];
#pragma unroll
    for (int pt = 0; pt < NT; ++pt) {
      const int i = 16 * pt + l15;
      float gm = s_mx[i];
#pragma unroll
      for (int w = 1; w < SLP_WAVES; ++w) gm = fmaxf(gm, s_mx[w * SLP_MAX_STEP + i]);
      float tot = 0.f;
#pragma unroll
      for (int w = 0; w < SLP_WAVES; ++w) {
        const float mw = s_mx[w * SLP_MAX_STEP + i];
        tot += s_se[w * SLP_MAX_STEP + i] * ((mw == -INFINITY) ? 0.f : __expf(mw - gm));   // wavefronts without a component
      }
      f_[pt] = (mx[pt] == -INFINITY) ? 0.f : __expf(mx[pt] - gm);
      inv_[pt] = 1.f / tot;
      if (wv == 0 && g == 0 && i < n) s_lp[i] = gm + logf(tot);
    }
#pragma unroll
    for (int w = 0; w < SLP_WAVES; ++w) {
      if (wv == w) {
#pragma unroll
        for (int pt = 0; pt < NT; ++pt) {
          const int i = 16 * pt + l15;
#pragma unroll
          for (int jt = 0; jt < RT; ++jt) {
            const int j0 = 16 * jt + 4 * g;
            if (i < n && j0 < R) {
              f32x4* dst = reinterpret_cast<f32x4*>(s_gn + i * R + j0);
              f32x4 val = G[pt][jt] * f_[pt];
              if (w > 0) val = *dst + val;
              if (w == SLP_WAVES - 1) val *= inv_[pt];             // -d lp / d t_j = sum_k r_k (Sigma_k^-1 (t - m_k))_j
              *dst = val;
            }
          }
        }
      }
      __syncthreads();
    }

    // ---- phase B: clip + Adam on the n_step * R elements, record row; then the fp32 copy of the elements this thread moved
    slp_clip_adam_record(A, R, tid, p, it, s_full, s_m, s_v, s_unit, s_c, s_scal, s_gn, s_lp);
    for (int e = tid; e < ne; e += SLP_THREADS) {
      const int i = e / R;
      s_t[i * TS + (e - i * R)] = (float)s_pts[e];
    }
    __syncthreads();
  }

  slp_store_path(A, R, tid, p, s_full, s_m, s_v);
}

template <int RT, int NT>
int slpw_launch(const SlpArgs& A, int R, int P, size_t lds, hipStream_t stream) {
  // allow > 64 KB of dynamic LDS (gfx950: 160 KB per workgroup) -- once per process and instantiation, safe under concurrent callers
  static std::once_flag attr_once;
  static hipError_t attr_rc = hipSuccess;
  std::call_once(attr_once, [] {
    attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(slp_wide_optimise_kernel<RT, NT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SLPW_MAX_LDS);
  });
  if (attr_rc != hipSuccess) return LADDER_E_LAUNCH;
  hipLaunchKernelGGL((slp_wide_optimise_kernel<RT, NT>), dim3((unsigned)P), dim3(SLP_THREADS), lds, stream, A, R);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

template <int RT>
int slpw_launch_nt(int nt, const SlpArgs& A, int R, int P, size_t lds, hipStream_t stream) {
  switch (nt) {
    case 1: return slpw_launch<RT, 1>(A, R, P, lds, stream);
    case 2: return slpw_launch<RT, 2>(A, R, P, lds, stream);
    case 3: return slpw_launch<RT, 3>(A, R, P, lds, stream);
    default:                                                     // (RT = 4 means R >= 52: n_step * R <= 2048 leaves at most 3 point tiles)
      if constexpr (RT < 4) return slpw_launch<RT, 4>(A, R, P, lds, stream);
      return LADDER_E_SHAPE;
  }
}

bool slpw_shape_ok(int n_step, int R) {
  return R > 8 && R <= SLPW_MAX_R && R % 4 == 0 && n_step >= 1 && n_step <= SLP_MAX_STEP && n_step * R <= SLPW_MAX_ELEMS;
}

}  // namespace

extern "C" {

size_t ladder_slp_wide_state_bytes(int P, int n_step, int R) {
  if (P < 1 || !slpw_shape_ok(n_step, R)) return 0;
  return (size_t)3 * P * n_step * R * sizeof(double);
}

int ladder_slp_wide_optimise(const float* start, const float* end, float* pts, const float* params, int K, int R, int P, int n_step, int n_iter,
                             int t0, double lr, double beta1, double beta2, double eps, double clip, double w_path, double w_equal, double* state,
                             double* record, ladder_stream_t stream) {
  if (start == nullptr || end == nullptr || pts == nullptr || params == nullptr) return LADDER_E_SHAPE;
  if (!slpw_shape_ok(n_step, R) || K < 1 || K > 1024 || P < 1 || n_iter < 1 || n_iter > 4096 || t0 < 0) return LADDER_E_SHAPE;
  if (t0 > 0 && state == nullptr) return LADDER_E_SHAPE;
  const int nt = (n_step + 15) / 16, rt = (R + 15) / 16;
  const size_t lds = SlpwLayout(n_step, R, nt * 16).bytes();
  if (lds > SLPW_MAX_LDS) return LADDER_E_SHAPE;
  SlpArgs A{start, end, pts, params, K, n_step, n_iter, t0, lr, beta1, beta2, eps, clip, w_path, w_equal, state, record, (size_t)P * n_step * R};
  switch (rt) {
    case 1: return slpw_launch_nt<1>(nt, A, R, P, lds, (hipStream_t)stream);
    case 2: return slpw_launch_nt<2>(nt, A, R, P, lds, (hipStream_t)stream);
    case 3: return slpw_launch_nt<3>(nt, A, R, P, lds, (hipStream_t)stream);
    default: return slpw_launch_nt<4>(nt, A, R, P, lds, (hipStream_t)stream);
  }
}

}  // extern "C"
