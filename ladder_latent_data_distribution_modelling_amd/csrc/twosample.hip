// Two-sample statistics on the device: the all-pairs walks behind improved precision / recall (Kynkaanniemi et al., 2019) and the kernel inception
// distance (Binkowski et al., 2018), for feature rows [n, 512] and latent codes [n, Z] alike.
//
//   pairs_row_norms_kernel       norms[i] = sum_k (x_ik - c_k)^2, float64, k ascending
//   pairs_walk_kernel<Policy>    ONE pair-walk core, three epilogue policies:
//       KnnPolicy      the k smallest squared distances of every row of a set to the other rows of the same set (self excluded by INDEX)
//       CountPolicy    for every query row the number of reference rows whose k-NN ball holds it (d <= r2[j], non-strict)
//       PolyPolicy     for every subset block the three sums of the polynomial kernel (gamma u.v + coef0)^degree: x-x and y-y off the diagonal, x-y
//   pairs_*_merge_kernel         the per-split partials of a walk, folded in split order
//
// The core.  A workgroup of four wavefronts owns a 64-row tile of set A and walks the 64-row tiles of set B that its column split covers.  The
// contraction over D runs on v_mfma_f64_16x16x4_f64 (lane maps: head of fid.hip): wavefront w owns rows 16 w .. 16 w + 15 of the tile as four 16 x 16
// accumulators, so after a tile's last k-step lane (m = lane & 15, k = lane >> 4) holds G[16 w + k + 4 r][16 q + m] in acc[q][r].  Operands are fp32
// rows in global memory; a chunk of 32 columns of both tiles is fetched into registers (128-bit loads when D % 4 == 0 and the rows are 16-byte
// aligned) while the previous chunk is multiplied, then centred (x - c, exact in float64 for operands of like magnitude), widened and laid into LDS
// with a row stride of 34 doubles, on which the 32 lanes of a ds_read_b64 group hit 32 different banks.  Rows past the end of a set and columns past D
// enter as exact zeros AFTER centring.  LDS: 2 x 64 x 34 doubles = 34 816 bytes, static; the 64 x 65 distance tile of the k-NN epilogue and its final
// merge alias the same words between barriers.
//
// No n x m array exists in global memory: a (row tile, split) leaves k candidates, one count or one partial sum per row / per workgroup in the
// workspace.  No floating-point atomics; every floating-point sum has one fixed order (k-step order inside an accumulator; q, r order inside a lane;
// the xor butterfly over a wavefront; wavefront 0 .. 3; tile order; split order), so a call gives the same bits every time.  The k-NN radii and the
// counts are order-independent anyway (a k-th smallest value, an integer), so their column splits are free to follow the chip: pairs_best_split picks
// the split that fills PW_RESIDENT workgroup slots in the fewest whole rounds (gw_best_split of mixture_wide.hip is the precedent).  The polynomial
// sums take no column split: their subset blocks ride on blockIdx.y, and a block's bits must not depend on how many blocks share the launch.
#include "common.h"

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int PW_TILE = 64, PW_KC = 32, PW_LD = PW_KC + 2, PW_DLD = PW_TILE + 1, PW_MAXK = 8;
constexpr int PW_LDS_DOUBLES = 2 * PW_TILE * PW_LD;
constexpr int PW_MAX_D = 32768, PW_MAX_ROWS = 1 << 24, PW_MAX_BLOCKS = 65535, PW_MAX_SPLITS = 64, PW_RESIDENT = 512;      // (256 CUs x the two workgroups that every form's register count admits)
static_assert(PW_TILE * PW_DLD <= PW_LDS_DOUBLES && 4 * PW_TILE * PW_MAXK <= PW_LDS_DOUBLES, "the epilogues alias the operand staging");
static_assert(PW_LDS_DOUBLES * sizeof(double) <= 65536, "static LDS: no launch attribute");

// What a workgroup walks: rows [ti * 64, ...) of a [na, D] against the 64-row tiles t0 .. t1 - 1 of b [nb, D].
struct PwJob {
  const float *a, *b, *shift;
  int na, nb, D, ti, t0, t1;
};

// ------------------------------------------------------------------------------------------------ the core
// One chunk of 32 columns of both tiles in registers: 8 floats of A, 8 of B, the 8 shift values they share, and which of them are real.
template <bool VEC>
struct PwChunk {
  float a[8], b[8], c[8];
  unsigned va, vb;                  // bit e: element e is inside its set and inside D

  // element e of thread t: row r(e), column c(e) of the 64 x 32 chunk.  VEC: two float4 per operand (8 threads cover a row's 128 bytes);
  // scalar: eight floats, 32 threads per row.
  static __device__ __forceinline__ int row(int t, int e) { return VEC ? (t + 256 * (e >> 2)) >> 3 : (t + 256 * e) >> 5; }
  static __device__ __forceinline__ int col(int t, int e) { return VEC ? (((t + 256 * (e >> 2)) & 7) << 2) + (e & 3) : (t + 256 * e) & 31; }

  __device__ __forceinline__ void fetch(const PwJob& j, int tj, int k0) {
    const int t = threadIdx.x;
    va = vb = 0u;
    if (VEC) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int r = row(t, 4 * u), cc = k0 + col(t, 4 * u);
        const bool kin = cc < j.D;                                            // (D % 4 == 0: the four columns stand or fall together)
        const int ra = j.ti * PW_TILE + r, rb = tj * PW_TILE + r;
        float4 xa = make_float4(0.f, 0.f, 0.f, 0.f), xb = xa, xc = xa;
        if (kin && ra < j.na) { xa = *reinterpret_cast<const float4*>(j.a + (size_t)ra * j.D + cc); va |= 0xFu << (4 * u); }
        if (kin && rb < j.nb) { xb = *reinterpret_cast<const float4*>(j.b + (size_t)rb * j.D + cc); vb |= 0xFu << (4 * u); }
        if (kin && j.shift != nullptr) xc = *reinterpret_cast<const float4*>(j.shift + cc);
        a[4 * u] = xa.x, a[4 * u + 1] = xa.y, a[4 * u + 2] = xa.z, a[4 * u + 3] = xa.w;
        b[4 * u] = xb.x, b[4 * u + 1] = xb.y, b[4 * u + 2] = xb.z, b[4 * u + 3] = xb.w;
        c[4 * u] = xc.x, c[4 * u + 1] = xc.y, c[4 * u + 2] = xc.z, c[4 * u + 3] = xc.w;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int r = row(t, e), cc = k0 + col(t, e);
        const bool kin = cc < j.D;
        const int ra = j.ti * PW_TILE + r, rb = tj * PW_TILE + r;
        a[e] = b[e] = c[e] = 0.f;
        if (kin && ra < j.na) { a[e] = j.a[(size_t)ra * j.D + cc]; va |= 1u << e; }
        if (kin && rb < j.nb) { b[e] = j.b[(size_t)rb * j.D + cc]; vb |= 1u << e; }
        if (kin && j.shift != nullptr) c[e] = j.shift[cc];
      }
    }
  }

  // centre, widen, lay into LDS: As [64][PW_LD] | Bs [64][PW_LD]
  __device__ __forceinline__ void store(double* lds) const {
    const int t = threadIdx.x;
    double* As = lds;
    double* Bs = lds + PW_TILE * PW_LD;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int o = row(t, e) * PW_LD + col(t, e);
      As[o] = ((va >> e) & 1u) ? (double)a[e] - (double)c[e] : 0.0;
      Bs[o] = ((vb >> e) & 1u) ? (double)b[e] - (double)c[e] : 0.0;
    }
  }
};

// The k-steps of one staged chunk (`steps` of them: the last chunk of a D that is no multiple of 32 stops early; uniform over the workgroup).
__device__ __forceinline__ void pw_multiply(const double* lds, int steps, double4_t (&acc)[4]) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, k = lane >> 4;
  const double* ap = lds + (wave * 16 + m) * PW_LD + k;
  const double* bp = lds + PW_TILE * PW_LD + m * PW_LD + k;
  for (int s = 0; s < steps; ++s) {                                  // (left rolled: straight-line code for a whole chunk costs 60 VGPRs and a wave of occupancy)
    const double a = ap[4 * s];
    double b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] = bp[q * 16 * PW_LD + 4 * s];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[q], acc[q], 0, 0, 0);
  }
}

// The walk: for every B tile of the job, G = (A tile - c)(B tile - c)^T in acc, then policy.tile(acc, tj).  The policy may use `lds` inside tile() and
// must leave it behind a barrier.
template <bool VEC, class Policy>
__device__ __forceinline__ void pw_walk(const PwJob& j, Policy& policy, double* lds) {
  const int nchunk = (j.D + PW_KC - 1) / PW_KC;
  PwChunk<VEC> ch;
  if (j.t0 < j.t1) ch.fetch(j, j.t0, 0);
  for (int tj = j.t0; tj < j.t1; ++tj) {
    double4_t acc[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = double4_t{0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nchunk; ++c) {
      ch.store(lds);
      __syncthreads();
      if (c + 1 < nchunk) ch.fetch(j, tj, (c + 1) * PW_KC);
      else if (tj + 1 < j.t1) ch.fetch(j, tj + 1, 0);
      const int left = j.D - c * PW_KC;
      pw_multiply(lds, ((left < PW_KC ? left : PW_KC) + 3) >> 2, acc);
      __syncthreads();
    }
    policy.tile(acc, tj, lds);
  }
}

// VEC is the host's choice (pw_launch): the 128-bit form needs D % 4 == 0 and 16-byte aligned sets and shift, and then every row and every subset
// block starts on 16 bytes.  Two kernels, not one branch: the scalar form's sixteen row addresses would cost the vector form a third of its occupancy
// (132 against 189 VGPRs in the k-NN walk).
template <bool VEC, class Policy>
__global__ __launch_bounds__(256) void pairs_walk_kernel(typename Policy::Args args) {
  __shared__ double lds[PW_LDS_DOUBLES];
  Policy policy;
  PwJob j;
  policy.begin(args, j);
  pw_walk<VEC>(j, policy, lds);
  policy.finish(args, lds);
}

// ------------------------------------------------------------------------------------------------ sorted short lists
// best[0 .. 7] ascending; an insertion keeps the 8 smallest, whatever k is (callers skip values that are not below best[7]): the k-th smallest is
// best[k - 1], picked once at the very end with constant indices, so the list stays in registers.
__device__ __forceinline__ void pw_insert(double (&best)[PW_MAXK], double v) {
#pragma unroll
  for (int s = 0; s < PW_MAXK; ++s) {
    const double lo = fmin(best[s], v);
    v = fmax(best[s], v);
    best[s] = lo;
  }
}

// ------------------------------------------------------------------------------------------------ policy: k nearest neighbours inside one set
struct KnnPolicy {
  struct Args {
    const float *x, *shift;
    const double* norms;
    int n, D, k, tiles, per_split, rows_pad;
    double* cand;                  // [split][k][rows_pad]
  };
  const double* norms;
  int n, k, ti;
  double nrow[4], best[PW_MAXK];

  __device__ __forceinline__ void begin(const Args& g, PwJob& j) {
    const int nsplit = (g.tiles + g.per_split - 1) / g.per_split;
    ti = blockIdx.x / nsplit;
    const int split = blockIdx.x % nsplit;
    j = PwJob{g.x, g.x, g.shift, g.n, g.n, g.D, ti, split * g.per_split, min(g.tiles, (split + 1) * g.per_split)};
    norms = g.norms, n = g.n, k = g.k;
    const int wave = threadIdx.x >> 6, kq = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = ti * PW_TILE + wave * 16 + kq + 4 * r;
      nrow[r] = gi < n ? norms[gi] : 0.0;
    }
#pragma unroll
    for (int s = 0; s < PW_MAXK; ++s) best[s] = __builtin_inf();
  }

  // distance tile -> LDS (self and rows past the set as +inf), then thread (wave w, lane l) folds columns 16 w .. 16 w + 15 of row l into its list
  __device__ __forceinline__ void tile(const double4_t (&acc)[4], int tj, double* lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gj = tj * PW_TILE + 16 * q + m;
      const double ncol = gj < n ? norms[gj] : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = wave * 16 + kq + 4 * r;
        const double d = fmax(nrow[r] + ncol - 2.0 * acc[q][r], 0.0);
        lds[row * PW_DLD + 16 * q + m] = (gj < n && gj != ti * PW_TILE + row) ? d : __builtin_inf();
      }
    }
    __syncthreads();
    for (int c = 0; c < 16; ++c) {
      const double d = lds[lane * PW_DLD + wave * 16 + c];
      if (d < best[PW_MAXK - 1]) pw_insert(best, d);
    }
    __syncthreads();
  }

  // the four lists of a row meet in LDS; threads 0 .. 63 fold them and write the row's k candidates of this split
  __device__ __forceinline__ void finish(const Args& g, double* lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < PW_MAXK; ++s) lds[(wave * PW_TILE + lane) * PW_MAXK + s] = best[s];
    __syncthreads();
    if (wave != 0) return;
    for (int w = 1; w < 4; ++w)
      for (int s = 0; s < PW_MAXK; ++s) {
        const double d = lds[(w * PW_TILE + lane) * PW_MAXK + s];
        if (d < best[PW_MAXK - 1]) pw_insert(best, d);
      }
    const int nsplit = (g.tiles + g.per_split - 1) / g.per_split, split = blockIdx.x % nsplit;
#pragma unroll
    for (int s = 0; s < PW_MAXK; ++s)
      if (s < k) g.cand[((size_t)split * k + s) * g.rows_pad + (size_t)ti * PW_TILE + lane] = best[s];
  }
};

// r2[i] = the k-th smallest of the row's nsplit * k candidates
__global__ __launch_bounds__(256) void pairs_knn_merge_kernel(const double* __restrict__ cand, int n, int k, int nsplit, int rows_pad, double* __restrict__ r2) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double best[PW_MAXK];
#pragma unroll
  for (int s = 0; s < PW_MAXK; ++s) best[s] = __builtin_inf();
  for (int c = 0; c < nsplit * k; ++c) {
    const double d = cand[(size_t)c * rows_pad + i];
    if (d < best[PW_MAXK - 1]) pw_insert(best, d);
  }
#pragma unroll
  for (int s = 0; s < PW_MAXK; ++s)
    if (s == k - 1) r2[i] = best[s];
}

// ------------------------------------------------------------------------------------------------ policy: ball membership counts
struct CountPolicy {
  struct Args {
    const float *q, *a, *shift;
    const double *norms_q, *norms_a, *r2;
    int m, n, D, tiles, per_split, rows_pad;
    int* part;                     // [split][rows_pad]
  };
  const double *norms_a, *r2;
  int n, ti, cnt[4];
  double nrow[4];

  __device__ __forceinline__ void begin(const Args& g, PwJob& j) {
    const int nsplit = (g.tiles + g.per_split - 1) / g.per_split;
    ti = blockIdx.x / nsplit;
    const int split = blockIdx.x % nsplit;
    j = PwJob{g.q, g.a, g.shift, g.m, g.n, g.D, ti, split * g.per_split, min(g.tiles, (split + 1) * g.per_split)};
    norms_a = g.norms_a, r2 = g.r2, n = g.n;
    const int wave = threadIdx.x >> 6, kq = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gi = ti * PW_TILE + wave * 16 + kq + 4 * r;
      nrow[r] = gi < g.m ? g.norms_q[gi] : 0.0;
      cnt[r] = 0;
    }
  }

  __device__ __forceinline__ void tile(const double4_t (&acc)[4], int tj, double*) {
    const int m = threadIdx.x & 15;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gj = tj * PW_TILE + 16 * q + m;
      const bool in = gj < n;
      const double ncol = in ? norms_a[gj] : 0.0, rad = in ? r2[gj] : -1.0;
#pragma unroll
      for (int r = 0; r < 4; ++r) cnt[r] += (in && fmax(nrow[r] + ncol - 2.0 * acc[q][r], 0.0) <= rad) ? 1 : 0;
    }
  }

  __device__ __forceinline__ void finish(const Args& g, double*) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
    const int nsplit = (g.tiles + g.per_split - 1) / g.per_split, split = blockIdx.x % nsplit;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int c = cnt[r];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) c += __shfl_xor(c, o, 64);              // (the 16 lanes that share a row)
      if (m == 0) g.part[(size_t)split * g.rows_pad + (size_t)ti * PW_TILE + wave * 16 + kq + 4 * r] = c;
    }
  }
};

__global__ __launch_bounds__(256) void pairs_count_merge_kernel(const int* __restrict__ part, int m, int nsplit, int rows_pad, int* __restrict__ counts) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  int c = 0;
  for (int s = 0; s < nsplit; ++s) c += part[(size_t)s * rows_pad + i];
  counts[i] = c;
}

// ------------------------------------------------------------------------------------------------ policy: polynomial-kernel sums per subset block
struct PolyPolicy {
  struct Args {
    const float *x, *y;
    int sx, sy, D, degree, tx, ty;          // tx, ty: 64-row tiles of a block of x / of y
    double gamma, coef0;
    double* part;                           // [block][2 tx + ty]: x-x row tiles, y-y row tiles, x-y row tiles
  };
  int na, nb, ti, degree;
  bool off_diagonal;
  double gamma, coef0, sum;

  __device__ __forceinline__ void begin(const Args& g, PwJob& j) {
    const int job = blockIdx.x, blk = blockIdx.y;
    const float* xb = g.x + (size_t)blk * g.sx * g.D;
    const float* yb = g.y + (size_t)blk * g.sy * g.D;
    if (job < g.tx) j = PwJob{xb, xb, nullptr, g.sx, g.sx, g.D, job, 0, g.tx};
    else if (job < g.tx + g.ty) j = PwJob{yb, yb, nullptr, g.sy, g.sy, g.D, job - g.tx, 0, g.ty};
    else j = PwJob{xb, yb, nullptr, g.sx, g.sy, g.D, job - g.tx - g.ty, 0, g.ty};
    off_diagonal = job < g.tx + g.ty;
    na = j.na, nb = j.nb, ti = j.ti, degree = g.degree, gamma = g.gamma, coef0 = g.coef0, sum = 0.0;
  }

  __device__ __forceinline__ void tile(const double4_t (&acc)[4], int tj, double*) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, m = lane & 15, kq = lane >> 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int gj = tj * PW_TILE + 16 * q + m;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gi = ti * PW_TILE + wave * 16 + kq + 4 * r;
        const double t = gamma * acc[q][r] + coef0, t2 = t * t;
        const double v = degree == 1 ? t : degree == 2 ? t2 : degree == 3 ? t2 * t : t2 * t2;
        if (gi < na && gj < nb && !(off_diagonal && gi == gj)) sum += v;
      }
    }
  }

  __device__ __forceinline__ void finish(const Args& g, double* lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const double s = wave_sum_d(sum);
    if (lane == 0) lds[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) g.part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
  }
};

// sums[b][p] = the row-tile partials of pair set p of block b, in tile order
__global__ __launch_bounds__(64) void pairs_poly_merge_kernel(const double* __restrict__ part, int n_blocks, int tx, int ty, double* __restrict__ sums) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= 3 * n_blocks) return;
  const int b = i / 3, p = i % 3;
  const int first = p == 0 ? 0 : p == 1 ? tx : tx + ty, count = p == 1 ? ty : tx;
  const double* src = part + (size_t)b * (2 * tx + ty) + first;
  double acc = 0.0;
  for (int t = 0; t < count; ++t) acc += src[t];
  sums[i] = acc;
}

// ------------------------------------------------------------------------------------------------ row norms
__global__ __launch_bounds__(64) void pairs_row_norms_kernel(const float* __restrict__ x, int n, int D, const float* __restrict__ shift, double* __restrict__ norms) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float* row = x + (size_t)i * D;
  double acc = 0.0;
  for (int k = 0; k < D; ++k) {
    const double d = (double)row[k] - (shift != nullptr ? (double)shift[k] : 0.0);
    acc += d * d;
  }
  norms[i] = acc;
}

// ------------------------------------------------------------------------------------------------ host
inline int pw_tiles(int rows) { return (rows + PW_TILE - 1) / PW_TILE; }
inline bool pw_rows_ok(long long rows) { return rows >= 1 && rows <= PW_MAX_ROWS; }
inline bool pw_width_ok(int D) { return D >= 1 && D <= PW_MAX_D; }
inline bool pw_off8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; }

// Column tiles per split: the split count (at most PW_MAX_SPLITS) whose row_tiles * splits workgroups take the fewest whole rounds of PW_RESIDENT slots
// times the tiles a workgroup then walks; the smallest such count wins a tie.
int pairs_best_split(int row_tiles, int col_tiles) {
  int best = 1;
  long long best_cost = -1;
  for (int ks = 1; ks <= PW_MAX_SPLITS && ks <= col_tiles; ++ks) {
    const long long cost = (((long long)row_tiles * ks + PW_RESIDENT - 1) / PW_RESIDENT) * ((col_tiles + ks - 1) / ks);
    if (best_cost < 0 || cost < best_cost) {
      best = ks;
      best_cost = cost;
    }
  }
  return (col_tiles + best - 1) / best;
}

struct PwPlan {
  int row_tiles, col_tiles, per_split, nsplit, rows_pad;
};
inline PwPlan pw_plan(int rows, int cols) {
  PwPlan p;
  p.row_tiles = pw_tiles(rows), p.col_tiles = pw_tiles(cols);
  p.per_split = pairs_best_split(p.row_tiles, p.col_tiles);
  p.nsplit = (p.col_tiles + p.per_split - 1) / p.per_split;
  p.rows_pad = p.row_tiles * PW_TILE;
  return p;
}

template <class Policy>
void pw_launch(dim3 grid, ladder_stream_t stream, const typename Policy::Args& g, int D, const void* a, const void* b, const void* shift) {
  const bool vec = (D & 3) == 0 && ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(shift)) & 15u) == 0;
  if (vec) hipLaunchKernelGGL((pairs_walk_kernel<true, Policy>), grid, dim3(256), 0, stream, g);
  else hipLaunchKernelGGL((pairs_walk_kernel<false, Policy>), grid, dim3(256), 0, stream, g);
}

}  // namespace

extern "C" {

size_t ladder_pairs_workspace_bytes(int rows, int cols, int D, int k, int n_blocks) {
  if (!pw_width_ok(D) || rows < 1 || cols < 1) return 0;
  if (n_blocks == 0 && k >= 1) {                                               // k-NN radii of one set
    if (rows != cols || !pw_rows_ok(rows) || k > PW_MAXK || k > rows - 1) return 0;
    const PwPlan p = pw_plan(rows, rows);
    return (size_t)p.nsplit * k * p.rows_pad * sizeof(double);
  }
  if (n_blocks == 0 && k == 0) {                                               // ball counts: rows queries against cols balls
    if (!pw_rows_ok(rows) || !pw_rows_ok(cols)) return 0;
    const PwPlan p = pw_plan(rows, cols);
    return (size_t)p.nsplit * p.rows_pad * sizeof(int);
  }
  if (n_blocks >= 1 && n_blocks <= PW_MAX_BLOCKS && k == 0) {                  // polynomial sums: n_blocks blocks of rows x rows and cols y rows
    if (!pw_rows_ok((long long)rows * n_blocks) || !pw_rows_ok((long long)cols * n_blocks)) return 0;
    return (size_t)n_blocks * (2 * pw_tiles(rows) + pw_tiles(cols)) * sizeof(double);
  }
  return 0;
}

int ladder_pairs_row_norms(const float* x, int n, int D, const float* shift, double* norms, ladder_stream_t stream) {
  if (x == nullptr || norms == nullptr || !pw_rows_ok(n) || !pw_width_ok(D)) return LADDER_E_SHAPE;
  if (pw_off8(norms)) return LADDER_E_ALIGN;
  hipLaunchKernelGGL(pairs_row_norms_kernel, dim3((n + 63) / 64), dim3(64), 0, stream, x, n, D, shift, norms);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_pairs_knn_radii(const float* a, const double* norms_a, int n, int D, const float* shift, int k, double* r2, void* ws, size_t ws_bytes,
                           ladder_stream_t stream) {
  if (a == nullptr || norms_a == nullptr || r2 == nullptr || !pw_rows_ok(n) || !pw_width_ok(D) || k < 1 || k > PW_MAXK || k > n - 1) return LADDER_E_SHAPE;
  if (pw_off8(norms_a) || pw_off8(r2) || pw_off8(ws)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_pairs_workspace_bytes(n, n, D, k, 0)) return LADDER_E_WORKSPACE;
  const PwPlan p = pw_plan(n, n);
  KnnPolicy::Args g{a, shift, norms_a, n, D, k, p.col_tiles, p.per_split, p.rows_pad, static_cast<double*>(ws)};
  pw_launch<KnnPolicy>(dim3(p.row_tiles * p.nsplit), stream, g, D, a, a, shift);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(pairs_knn_merge_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const double*)g.cand, n, k, p.nsplit, p.rows_pad, r2);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_pairs_ball_counts(const float* q, const double* norms_q, int m, const float* a, const double* norms_a, const double* r2, int n, int D,
                             const float* shift, int* counts, void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (q == nullptr || norms_q == nullptr || a == nullptr || norms_a == nullptr || r2 == nullptr || counts == nullptr || !pw_rows_ok(m) || !pw_rows_ok(n) ||
      !pw_width_ok(D))
    return LADDER_E_SHAPE;
  if (pw_off8(norms_q) || pw_off8(norms_a) || pw_off8(r2) || (reinterpret_cast<uintptr_t>(ws) & 3u) || (reinterpret_cast<uintptr_t>(counts) & 3u)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_pairs_workspace_bytes(m, n, D, 0, 0)) return LADDER_E_WORKSPACE;
  const PwPlan p = pw_plan(m, n);
  CountPolicy::Args g{q, a, shift, norms_q, norms_a, r2, m, n, D, p.col_tiles, p.per_split, p.rows_pad, static_cast<int*>(ws)};
  pw_launch<CountPolicy>(dim3(p.row_tiles * p.nsplit), stream, g, D, q, a, shift);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(pairs_count_merge_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, (const int*)g.part, m, p.nsplit, p.rows_pad, counts);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

int ladder_pairs_poly_sums(const float* x, int sx, const float* y, int sy, int n_blocks, int D, int degree, double gamma, double coef0, double* sums,
                           void* ws, size_t ws_bytes, ladder_stream_t stream) {
  if (x == nullptr || y == nullptr || sums == nullptr || sx < 1 || sy < 1 || n_blocks < 1 || n_blocks > PW_MAX_BLOCKS || !pw_width_ok(D) || degree < 1 ||
      degree > 4 || !pw_rows_ok((long long)sx * n_blocks) || !pw_rows_ok((long long)sy * n_blocks))
    return LADDER_E_SHAPE;
  if (pw_off8(sums) || pw_off8(ws)) return LADDER_E_ALIGN;
  if (ws == nullptr || ws_bytes < ladder_pairs_workspace_bytes(sx, sy, D, 0, n_blocks)) return LADDER_E_WORKSPACE;
  const int tx = pw_tiles(sx), ty = pw_tiles(sy);
  PolyPolicy::Args g{x, y, sx, sy, D, degree, tx, ty, gamma, coef0, static_cast<double*>(ws)};
  pw_launch<PolyPolicy>(dim3(2 * tx + ty, n_blocks), stream, g, D, x, y, nullptr);
  LADDER_CHECK_LAUNCH();
  hipLaunchKernelGGL(pairs_poly_merge_kernel, dim3((3 * n_blocks + 63) / 64), dim3(64), 0, stream, (const double*)g.part, n_blocks, tx, ty, sums);
  LADDER_CHECK_LAUNCH();
  return LADDER_OK;
}

}  // extern "C"
