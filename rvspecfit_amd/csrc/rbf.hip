// Multiquadric radial-basis interpolation with S right-hand sides: what
// regularize_grid.converter asks of scipy's RBFInterpolator (regularize_grid.py:118-140;
// scipy/interpolate/_rbfinterp.py: _build_system, _build_and_solve_system,
// _chunk_evaluator) for kernel='multiquadric', degree 0.  fp64 throughout; ordinary
// vector loads and stores only; steps are ordered by launches, no block waits on another.
//
//     K[i,j] = -sqrt(|eps y_i - eps y_j|^2 + 1)
//     [ K + diag(s)  1 ] [ c   ]   [ d ]
//     [ 1^T          0 ] [ lam ] = [ 0 ]
//     out[m,:] = sum_j -sqrt(|eps x_m - eps y_j|^2 + 1) c[j,:] + lam
//
// K is positive definite on {c : sum c = 0}.  With A = K + diag(s) + a 1 1^T and
// 1^T c = 0, A c = (K + diag(s)) c = d - 1 lam, so with U = A^-1 d and w = A^-1 1
//     lam = (1^T U) / (1^T w),    c = U - w lam:
// one blocked Cholesky of A and one more right-hand side (the column of ones) instead
// of a pivoted LU of the bordered matrix.  a = sqrt(|eps (max y - min y)|^2 + 1), the
// kernel of the bounding box's diagonal, is >= max |K_ij|.  That A is positive definite
// for it is an observation, not a theorem: a pivot that is not finite and above
// 8 N eps a (what the rounding of the row's N products leaves of an exact zero:
// coincident nodes) sets RVS_ST_RBF_NOTPD and the caller raises.
//
// The factor is held as [Np, Np] row-major, Np = N rounded up to RBF_NB, the padding an
// identity; the right-hand sides as X [Np, ldx], ldx = S + 1 rounded up to 16, padding
// rows zero: no kernel needs a bound in the N direction.
#include "common.h"

#define RBF_NB 64     // block of the factorisation and of the triangular solves
#define RBF_BM 64     // tile of the product kernels: BM x BN outputs, slabs of BK
#define RBF_BN 128
#define RBF_BK 32
// As [m][k]: a fragment read (16 rows x 2 k per half wave, ds_read_b64) lands on
// (2 (34 r + kq)) mod 64 = 32 distinct bank pairs; Bs [k][n]: 16 consecutive n, the
// second k row 2 * 144 mod 64 = 32 banks on.
#define RBF_LDA (RBF_BK + 2)
#define RBF_LDB (RBF_BN + 16)
#define RBF_HDR 8     // doubles in front of the factor: [0] = a

typedef double rbf_d4 __attribute__((ext_vector_type(4)));

static inline int rbf_np(int N) { return (N + RBF_NB - 1) / RBF_NB * RBF_NB; }
static inline int64_t rbf_ldx(int S) { return ((int64_t)S + 1 + 15) / 16 * 16; }

// One staged slab through v_mfma_f64_16x16x4_f64.  Wave (wm, wn) of the 2 x 2 owns 32
// rows x 64 columns: 2 x 4 tiles.  Operands: lane l holds A[l & 15][l >> 4] and
// B[l >> 4][l & 15]; result register q of lane l is row (l >> 4) + 4 q, column l & 15.
__device__ __forceinline__ void rbf_mma_slab(const double *As, const double *Bs,
                                             rbf_d4 (&acc)[2][4], int wm, int wn,
                                             int lane) {
  const int r = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int k0 = 0; k0 < RBF_BK; k0 += 4) {
    double a[2], b[4];
#pragma unroll
    for (int i = 0; i < 2; i++) a[i] = As[(wm * 32 + i * 16 + r) * RBF_LDA + k0 + kq];
#pragma unroll
    for (int j = 0; j < 4; j++) b[j] = Bs[(k0 + kq) * RBF_LDB + wn * 64 + j * 16 + r];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int j = 0; j < 4; j++)
        acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
  }
}

// ---------------------------------------------------------------------------
// Assembly
// ---------------------------------------------------------------------------
// a, and the finite check of the nodes and the smoothing; one block
__global__ void __launch_bounds__(256)
rbf_bbox_kernel(const double *__restrict__ y, int N, int ndim, double eps,
                const double *__restrict__ smoothing, double *__restrict__ hdr,
                int32_t *__restrict__ status) {
  __shared__ double red[4];
  __shared__ int s_bad;
  const int tid = threadIdx.x;
  if (tid == 0) s_bad = 0;
  __syncthreads();
  int bad = 0;
  double diag2 = 0;
  for (int d = 0; d < ndim; d++) {
    double lo = 1e300, hi = -1e300;
    for (int i = tid; i < N; i += 256) {
      const double v = y[(int64_t)i * ndim + d] * eps;
      bad |= !isfinite(v);
      lo = fmin(lo, v);
      hi = fmax(hi, v);
    }
    hi = wave_max(hi);
    lo = -wave_max(-lo);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = hi;
    __syncthreads();
    hi = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = lo;
    __syncthreads();
    lo = fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
    diag2 += (hi - lo) * (hi - lo);
  }
  if (smoothing)
    for (int i = tid; i < N; i += 256) bad |= !isfinite(smoothing[i]);
  if (bad) s_bad = 1;
  __syncthreads();
  if (tid == 0) {
    hdr[0] = sqrt(diag2 + 1.0);
    if (s_bad) atomicOr(status, RVS_ST_NONFINITE);
  }
}

// the full symmetric A (the factorisation reads its lower triangle), identity padding
__global__ void __launch_bounds__(256)
rbf_assemble_kernel(const double *__restrict__ y, int N, int Np, int ndim, double eps,
                    const double *__restrict__ smoothing, const double *__restrict__ hdr,
                    double *__restrict__ A) {
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  const int i = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (i >= Np || j >= Np) return;
  double v = i == j ? 1.0 : 0.0;
  if (i < N && j < N) {
    double r2 = 0;
    for (int d = 0; d < ndim; d++) {
      const double t = y[(int64_t)i * ndim + d] * eps - y[(int64_t)j * ndim + d] * eps;
      r2 = fma(t, t, r2);
    }
    v = hdr[0] - sqrt(r2 + 1.0);
    if (i == j && smoothing) v += smoothing[i];
  }
  A[(int64_t)i * Np + j] = v;
}

// ---------------------------------------------------------------------------
// Diagonal block: Cholesky of the lower triangle of one RBF_NB x RBF_NB block in LDS
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
rbf_potrf_kernel(double *__restrict__ A, int64_t lda, const double *__restrict__ hdr,
                 int N, int32_t *__restrict__ status) {
  __shared__ double T[RBF_NB * (RBF_NB + 1)];
  const int tid = threadIdx.x;
  for (int e = tid; e < RBF_NB * RBF_NB; e += 256) {
    const int i = e >> 6, c = e & 63;
    T[i * (RBF_NB + 1) + c] = c <= i ? A[i * lda + c] : 0.0;
  }
  // a pivot that the rounding of N products of size a cannot tell from zero
  const double tiny = 8.0 * N * 2.220446049250313e-16 * hdr[0];
  int bad = 0;
  for (int j = 0; j < RBF_NB; j++) {
    __syncthreads();
    double p = T[j * (RBF_NB + 1) + j];
    if (!(p > tiny) || !isfinite(p)) {
      bad = 1;
      p = 1.0;
    }
    const double dj = sqrt(p);
    __syncthreads();
    if (tid >= j && tid < RBF_NB)
      T[tid * (RBF_NB + 1) + j] = tid == j ? dj : T[tid * (RBF_NB + 1) + j] / dj;
    __syncthreads();
    for (int e = tid; e < RBF_NB * RBF_NB; e += 256) {
      const int i = e >> 6, c = e & 63;
      if (c > j && c <= i)
        T[i * (RBF_NB + 1) + c] =
            fma(-T[i * (RBF_NB + 1) + j], T[c * (RBF_NB + 1) + j], T[i * (RBF_NB + 1) + c]);
    }
  }
  __syncthreads();
  for (int e = tid; e < RBF_NB * RBF_NB; e += 256) {
    const int i = e >> 6, c = e & 63;
    if (c <= i) A[i * lda + c] = T[i * (RBF_NB + 1) + c];
  }
  if (tid == 0 && bad) atomicOr(status, RVS_ST_RBF_NOTPD);
}

// ---------------------------------------------------------------------------
// Triangular solve with one diagonal block L (lower, RBF_NB x RBF_NB): thread t solves
// L x = b (BACK: L^T x = b) for the vector b[r] = Bm[r sr + t st] in place, by
// substitution with x in registers.  st = 1: the columns of a block row of right-hand
// sides; sr = 1: the rows of a panel (x L^T = b is L x^T = b^T).
// ---------------------------------------------------------------------------
template <bool BACK>
__global__ void __launch_bounds__(128)
rbf_trsm_kernel(const double *__restrict__ Ld, int64_t ldl, double *__restrict__ Bm,
                int64_t sr, int64_t st, int64_t nt) {
  __shared__ double Ls[RBF_NB * RBF_NB];
  for (int e = threadIdx.x; e < RBF_NB * RBF_NB; e += 128)
    Ls[e] = Ld[(e >> 6) * ldl + (e & 63)];
  __syncthreads();
  const int64_t t = (int64_t)blockIdx.x * 128 + threadIdx.x;
  if (t >= nt) return;
  double *b = Bm + t * st;
  double x[RBF_NB];
#pragma unroll
  for (int r = 0; r < RBF_NB; r++) x[r] = b[r * sr];
  if (!BACK) {
#pragma unroll
    for (int r = 0; r < RBF_NB; r++) {
      double s = x[r];
#pragma unroll
      for (int p = 0; p < r; p++) s = fma(-Ls[r * RBF_NB + p], x[p], s);
      x[r] = s / Ls[r * RBF_NB + r];
    }
  } else {
#pragma unroll
    for (int r = RBF_NB - 1; r >= 0; r--) {
      double s = x[r];
#pragma unroll
      for (int p = RBF_NB - 1; p > r; p--) s = fma(-Ls[p * RBF_NB + r], x[p], s);
      x[r] = s / Ls[r * RBF_NB + r];
    }
  }
#pragma unroll
  for (int r = 0; r < RBF_NB; r++) b[r * sr] = x[r];
}

// ---------------------------------------------------------------------------
// Update: C [m, n] -= A [m, k] B [k, n]; m a multiple of RBF_BM, k of RBF_BK, n any.
// A(i, p) = A[i lda + p], TA: A[p lda + i]; B(p, j) = B[p ldb + j], TB: B[j ldb + p].
// lower: tiles wholly above the diagonal are left alone.  Serves the trailing update of
// the factorisation (TB, lower) and the blocked forward (plain) and backward (TA)
// substitutions of the right-hand sides.
// ---------------------------------------------------------------------------
template <bool TA, bool TB>
__global__ void __launch_bounds__(256)
rbf_update_kernel(const double *__restrict__ A, int64_t lda, const double *__restrict__ B,
                  int64_t ldb, double *__restrict__ C, int64_t ldc, int m, int n, int k,
                  int lower) {
  __shared__ double As[RBF_BM * RBF_LDA];
  __shared__ double Bs[RBF_BK * RBF_LDB];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  const int m0 = blockIdx.y * RBF_BM, n0 = blockIdx.x * RBF_BN;
  if (lower && n0 > m0 + RBF_BM - 1) return;
  rbf_d4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (rbf_d4){0, 0, 0, 0};
  for (int k0 = 0; k0 < k; k0 += RBF_BK) {
    double ra[8], rb[16];
    if (!TA) {      // lanes along k
      const int kk = tid & 31, mm = tid >> 5;
#pragma unroll
      for (int q = 0; q < 8; q++) ra[q] = A[(int64_t)(m0 + mm + 8 * q) * lda + k0 + kk];
    } else {        // lanes along m
      const int mm = tid & 63, kk = tid >> 6;
#pragma unroll
      for (int q = 0; q < 8; q++) ra[q] = A[(int64_t)(k0 + kk + 4 * q) * lda + m0 + mm];
    }
    if (!TB) {      // lanes along n
      const int nn = tid & 127, kk = tid >> 7;
#pragma unroll
      for (int q = 0; q < 16; q++)
        rb[q] = n0 + nn < n ? B[(int64_t)(k0 + kk + 2 * q) * ldb + n0 + nn] : 0.0;
    } else {        // lanes along k
      const int kk = tid & 31, nn = tid >> 5;
#pragma unroll
      for (int q = 0; q < 16; q++)
        rb[q] = n0 + nn + 8 * q < n ? B[(int64_t)(n0 + nn + 8 * q) * ldb + k0 + kk] : 0.0;
    }
    __syncthreads();
    if (!TA) {
      const int kk = tid & 31, mm = tid >> 5;
#pragma unroll
      for (int q = 0; q < 8; q++) As[(mm + 8 * q) * RBF_LDA + kk] = ra[q];
    } else {
      const int mm = tid & 63, kk = tid >> 6;
#pragma unroll
      for (int q = 0; q < 8; q++) As[mm * RBF_LDA + kk + 4 * q] = ra[q];
    }
    if (!TB) {
      const int nn = tid & 127, kk = tid >> 7;
#pragma unroll
      for (int q = 0; q < 16; q++) Bs[(kk + 2 * q) * RBF_LDB + nn] = rb[q];
    } else {
      const int kk = tid & 31, nn = tid >> 5;
#pragma unroll
      for (int q = 0; q < 16; q++) Bs[kk * RBF_LDB + nn + 8 * q] = rb[q];
    }
    __syncthreads();
    rbf_mma_slab(As, Bs, acc, wm, wn, lane);
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int col = n0 + wn * 64 + j * 16 + (lane & 15);
      if (col >= n) continue;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int row = m0 + wm * 32 + i * 16 + (lane >> 4) + 4 * q;
        double *c = C + (int64_t)row * ldc + col;
        *c = *c - acc[i][j][q];
      }
    }
}

template <bool TA, bool TB>
static void rbf_update(const double *A, int64_t lda, const double *B, int64_t ldb,
                       double *C, int64_t ldc, int m, int64_t n, int k, int lower,
                       hipStream_t st) {
  const dim3 grid((unsigned)((n + RBF_BN - 1) / RBF_BN), m / RBF_BM);
  hipLaunchKernelGGL((rbf_update_kernel<TA, TB>), grid, dim3(256), 0, st, A, lda, B, ldb,
                     C, ldc, m, (int)n, k, lower);
}

// ---------------------------------------------------------------------------
// Right-hand sides
// ---------------------------------------------------------------------------
// X [Np, ldx] = [d | 1 | 0], rows behind N zero; RVS_ST_NONFINITE for a value of d
template <typename DT>
__global__ void __launch_bounds__(256)
rbf_rhs_kernel(const DT *__restrict__ d, int64_t d_stride, int N, int S, int64_t ldx,
               double *__restrict__ X, int32_t *__restrict__ status) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int i = blockIdx.y;
  if (s >= ldx) return;
  double v = 0;
  if (i < N) {
    if (s < S) {
      v = (double)d[(int64_t)i * d_stride + s];
      if (!isfinite(v)) atomicOr(status, RVS_ST_NONFINITE);
    } else if (s == S) {
      v = 1.0;
    }
  }
  X[(int64_t)i * ldx + s] = v;
}

// lam = 1^T U / 1^T w and c = U - w lam, one thread per column, sums in row order
__global__ void __launch_bounds__(256)
rbf_finish_kernel(double *__restrict__ X, int64_t ldx, int N, int S,
                  double *__restrict__ lam) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= S) return;
  double su = 0, sw = 0;
  for (int i = 0; i < N; i++) {
    su += X[(int64_t)i * ldx + s];
    sw += X[(int64_t)i * ldx + S];
  }
  const double l = su / sw;
  for (int i = 0; i < N; i++)
    X[(int64_t)i * ldx + s] = fma(-X[(int64_t)i * ldx + S], l, X[(int64_t)i * ldx + s]);
  lam[s] = l;
}

// ---------------------------------------------------------------------------
// Fused evaluation: a block takes RBF_BM points x RBF_BN columns and walks the nodes in
// slabs of RBF_BK.  The kernel values of the slab are made from the coordinates (thread:
// one node, 8 of the 64 points) straight into the A operand's LDS image; the M x N
// kernel matrix never exists in memory.
// ---------------------------------------------------------------------------
template <typename OT>
__global__ void __launch_bounds__(256)
rbf_eval_kernel(const double *__restrict__ x, int M, const double *__restrict__ y, int N,
                int Np, int ndim, double eps, const double *__restrict__ c, int64_t ldc,
                const double *__restrict__ lam, int S, OT *__restrict__ out,
                int64_t ldo) {
  __shared__ double As[RBF_BM * RBF_LDA];
  __shared__ double Bs[RBF_BK * RBF_LDB];
  __shared__ double xs[RBF_BM * 8];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  const int m0 = blockIdx.y * RBF_BM, n0 = blockIdx.x * RBF_BN;
  for (int e = tid; e < RBF_BM * 8; e += 256) {
    const int mm = e >> 3, d = e & 7;
    xs[e] = (m0 + mm < M && d < ndim) ? x[(int64_t)(m0 + mm) * ndim + d] * eps : 0.0;
  }
  rbf_d4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (rbf_d4){0, 0, 0, 0};
  const int jj = tid & 31, mq = tid >> 5;
  const int nn = tid & 127, kb = tid >> 7;
  for (int j0 = 0; j0 < Np; j0 += RBF_BK) {
    double rb[16], yj[8], ra[8];
#pragma unroll
    for (int q = 0; q < 16; q++)
      rb[q] = n0 + nn < S ? c[(int64_t)(j0 + kb + 2 * q) * ldc + n0 + nn] : 0.0;
    const int j = j0 + jj;
#pragma unroll
    for (int d = 0; d < 8; d++)
      yj[d] = (j < N && d < ndim) ? y[(int64_t)j * ndim + d] * eps : 0.0;
    __syncthreads();      // xs filled (first slab); the previous slab's reads are done
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const double *xm = xs + (mq + 8 * q) * 8;
      double r2 = 0;
#pragma unroll
      for (int d = 0; d < 8; d++) {
        const double t = xm[d] - yj[d];
        r2 = fma(t, t, r2);
      }
      ra[q] = j < N ? -sqrt(r2 + 1.0) : 0.0;
    }
#pragma unroll
    for (int q = 0; q < 8; q++) As[(mq + 8 * q) * RBF_LDA + jj] = ra[q];
#pragma unroll
    for (int q = 0; q < 16; q++) Bs[(kb + 2 * q) * RBF_LDB + nn] = rb[q];
    __syncthreads();
    rbf_mma_slab(As, Bs, acc, wm, wn, lane);
  }
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int col = n0 + wn * 64 + j * 16 + (lane & 15);
      if (col >= S) continue;
      const double l = lam[col];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int row = m0 + wm * 32 + i * 16 + (lane >> 4) + 4 * q;
        if (row < M) out[(int64_t)row * ldo + col] = (OT)(acc[i][j][q] + l);
      }
    }
}

// ---------------------------------------------------------------------------
// Entry points
// ---------------------------------------------------------------------------
static inline bool rbf_shape_ok(int N, int S) {
  return N >= 1 && N <= RVS_RBF_MAX_N && S >= 1 && S <= RVS_RBF_MAX_S;
}

extern "C" int64_t rvs_rbf_work_size(int N, int S) {
  if (!rbf_shape_ok(N, S)) return RVS_E_ARG;
  const int64_t np = rbf_np(N), ldx = rbf_ldx(S);
  return RBF_HDR + np * np + np * ldx + ldx;
}

extern "C" int rvs_rbf_factor(const double *y, int N, int ndim, double eps,
                              const double *smoothing, double *work, int32_t *status,
                              void *stream) {
  if (!y || !work || !status) return RVS_E_ARG;
  if (!rbf_shape_ok(N, 1) || ndim < 1 || ndim > 8 || !(eps > 0) || !(eps < 1e300))
    return RVS_E_ARG;
  const int np = rbf_np(N), nb = np / RBF_NB;
  double *L = work + RBF_HDR;
  hipStream_t st = rvs_stream(stream);
  hipLaunchKernelGGL(rbf_bbox_kernel, dim3(1), dim3(256), 0, st, y, N, ndim, eps,
                     smoothing, work, status);
  hipLaunchKernelGGL(rbf_assemble_kernel, dim3(np / 64, np / 4), dim3(256), 0, st, y, N,
                     np, ndim, eps, smoothing, work, L);
  RVS_LAUNCH_CHECK();
  for (int j = 0; j < nb; j++) {
    double *Ljj = L + (int64_t)j * RBF_NB * np + j * RBF_NB;
    hipLaunchKernelGGL(rbf_potrf_kernel, dim3(1), dim3(256), 0, st, Ljj, (int64_t)np,
                       work, N, status);
    const int rem = np - (j + 1) * RBF_NB;
    if (rem > 0) {
      double *L21 = Ljj + (int64_t)RBF_NB * np;
      hipLaunchKernelGGL(rbf_trsm_kernel<false>, dim3((rem + 127) / 128), dim3(128), 0,
                         st, Ljj, (int64_t)np, L21, (int64_t)1, (int64_t)np,
                         (int64_t)rem);
      rbf_update<false, true>(L21, np, L21, np, L21 + RBF_NB, np, rem, rem, RBF_NB, 1,
                              st);
    }
    RVS_LAUNCH_CHECK();
  }
  return 0;
}

extern "C" int rvs_rbf_solve(const void *d, int d_f32, int64_t d_stride, int N, int S,
                             double *work, int32_t *status, void *stream) {
  if (!d || !work || !status) return RVS_E_ARG;
  if (!rbf_shape_ok(N, S) || d_stride < S) return RVS_E_ARG;
  const int np = rbf_np(N), nb = np / RBF_NB;
  const int64_t ldx = rbf_ldx(S), s1 = (int64_t)S + 1;
  double *L = work + RBF_HDR, *X = L + (int64_t)np * np, *lam = X + np * ldx;
  hipStream_t st = rvs_stream(stream);
  const dim3 rg((unsigned)((ldx + 255) / 256), np);
  if (d_f32)
    hipLaunchKernelGGL(rbf_rhs_kernel<float>, rg, dim3(256), 0, st, (const float *)d,
                       d_stride, N, S, ldx, X, status);
  else
    hipLaunchKernelGGL(rbf_rhs_kernel<double>, rg, dim3(256), 0, st, (const double *)d,
                       d_stride, N, S, ldx, X, status);
  RVS_LAUNCH_CHECK();
  const dim3 tg((unsigned)((s1 + 127) / 128));
  for (int i = 0; i < nb; i++) {          // L Y = [d | 1]
    const double *Li = L + (int64_t)i * RBF_NB * np;
    double *Xi = X + (int64_t)i * RBF_NB * ldx;
    if (i > 0)
      rbf_update<false, false>(Li, np, X, ldx, Xi, ldx, RBF_NB, s1, i * RBF_NB, 0, st);
    hipLaunchKernelGGL(rbf_trsm_kernel<false>, tg, dim3(128), 0, st, Li + i * RBF_NB,
                       (int64_t)np, Xi, ldx, (int64_t)1, s1);
    RVS_LAUNCH_CHECK();
  }
  for (int i = nb - 1; i >= 0; i--) {     // L^T [U | w] = Y
    const double *Lb = L + (int64_t)(i + 1) * RBF_NB * np + i * RBF_NB;
    double *Xi = X + (int64_t)i * RBF_NB * ldx;
    if (i < nb - 1)
      rbf_update<true, false>(Lb, np, Xi + RBF_NB * ldx, ldx, Xi, ldx, RBF_NB, s1,
                              np - (i + 1) * RBF_NB, 0, st);
    hipLaunchKernelGGL(rbf_trsm_kernel<true>, tg, dim3(128), 0, st,
                       L + (int64_t)i * RBF_NB * np + i * RBF_NB, (int64_t)np, Xi, ldx,
                       (int64_t)1, s1);
    RVS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rbf_finish_kernel, dim3((S + 255) / 256), dim3(256), 0, st, X, ldx,
                     N, S, lam);
  RVS_LAUNCH_CHECK();
  return 0;
}

extern "C" int rvs_rbf_eval(const double *x, int M, const double *y, int N, int ndim,
                            double eps, const double *work, int S, int float_bits,
                            void *out, int64_t out_stride, void *stream) {
  if (!x || !y || !work || !out) return RVS_E_ARG;
  if (!rbf_shape_ok(N, S) || ndim < 1 || ndim > 8 || !(eps > 0) || !(eps < 1e300))
    return RVS_E_ARG;
  if (M < 1 || M > RVS_RBF_MAX_M || out_stride < S) return RVS_E_ARG;
  if (float_bits != 32 && float_bits != 64) return RVS_E_ARG;
  const int np = rbf_np(N);
  const int64_t ldx = rbf_ldx(S);
  const double *X = work + RBF_HDR + (int64_t)np * np, *lam = X + np * ldx;
  const dim3 grid((S + RBF_BN - 1) / RBF_BN, (M + RBF_BM - 1) / RBF_BM);
  if (float_bits == 32)
    hipLaunchKernelGGL(rbf_eval_kernel<float>, grid, dim3(256), 0, rvs_stream(stream), x,
                       M, y, N, np, ndim, eps, X, ldx, lam, S, (float *)out, out_stride);
  else
    hipLaunchKernelGGL(rbf_eval_kernel<double>, grid, dim3(256), 0, rvs_stream(stream),
                       x, M, y, N, np, ndim, eps, X, ldx, lam, S, (double *)out,
                       out_stride);
  RVS_LAUNCH_CHECK();
  return 0;
}
