// nn_train.hip -- trainer of the MLP template interpolator (the network nn.hip
// evaluates): forward, L1 loss, backward and Adam of one optimiser step as plain
// stream launches, a whole epoch per host call.
//
// Reference: py/rvspecfit/nn/train_interpolator.py:284-322 (the step: model(x) *
// SD_0 + D_0, l1_loss / spread0, backward, Adam) on py/rvspecfit/nn/
// NNInterpolator.py:14-91 with withbn = False and SiLU: Linear + SiLU for every
// layer but the last (pc_layer), which is Linear alone.
//
// Everything is float32 on v_mfma_f32_32x32x2_f32 (exact f32 products, one f32 fma
// chain per output in ascending k: a run is reproducible bit for bit).  No float
// atomics: the one product that is split along K (dA of the output layer) writes
// its partial tiles to scratch and a second kernel adds them in split order; the
// loss is folded from per-block float64 partials in block order.
//
// One step with L linear layers is 3 L + 1 launches (16 for the reference's default
// of five layers):
//   L - 1  nt_fwd_kernel        z_l = a_{l-1} W_l^T + b_l, a_l = silu(z_l), both kept
//   1      nt_loss_kernel       output layer fused with the loss: R is never stored,
//                               g = sign(R - dat) SD_0 / (rows npix spread0) is
//   1      nt_dw_kernel         dW_pc = g^T a, db_pc = column sums of g (same launch)
//   1      nt_da_split_kernel   partial tiles of g W_pc over chunks of 128 pixels
//   1      nt_da_fold_kernel    their sum in chunk order, times silu'(z); block 0
//                               folds the loss partials into the epoch's float64 sum
//   2(L-1)-1  nt_dw_kernel / nt_da_kernel of the hidden layers (dA carries the SiLU
//                               derivative of the layer below in its epilogue)
//   1      nt_adam_kernel       every parameter tensor in one launch
// ORDER OF dA AND THE UPDATE: dA_l = g_l W_l needs W_l as the forward pass used it.
// The update is the LAST launch of a step and the only one that writes a weight, so
// stream order alone puts every read of W_l before its update (nt_step, nt_adam).
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define NT_BM 64
#define NT_BN 64
#define NT_BK 32
#define NT_LD 65           // LDS row of one k: 64 outer elements + 1 (stores 2-way at most)
#define NT_NP (NT_BM * NT_BK / 256)   // elements per thread, operand and slab
#define NT_SPLIT_K 128     // pixels per chunk of the split dA product
#define NT_MAXL 8          // linear layers at most

// One operand of a product C[o_a, o_b] = sum_k A(o_a, k) B(o_b, k): element (o, k) is
// p[io(o) * so + ik(k) * sk]; io / ik (nullable) gather the rows of a batch by index,
// clamped to [0, nidx).
struct NtOp {
  const float *p;
  int64_t so, sk;
  const int32_t *io, *ik;
  int nidx;
};

__device__ __forceinline__ void nt_coord(const NtOp &op, int p, int &o, int &k) {
  const int t = threadIdx.x;
  if (op.sk == 1) {   // rows contiguous along k: 128-byte runs per row
    k = t & 31;
    o = (t >> 5) + 8 * p;
  } else {            // contiguous along the outer index: 256-byte runs per k
    o = t & 63;
    k = (t >> 6) + 4 * p;
  }
}

__device__ __forceinline__ void nt_fetch(const NtOp &op, int O, int o0, int ks, int kend,
                                         float (&r)[NT_NP]) {
#pragma unroll
  for (int p = 0; p < NT_NP; p++) {
    int o, k;
    nt_coord(op, p, o, k);
    const int go = o0 + o, gk = ks + k;
    float v = 0.f;
    if (go < O && gk < kend) {
      const int64_t ro = op.io ? min(max(op.io[go], 0), op.nidx - 1) : go;
      const int64_t rk = op.ik ? min(max(op.ik[gk], 0), op.nidx - 1) : gk;
      v = op.p[ro * op.so + rk * op.sk];
    }
    r[p] = v;
  }
}

__device__ __forceinline__ void nt_stash(const NtOp &op, float *s, const float (&r)[NT_NP]) {
#pragma unroll
  for (int p = 0; p < NT_NP; p++) {
    int o, k;
    nt_coord(op, p, o, k);
    s[k * NT_LD + o] = r[p];
  }
}

// The 64 x 64 tile at (m0, n0) of sum_{k0 <= k < k1} A(m, k) B(n, k): four waves of one
// 32 x 32 MFMA tile each, K in slabs of 32 through LDS ([k][outer]: lane (outer, k =
// lane / 32) of the MFMA reads consecutive words), the next slab's loads in flight
// under the current slab's products.  epi(row, col, value) for the elements inside
// M x N; slab(As) is called once per staged slab (all threads, between barriers).
template <class Epi, class Slab>
__device__ __forceinline__ void nt_tile(const NtOp &A, const NtOp &B, int M, int N, int k0,
                                        int k1, int m0, int n0, float *lds, Epi &&epi,
                                        Slab &&slab) {
  float *As = lds, *Bs = lds + NT_BK * NT_LD;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  f32x16 acc;
#pragma unroll
  for (int q = 0; q < 16; q++) acc[q] = 0.f;
  float ra[NT_NP], rb[NT_NP];
  nt_fetch(A, M, m0, k0, k1, ra);
  nt_fetch(B, N, n0, k0, k1, rb);
  for (int ks = k0; ks < k1; ks += NT_BK) {
    __syncthreads();   // the previous slab has been read
    nt_stash(A, As, ra);
    nt_stash(B, Bs, rb);
    __syncthreads();
    if (ks + NT_BK < k1) {
      nt_fetch(A, M, m0, ks + NT_BK, k1, ra);
      nt_fetch(B, N, n0, ks + NT_BK, k1, rb);
    }
    slab(As);
    const float *ap = As + (lane >> 5) * NT_LD + wm * 32 + (lane & 31);
    const float *bp = Bs + (lane >> 5) * NT_LD + wn * 32 + (lane & 31);
#pragma unroll
    for (int kk = 0; kk < NT_BK; kk += 2)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[kk * NT_LD], bp[kk * NT_LD], acc, 0, 0,
                                                 0);
  }
  const int col = n0 + wn * 32 + (lane & 31);
#pragma unroll
  for (int r = 0; r < 16; r++) {
    const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (row < M && col < N) epi(row, col, acc[r]);
  }
}

__device__ __forceinline__ float nt_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }
// d silu(z) / dz = s (1 + z (1 - s)), s = sigmoid(z)
__device__ __forceinline__ float nt_dsilu(float z) {
  const float s = nt_sigmoid(z);
  return s * (1.0f + z * (1.0f - s));
}

#define NT_TILE_OF_BLOCK(Mv)                          \
  const int ntm_ = ((Mv) + NT_BM - 1) / NT_BM;        \
  const int m0 = ((int)blockIdx.x % ntm_) * NT_BM;    \
  const int n0 = ((int)blockIdx.x / ntm_) * NT_BN;    \
  __shared__ float lds[2 * NT_BK * NT_LD]

// z = X W^T + b, a = silu(z); X [rows, K] (or the rows `idx` of it), W [N, K]
__global__ void __launch_bounds__(256)
    nt_fwd_kernel(const float *__restrict__ X, const int32_t *__restrict__ idx, int nidx,
                  const float *__restrict__ W, const float *__restrict__ bias, int rows,
                  int K, int N, float *__restrict__ z, float *__restrict__ a) {
  NT_TILE_OF_BLOCK(rows);
  const NtOp A = {X, K, 1, idx, nullptr, nidx}, B = {W, K, 1, nullptr, nullptr, 0};
  nt_tile(A, B, rows, N, 0, K, m0, n0, lds,
          [&](int row, int col, float v) {
            const float y = v + bias[col];
            z[(int64_t)row * N + col] = y;
            a[(int64_t)row * N + col] = y * nt_sigmoid(y);
          },
          [](const float *) {});
}

// Output layer and loss (train_interpolator.py:292-293): R = (a W^T + b) SD_0 + D_0,
// r = R - dat[idx[row]], losspart[block] = sum |r| (float64), and when g != NULL
// g = sign(r) SD_0 gscale with sign(0) = 0 as torch.sign; resid (nullable) = r.
__global__ void __launch_bounds__(256)
    nt_loss_kernel(const float *__restrict__ X, const float *__restrict__ W,
                   const float *__restrict__ bias, const float *__restrict__ D0,
                   const float *__restrict__ SD0, const float *__restrict__ dats,
                   const int32_t *__restrict__ idx, int nidx, int rows, int K, int N,
                   float gscale, float *__restrict__ g, float *__restrict__ resid,
                   double *__restrict__ losspart) {
  NT_TILE_OF_BLOCK(rows);
  __shared__ double red[4];
  const NtOp A = {X, K, 1, nullptr, nullptr, 0}, B = {W, K, 1, nullptr, nullptr, 0};
  double part = 0.0;
  nt_tile(A, B, rows, N, 0, K, m0, n0, lds,
          [&](int row, int col, float v) {
            const float sd = SD0[col];
            const float R = fmaf(v + bias[col], sd, D0[col]);
            const int64_t dr = min(max(idx[row], 0), nidx - 1);
            const float r = R - dats[dr * N + col];
            part += (double)fabsf(r);
            if (g)
              g[(int64_t)row * N + col] =
                  (r > 0.f ? sd : (r < 0.f ? -sd : 0.f)) * gscale;
            if (resid) resid[(int64_t)row * N + col] = r;
          },
          [](const float *) {});
  part = block_sum<4>(part, red);
  if (threadIdx.x == 0) losspart[blockIdx.x] = part;
}

// dW = G^T Aprev: dW [N, K] from G [rows, N] and Aprev [rows, K] (or the rows `idx` of
// it); db[n] = sum_rows G[., n] by the blocks of the first column tile, from the
// staged slabs (ascending row order).
__global__ void __launch_bounds__(256)
    nt_dw_kernel(const float *__restrict__ G, const float *__restrict__ Aprev,
                 const int32_t *__restrict__ idx, int nidx, int rows, int N, int K,
                 float *__restrict__ dW, float *__restrict__ db) {
  NT_TILE_OF_BLOCK(N);
  const NtOp A = {G, 1, N, nullptr, nullptr, 0}, B = {Aprev, 1, K, nullptr, idx, nidx};
  float bsum = 0.f;
  const bool do_b = n0 == 0 && threadIdx.x < NT_BM;
  nt_tile(A, B, N, K, 0, rows, m0, n0, lds,
          [&](int row, int col, float v) { dW[(int64_t)row * K + col] = v; },
          [&](const float *As) {
            if (do_b)
              for (int k = 0; k < NT_BK; k++) bsum += As[k * NT_LD + threadIdx.x];
          });
  if (do_b && m0 + (int)threadIdx.x < N) db[m0 + threadIdx.x] = bsum;
}

// dA = (G W) silu'(z): G [rows, N], W [N, K], z and the result [rows, K]
__global__ void __launch_bounds__(256)
    nt_da_kernel(const float *__restrict__ G, const float *__restrict__ W,
                 const float *__restrict__ z, int rows, int N, int K,
                 float *__restrict__ gprev) {
  NT_TILE_OF_BLOCK(rows);
  const NtOp A = {G, N, 1, nullptr, nullptr, 0}, B = {W, 1, K, nullptr, nullptr, 0};
  nt_tile(A, B, rows, K, 0, N, m0, n0, lds,
          [&](int row, int col, float v) {
            const int64_t e = (int64_t)row * K + col;
            gprev[e] = v * nt_dsilu(z[e]);
          },
          [](const float *) {});
}

// The same product over the pixels [split NT_SPLIT_K, +NT_SPLIT_K) only (blockIdx.y =
// split), unscaled, to part [nsplit, rows, K]
__global__ void __launch_bounds__(256)
    nt_da_split_kernel(const float *__restrict__ G, const float *__restrict__ W, int rows,
                       int N, int K, float *__restrict__ part) {
  NT_TILE_OF_BLOCK(rows);
  const NtOp A = {G, N, 1, nullptr, nullptr, 0}, B = {W, 1, K, nullptr, nullptr, 0};
  const int k0 = blockIdx.y * NT_SPLIT_K;
  float *out = part + (int64_t)blockIdx.y * rows * K;
  nt_tile(A, B, rows, K, k0, min(k0 + NT_SPLIT_K, N), m0, n0, lds,
          [&](int row, int col, float v) { out[(int64_t)row * K + col] = v; },
          [](const float *) {});
}

// sum of the loss partials in block order: accum += S / spread0 (lossAccum,
// train_interpolator.py:322), step = S / (count spread0) (the step's loss); one wave
__device__ __forceinline__ void nt_loss_fold(const double *__restrict__ losspart, int npart,
                                             double spread0, double count,
                                             double *__restrict__ accum,
                                             double *__restrict__ step) {
  if (threadIdx.x >= 64) return;
  double s = 0.0;
  for (int i = threadIdx.x; i < npart; i += 64) s += losspart[i];
  s = wave_sum(s);
  if (threadIdx.x == 0) {
    if (accum) accum[0] += s / spread0;
    if (step) step[0] = s / (count * spread0);
  }
}

__global__ void __launch_bounds__(256)
    nt_da_fold_kernel(const float *__restrict__ part, int nsplit, int64_t n,
                      const float *__restrict__ z, float *__restrict__ gprev,
                      const double *__restrict__ losspart, int npart, double spread0,
                      double count, double *__restrict__ accum, double *__restrict__ step) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) {
    float s = 0.f;
    for (int q = 0; q < nsplit; q++) s += part[q * n + e];   // fixed order
    gprev[e] = s * nt_dsilu(z[e]);
  }
  if (blockIdx.x == 0) nt_loss_fold(losspart, npart, spread0, count, accum, step);
}

__global__ void __launch_bounds__(64)
    nt_loss_fold_kernel(const double *__restrict__ losspart, int npart, double spread0,
                        double count, double *__restrict__ accum,
                        double *__restrict__ step) {
  nt_loss_fold(losspart, npart, spread0, count, accum, step);
}

// torch.optim.Adam (defaults: betas 0.9 / 0.999, eps 1e-8, no weight decay, no
// amsgrad) as torch/optim/adam.py:_single_tensor_adam states it, operation for
// operation in float32 with the Python scalars rounded to float32 where torch hands
// them to a float32 tensor operation:
//   m.lerp_(g, 1 - b1); v.mul_(b2).addcmul_(g, g, value = 1 - b2);
//   denom = (v.sqrt() / sqrt(1 - b2^t)).add_(eps); p.addcdiv_(m, denom, value = -lr / (1 - b1^t))
// lerp_ and addcmul_ are one fused multiply-add each in torch's CPU kernels (the
// moments of tests/golden/nn_train_cases.npz are reproduced bit for bit this way and
// not with separate roundings); addcdiv_ is (value m) / denom, then the sum.
struct NtAdam {
  float *p[2 * NT_MAXL], *m[2 * NT_MAXL], *v[2 * NT_MAXL];
  const float *g[2 * NT_MAXL];
  int64_t end[2 * NT_MAXL];   // running element count behind tensor i
  int n;
};
__global__ void __launch_bounds__(256)
    nt_adam_kernel(NtAdam T, float neg_step_size, float bc2_sqrt) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= T.end[T.n - 1]) return;
  int i = 0;
  while (e >= T.end[i]) i++;
  const int64_t j = e - (i ? T.end[i - 1] : 0);
  const float g = T.g[i][j];
  float m = T.m[i][j], v = T.v[i][j];
  m = __fmaf_rn(0.1f, __fsub_rn(g, m), m);
  v = __fmaf_rn(__fmul_rn(0.001f, g), g, __fmul_rn(v, 0.999f));
  // (sqrtf and / are correctly rounded in hipcc's default mode; the __fsqrt_rn
  // intrinsic is the approximate v_sqrt_f32 unless OCML_BASIC_ROUNDED_OPERATIONS is set)
  const float denom = __fadd_rn(__fdiv_rn(sqrtf(v), bc2_sqrt), 1e-8f);
  T.m[i][j] = m;
  T.v[i][j] = v;
  T.p[i][j] = __fadd_rn(T.p[i][j], __fdiv_rn(__fmul_rn(neg_step_size, m), denom));
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static bool nt_args_ok(int T, int B, int nlayer, const int32_t *dims) {
  if (T < 1 || B < 1 || B > RVS_NN_TRAIN_MAX_B || nlayer < 2 || nlayer > NT_MAXL || !dims)
    return false;
  if (dims[0] < 1 || dims[0] > 8) return false;
  for (int l = 1; l < nlayer; l++)
    if (dims[l] < 1 || dims[l] > RVS_NN_TRAIN_MAX_WIDTH) return false;
  return dims[nlayer] >= 1 && dims[nlayer] <= RVS_NN_TRAIN_MAX_NPIX;
}

// the caller's scratch, cut into 256-byte aligned pieces
struct NtWork {
  float *z[NT_MAXL], *a[NT_MAXL];   // [1 .. L-1]: pre-activations, activations
  float *gout, *gh[2], *part;
  double *losspart;
  float *dW[NT_MAXL], *db[NT_MAXL];
  int nsplit;
  int64_t bytes;
};
static NtWork nt_carve(void *work, int B, int L, const int32_t *dims) {
  NtWork w;
  char *base = (char *)work;
  int64_t off = 0;
  auto take = [&](int64_t nbytes) {
    char *p = base ? base + off : nullptr;
    off += (nbytes + 255) / 256 * 256;
    return p;
  };
  int maxhid = 1;
  for (int l = 1; l < L; l++) {
    w.z[l] = (float *)take(4ll * B * dims[l]);
    w.a[l] = (float *)take(4ll * B * dims[l]);
    if (dims[l] > maxhid) maxhid = dims[l];
  }
  const int npix = dims[L];
  w.gout = (float *)take(4ll * B * npix);
  w.gh[0] = (float *)take(4ll * B * maxhid);
  w.gh[1] = (float *)take(4ll * B * maxhid);
  w.nsplit = (npix + NT_SPLIT_K - 1) / NT_SPLIT_K;
  w.part = (float *)take(4ll * w.nsplit * B * dims[L - 1]);
  w.losspart = (double *)take(8ll * ((B + NT_BM - 1) / NT_BM) * ((npix + NT_BN - 1) / NT_BN));
  for (int l = 0; l < L; l++) {
    w.dW[l] = (float *)take(4ll * dims[l + 1] * dims[l]);
    w.db[l] = (float *)take(4ll * dims[l + 1]);
  }
  w.bytes = off;
  return w;
}

extern "C" int64_t rvs_nn_train_work_size(int T, int B, int nlayer, const int32_t *dims) {
  if (!nt_args_ok(T, B, nlayer, dims)) return RVS_E_ARG;
  return nt_carve(nullptr, B, nlayer, dims).bytes;
}

static inline dim3 nt_grid(int M, int N, int ny = 1) {
  return dim3(((M + NT_BM - 1) / NT_BM) * ((N + NT_BN - 1) / NT_BN), ny);
}

// forward + loss (+ backward when dW != NULL) of the `rows` rows idx[0 .. rows) of
// (dats, x): gradients to dW[l], db[l]; the loss to accum (+=) / step (=).
static int nt_step(const float *dats, const float *x, int T, const int32_t *idx, int rows,
                   int L, const int32_t *dims, const float *const *W, const float *const *b,
                   const float *D0, const float *SD0, double spread0, float *const *dW,
                   float *const *db, float *resid, double *accum, double *step,
                   const NtWork &w, hipStream_t st) {
  const int npix = dims[L], npc = dims[L - 1];
  for (int l = 0; l < L - 1; l++) {
    hipLaunchKernelGGL(nt_fwd_kernel, nt_grid(rows, dims[l + 1]), dim3(256), 0, st,
                       l ? w.a[l] : x, l ? nullptr : idx, T, W[l], b[l], rows, dims[l],
                       dims[l + 1], w.z[l + 1], w.a[l + 1]);
    RVS_LAUNCH_CHECK();
  }
  const double count = (double)rows * npix;
  const dim3 lgrid = nt_grid(rows, npix);
  hipLaunchKernelGGL(nt_loss_kernel, lgrid, dim3(256), 0, st, w.a[L - 1], W[L - 1],
                     b[L - 1], D0, SD0, dats, idx, T, rows, npc, npix,
                     (float)(1.0 / (count * spread0)), dW ? w.gout : nullptr, resid,
                     w.losspart);
  RVS_LAUNCH_CHECK();
  if (!dW) {
    hipLaunchKernelGGL(nt_loss_fold_kernel, dim3(1), dim3(64), 0, st, w.losspart,
                       (int)lgrid.x, spread0, count, accum, step);
    RVS_LAUNCH_CHECK();
    return 0;
  }
  // output layer: dW, db; dA split along the pixels, folded in split order
  hipLaunchKernelGGL(nt_dw_kernel, nt_grid(npix, npc), dim3(256), 0, st, w.gout,
                     w.a[L - 1], nullptr, 0, rows, npix, npc, dW[L - 1], db[L - 1]);
  RVS_LAUNCH_CHECK();
  hipLaunchKernelGGL(nt_da_split_kernel, nt_grid(rows, npc, w.nsplit), dim3(256), 0, st,
                     w.gout, W[L - 1], rows, npix, npc, w.part);
  RVS_LAUNCH_CHECK();
  const int64_t ne = (int64_t)rows * npc;
  float *g = w.gh[0], *gn = w.gh[1];
  hipLaunchKernelGGL(nt_da_fold_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0,
                     st, w.part, w.nsplit, ne, w.z[L - 1], g, w.losspart, (int)lgrid.x,
                     spread0, count, accum, step);
  RVS_LAUNCH_CHECK();
  for (int l = L - 2; l >= 0; l--) {   // g = dLoss / dz_{l+1} [rows, dims[l+1]]
    hipLaunchKernelGGL(nt_dw_kernel, nt_grid(dims[l + 1], dims[l]), dim3(256), 0, st, g,
                       l ? w.a[l] : x, l ? nullptr : idx, T, rows, dims[l + 1], dims[l],
                       dW[l], db[l]);
    RVS_LAUNCH_CHECK();
    if (l == 0) break;
    hipLaunchKernelGGL(nt_da_kernel, nt_grid(rows, dims[l]), dim3(256), 0, st, g, W[l],
                       w.z[l], rows, dims[l + 1], dims[l], gn);
    RVS_LAUNCH_CHECK();
    float *t = g;
    g = gn;
    gn = t;
  }
  return 0;
}

// the update of every tensor from the given gradients: the one launch of a step that
// writes weights, and the last (see the head of this file)
static int nt_adam(int L, const int32_t *dims, float *const *W, float *const *b,
                   const float *const *dW, const float *const *db, float *const *mW,
                   float *const *mb, float *const *vW, float *const *vb, double lr,
                   int step, hipStream_t st) {
  NtAdam A;
  int64_t end = 0;
  A.n = 2 * L;
  for (int l = 0; l < L; l++) {
    const int i = 2 * l;
    A.p[i] = W[l], A.g[i] = dW[l], A.m[i] = mW[l], A.v[i] = vW[l];
    A.end[i] = end += (int64_t)dims[l + 1] * dims[l];
    A.p[i + 1] = b[l], A.g[i + 1] = db[l], A.m[i + 1] = mb[l], A.v[i + 1] = vb[l];
    A.end[i + 1] = end += dims[l + 1];
  }
  const double bc1 = 1.0 - pow(0.9, (double)step), bc2 = 1.0 - pow(0.999, (double)step);
  hipLaunchKernelGGL(nt_adam_kernel, dim3((unsigned)((end + 255) / 256)), dim3(256), 0, st,
                     A, (float)(-(lr / bc1)), (float)sqrt(bc2));
  RVS_LAUNCH_CHECK();
  return 0;
}

static bool nt_ptrs_ok(int L, const void *const *a) {
  if (!a) return false;
  for (int l = 0; l < L; l++)
    if (!a[l]) return false;
  return true;
}
#define NT_PTRS(a) nt_ptrs_ok(nlayer, (const void *const *)(a))

extern "C" int rvs_nn_train_grad(const float *dats, const float *x, int T,
                                 const int32_t *rows, int nrows, int nlayer,
                                 const int32_t *dims, const float *const *W,
                                 const float *const *b, const float *D0, const float *SD0,
                                 double spread0, float *const *dW, float *const *db,
                                 double *loss, float *resid, void *work, void *stream) {
  if (!nt_args_ok(T, nrows, nlayer, dims) || !dats || !x || !rows || !D0 || !SD0 ||
      !loss || !work || !(spread0 > 0.0) || !NT_PTRS(W) || !NT_PTRS(b) ||
      (dW != nullptr) != (db != nullptr) || (dW && (!NT_PTRS(dW) || !NT_PTRS(db))))
    return RVS_E_ARG;
  const NtWork w = nt_carve(work, nrows, nlayer, dims);
  return nt_step(dats, x, T, rows, nrows, nlayer, dims, W, b, D0, SD0, spread0, dW, db,
                 resid, nullptr, loss, w, rvs_stream(stream));
}

extern "C" int rvs_nn_adam_step(int nlayer, const int32_t *dims, float *const *W,
                                float *const *b, const float *const *dW,
                                const float *const *db, float *const *mW, float *const *mb,
                                float *const *vW, float *const *vb, double lr, int step,
                                void *stream) {
  if (!nt_args_ok(1, 1, nlayer, dims) || step < 1 || !(lr >= 0.0) || !NT_PTRS(W) ||
      !NT_PTRS(b) || !NT_PTRS(dW) || !NT_PTRS(db) || !NT_PTRS(mW) || !NT_PTRS(mb) ||
      !NT_PTRS(vW) || !NT_PTRS(vb))
    return RVS_E_ARG;
  return nt_adam(nlayer, dims, W, b, dW, db, mW, mb, vW, vb, lr, step, rvs_stream(stream));
}

extern "C" int rvs_nn_train_epoch(const float *dats, const float *x, int T,
                                  const int32_t *perm, int ntrain, int B, int nlayer,
                                  const int32_t *dims, float *const *W, float *const *b,
                                  float *const *mW, float *const *mb, float *const *vW,
                                  float *const *vb, const float *D0, const float *SD0,
                                  double spread0, double lr, int step0, double *loss_accum,
                                  double *step_loss, void *work, void *stream) {
  if (!nt_args_ok(T, B, nlayer, dims) || ntrain < 1 || !dats || !x || !perm || !D0 ||
      !SD0 || !loss_accum || !work || !(spread0 > 0.0) || !(lr >= 0.0) || step0 < 0 ||
      !NT_PTRS(W) || !NT_PTRS(b) || !NT_PTRS(mW) || !NT_PTRS(mb) || !NT_PTRS(vW) ||
      !NT_PTRS(vb))
    return RVS_E_ARG;
  const NtWork w = nt_carve(work, B, nlayer, dims);
  hipStream_t st = rvs_stream(stream);
  int i = 0;
  for (int r0 = 0; r0 < ntrain; r0 += B, i++) {   // DataLoader(drop_last = False)
    const int rows = min(B, ntrain - r0);
    int rc = nt_step(dats, x, T, perm + r0, rows, nlayer, dims, W, b, D0, SD0, spread0,
                     w.dW, w.db, nullptr, loss_accum, step_loss ? step_loss + i : nullptr,
                     w, st);
    if (rc) return rc;
    rc = nt_adam(nlayer, dims, W, b, w.dW, w.db, mW, mb, vW, vb, lr, step0 + i + 1, st);
    if (rc) return rc;
  }
  return 0;
}
