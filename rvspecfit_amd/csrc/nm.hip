// Device-resident lock-step Nelder-Mead for S independent simplices, and the
// parameter mapping of vel_fit.chisq_func around the batched objective.
//
// vel_fit.process runs scipy's Nelder-Mead once per spectrum (vel_fit.py:627-637);
// here the S state machines live in HBM and advance together.  One round, as the
// stand-alone entry points that optimizer.py's DeviceNelderMead.minimize drives, is
//   rvs_nm_begin   termination test, centroid, reflection point  -> list1, X1
//   <objective>    F1 = f(X1)
//   rvs_nm_decide  branch per simplex; expansion / contraction point -> list2, X2
//   <objective>    F2 = f(X2)
//   rvs_nm_update  accept / replace / order; a simplex that must shrink is parked
//   (rare: rvs_nm_collect -> list3, then per vertex rvs_nm_shrink_point +
//    <objective> + rvs_nm_shrink_store, whenever the host next looks)
// Every kernel reads its job count from DEVICE memory (`counts`), so the host
// never has to synchronise inside a round: it launches with the last count it
// has seen as an upper bound (active sets only shrink) and refreshes that bound
// every few rounds.  List entries beyond the live count are padded with a copy
// of entry 0, so the objective kernels in between can run the full bound.
//
// The branch structure, constants (rho=1, chi=2, psi=0.5, sigma=0.5), stable
// vertex ordering (NaN last) and the order of the floating-point operations
// follow scipy/optimize/_optimize.py::_minimize_neldermead, the same as
// tests/refmachines/neldermead_torch.py (which tests/ checks against scipy itself).
//
// A round exists in four forms, which leave the same state to the bit:
//   stand-alone  nm_begin / nm_decide / nm_update_kernel: the entry points above
//   one block    nm_glue_begin / decide / update_kernel: rvs_nm_run, the bookkeeping
//                between two objective kernels (and their sum over the arms) in one
//   rows + pack  nm_glue_*_rows_kernel + nm_glue_*_pack_kernel: the same on as many
//                blocks as there are rows, the ordered compaction behind it
//   one launch   nm_glue_spec_prep / spec_kernel: all four candidate points of a
//                step evaluated together, one bookkeeping kernel per round
// and every part of the step is stated once, for all of them:
//   nm_case, nm_centroid, nm_point, nm_take   scipy's scalar decisions and points
//   nm_with_N                    N as a compile-time constant (the simplex in registers)
//   nm_may_step, nm_test_regs    flags and iteration count, termination test,
//                                reflection point: does the simplex step next round
//   nm_accept_regs               new point -> row N, order, store
//   nm_decide_row, nm_update_row what decide and update do for one row; glue_*_row
//                                add the value of the evaluation and the next test
//   nm_compact_rows, nm_pad_tail the rows that go on, in order, listed and mapped
// The forms differ in where a row's second value comes from, where the parked count
// is added and where a row's point waits (registers, or its own row of X1 / X2).
#include <type_traits>
#include "common.h"
#include "objective_sum.h"
#include "nm_internal.h"

// numpy evaluates every product and sum of the simplex arithmetic separately;
// a fused multiply-add would change the last bit and, eventually, the path
#pragma clang fp contract(off)

#define NM_MAXN 8
#define NM_NT 1024
// the one-block kernels that hold a whole simplex in registers ((N + 1) N + N + 1
// doubles: 98 VGPRs at N = 6, 162 at N = 8): eight waves, so that a wave has 256
#ifndef NM_UNT
#define NM_UNT 512
#endif

// counts layout (int32[8]): [0] jobs of list1, [1] jobs of list2, [2] length
// of list3, [3] simplices stepping this round, [4] simplices parked for a shrink
// flags: bit 0 active, bit 1 converged (success), bit 2 shrink pending
template <int NT = NM_NT>
__device__ __forceinline__ int block_excl_scan(int flag, int *total,
                                               int *sh /*[NT/64 + 1]*/) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = __ballot(flag);
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) sh[w] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
  for (int i = 0; i < NT / 64; i++) {
    const int c = sh[i];
    if (i < w) off += c;
    tot += c;
  }
  __syncthreads();
  *total = tot;
  return off + pre;
}

// ---------------------------------------------------------------------------
// vel_fit.ParamMapper.forward + the range / finiteness guard of chisq_func +
// VSiniMapper.to_vsini + the Normal priors of chisq_func0 (vel_fit.py:95-254)
// for J rows of the optimiser's parameter vectors.
//   X [J, n]: (vel, [vsini], free stellar parameters in specParams order)
//   src [ndim]: column of X feeding stellar parameter i, or -1 = fixed
//   fixed [S, ndim], vsini_fixed [S] (used when vsini_col < 0, nullable = no
//   rotation), prior_mean / prior_isig [S, ndim] (nullable; isig 0 = no prior)
// out: job_spec[j] = list[j], vel, vsini (nullable), params [J, ndim],
//      extra[j] = vsini penalty + priors, bad[j] (row answered with 1e30; its
//      vel/params are replaced by vel 0 / the fixed+start values `safe`)
// ---------------------------------------------------------------------------
struct MapSrc {
  int src[NM_MAXN];
};

// vel_fit.chisq_func's parameter mapping for ONE row: the optimiser's vector x of
// simplex r -> (velocity, vsini, template parameters, prior penalty, bad flag) of job j
struct MapP {
  int n, ndim, vsini_col;
  MapSrc M;
  const double *fixed, *vsini_fixed, *safe, *prior_mean, *prior_isig;
  double min_vel, max_vel, max_vsini;
  int32_t *job_spec;
  double *vel, *vsini, *params, *extra;
  int32_t *bad;
};

// entry idx of a vector that lives in registers (a chain of selects; each entry
// through a register first, or the compiler turns the chain into a load at a selected
// offset and the vector into scratch memory: template_dev.h sel_dim)
__device__ __forceinline__ double nm_pick(const double *x, int idx) {
  double v = x[0];
#pragma unroll
  for (int i = 1; i < NM_MAXN; i++) {
    double xi = x[i];
    asm volatile("" : "+v"(xi));
    v = (idx == i) ? xi : v;
  }
  return v;
}

// (x: the row in the caller's registers, NM_MAXN entries of which P.n count)
__device__ __forceinline__ void map_row_regs(const MapP &P, int j, int r,
                                             const double *x) {
  const int ndim = P.ndim;
  double v = x[0];
  double pen = 0;
  if (P.vsini) {
    double vs;
    if (P.vsini_col >= 0) {
      const double v0 = nm_pick(x, P.vsini_col);
      vs = fmin(fmax(v0, 0.0), P.max_vsini);  // np.clip
      if (v0 < 0 || v0 > P.max_vsini) pen += (vs - v0) * (vs - v0);
      if (v0 != v0) vs = v0;
    } else {
      vs = P.vsini_fixed[r];
    }
    P.vsini[j] = vs;
  }
  bool isbad = (v > P.max_vel) || (v < P.min_vel);
  double p[NM_MAXN];
#pragma unroll
  for (int i = 0; i < NM_MAXN; i++) {   // (p[] in registers: static indices)
    if (i >= ndim) break;
    p[i] = (P.M.src[i] >= 0) ? nm_pick(x, P.M.src[i]) : P.fixed[(int64_t)r * ndim + i];
    if (!(fabs(p[i]) <= 1.79e308)) isbad = true;
  }
  if (isbad) {
    v = 0;
#pragma unroll
    for (int i = 0; i < NM_MAXN; i++)
      if (i < ndim) p[i] = P.safe[(int64_t)r * ndim + i];
  }
  if (P.prior_mean)
#pragma unroll
    for (int i = 0; i < NM_MAXN; i++) {
      if (i >= ndim) break;
      const double d = (P.prior_mean[(int64_t)r * ndim + i] - p[i]) *
                       P.prior_isig[(int64_t)r * ndim + i];
      pen += d * d;
    }
  P.job_spec[j] = r;
  P.vel[j] = v;
#pragma unroll
  for (int i = 0; i < NM_MAXN; i++)
    if (i < ndim) P.params[(int64_t)j * ndim + i] = p[i];
  P.extra[j] = pen;
  P.bad[j] = isbad ? 1 : 0;
}

// row i < N of x (memory) <-> xr (registers: no indexing by a loop variable)
__device__ __forceinline__ void nm_get_row(double *xr, const double *x, int N) {
#pragma unroll
  for (int i = 0; i < NM_MAXN; i++) xr[i] = (i < N) ? x[i] : 0.0;
}
__device__ __forceinline__ void nm_put_row(double *x, const double *xr, int N) {
#pragma unroll
  for (int i = 0; i < NM_MAXN; i++)
    if (i < N) x[i] = xr[i];
}

// ---------------------------------------------------------------------------
// scipy's step, every part once
// ---------------------------------------------------------------------------

// body(std::integral_constant<int, N>): the simplex of N + 1 vertices in registers
// needs N at compile time (all loops unroll, all indices are static)
template <typename BODY>
__device__ __forceinline__ void nm_with_N(int N, BODY body) {
  switch (N) {
    case 1: body(std::integral_constant<int, 1>()); break;
    case 2: body(std::integral_constant<int, 2>()); break;
    case 3: body(std::integral_constant<int, 3>()); break;
    case 4: body(std::integral_constant<int, 4>()); break;
    case 5: body(std::integral_constant<int, 5>()); break;
    case 6: body(std::integral_constant<int, 6>()); break;
    case 7: body(std::integral_constant<int, 7>()); break;
    default: body(std::integral_constant<int, 8>()); break;
  }
}

// the case of a step from the value of the reflection point and the ordered values of
// the simplex: 0 accept reflection, 1 expansion, 2 outside contraction, 3 inside
__device__ __forceinline__ int nm_case(double fxr, double f0, double fn1, double fn) {
  if (fxr < f0) return 1;
  if (fxr < fn1) return 0;
  if (fxr < fn) return 2;
  return 3;
}

// one coordinate of the centroid of the N best vertices (v(k): that coordinate of
// vertex k): the sum in vertex order, then / N
template <typename V>
__device__ __forceinline__ double nm_centroid(int N, V v) {
  double xb = v(0);
  for (int k = 1; k < N; k++) xb = xb + v(k);
  return xb / N;
}

// one coordinate of the point of case c (0: the reflection point) from the centroid xb
// and the worst vertex w, scipy's expressions
__device__ __forceinline__ double nm_point(int c, double xb, double w) {
  if (c == 0) return (1 + 1.0) * xb - 1.0 * w;
  if (c == 1) return (1 + 1.0 * 2.0) * xb - 1.0 * 2.0 * w;
  if (c == 2) return (1 + 0.5 * 1.0) * xb - 0.5 * 1.0 * w;
  return (1 - 0.5) * xb + 0.5 * w;
}

// which point replaces the worst vertex (fxr: value of the reflection point, f2: of the
// second point of case c, fn: the worst vertex's), or none: the simplex must shrink
enum { NM_SHRINK, NM_TAKE_R, NM_TAKE_2 };
__device__ __forceinline__ int nm_take(int c, double fxr, double f2, double fn) {
  if (c == 0) return NM_TAKE_R;
  if (c == 1) return (f2 < fxr) ? NM_TAKE_2 : NM_TAKE_R;
  if (c == 2) return (f2 <= fxr) ? NM_TAKE_2 : NM_SHRINK;
  return (f2 < fn) ? NM_TAKE_2 : NM_SHRINK;
}

// The simplex is pulled into registers (N is a template parameter, all loops unroll):
// sorting it in place in global memory is a chain of ~50 dependent loads/stores, which
// made the bookkeeping kernels latency-bound.
template <int N>
__device__ __forceinline__ void nm_load_regs(const double *__restrict__ gs,
                                             const double *__restrict__ gf,
                                             double (&s)[N + 1][N], double (&f)[N + 1],
                                             int rows = N + 1) {
#pragma unroll
  for (int a = 0; a <= N; a++) {
    if (a >= rows) break;
    f[a] = gf[a];
#pragma unroll
    for (int i = 0; i < N; i++) s[a][i] = gs[a * N + i];
  }
}

template <int N>
__device__ __forceinline__ void nm_store_regs(double *gs, double *gf,
                                              const double (&s)[N + 1][N],
                                              const double (&f)[N + 1]) {
#pragma unroll
  for (int a = 0; a <= N; a++) {
    gf[a] = f[a];
#pragma unroll
    for (int i = 0; i < N; i++) gs[a * N + i] = s[a][i];
  }
}

// stable insertion sort of the N+1 vertices by f (NaN last), np.argsort order
template <int N>
__device__ __forceinline__ void nm_sort_regs(double (&s)[N + 1][N], double (&f)[N + 1]) {
#pragma unroll
  for (int a = 1; a <= N; a++) {
    const double fa = f[a];
    const double ka = (fa != fa) ? __builtin_inf() : fa;
    double xa[N];
#pragma unroll
    for (int i = 0; i < N; i++) xa[i] = s[a][i];
    bool placed = false;
#pragma unroll
    for (int b = a - 1; b >= 0; b--) {
      if (!placed) {
        const double fb = f[b];
        const double kb = (fb != fb) ? __builtin_inf() : fb;
        if (kb > ka) {
          f[b + 1] = fb;
#pragma unroll
          for (int i = 0; i < N; i++) s[b + 1][i] = s[b][i];
          if (b == 0) {
            f[0] = fa;
#pragma unroll
            for (int i = 0; i < N; i++) s[0][i] = xa[i];
            placed = true;
          }
        } else {
          f[b + 1] = fa;
#pragma unroll
          for (int i = 0; i < N; i++) s[b + 1][i] = xa[i];
          placed = true;
        }
      }
    }
  }
}

// the simplex at (gs, gf) ordered in place (after a shrink: all values are new)
__device__ void nm_order(double *gs, double *gf, int N) {
  nm_with_N(N, [&](auto n) {
    constexpr int NN = decltype(n)::value;
    double s[NN + 1][NN], f[NN + 1];
    nm_load_regs<NN>(gs, gf, s, f);
    nm_sort_regs<NN>(s, f);
    nm_store_regs<NN>(gs, gf, s, f);
  });
}

// The accepted point (src, fnew) becomes row N of the simplex at (gs, gf), the rows are
// ordered and stored; s, f stay with the caller, so that the next round's test and
// points come off the same registers -- the same operations on the same values as the
// steps through memory (store row N; load, sort, store; load, test), two round trips
// shorter.
template <int N>
__device__ __forceinline__ void nm_accept_regs(double *gs, double *gf,
                                               const double *__restrict__ src,
                                               double fnew, double (&s)[N + 1][N],
                                               double (&f)[N + 1]) {
  nm_load_regs<N>(gs, gf, s, f, N);
#pragma unroll
  for (int i = 0; i < N; i++) s[N][i] = src[i];
  f[N] = fnew;
  nm_sort_regs<N>(s, f);
  nm_store_regs<N>(gs, gf, s, f);
}

// May simplex r, after `nit` iterations, step in the coming round?  Not when it is
// not active or a shrink is pending; at maxiter it stops (scipy: the while-condition
// fails -> warnflag 2).
__device__ __forceinline__ bool nm_may_step(int32_t *flags, int r, int nit,
                                            int maxiter) {
  const int fl = flags[r];
  if ((fl & 5) != 1) return false;
  if (nit >= maxiter) {
    flags[r] = fl & ~1;
    return false;
  }
  return true;
}

// ... and does it?  scipy's termination test on the ordered simplex: converged
// (success) -> flags, 0; else 1 and xr = its reflection point
template <int N>
__device__ __forceinline__ int nm_test_regs(int32_t *flags, int r,
                                            const double (&s)[N + 1][N],
                                            const double (&f)[N + 1], double xatol,
                                            double fatol, double *xr) {
  double dx = 0, df = 0;
  bool anynan = (f[0] != f[0]);
#pragma unroll
  for (int k = 1; k <= N; k++) {
#pragma unroll
    for (int i = 0; i < N; i++) {
      dx = fmax(dx, fabs(s[k][i] - s[0][i]));
      if (s[k][i] != s[k][i] || s[0][i] != s[0][i]) anynan = true;
    }
    df = fmax(df, fabs(f[0] - f[k]));
    if (f[k] != f[k]) anynan = true;
  }
  // NaN propagates like np.max: a NaN difference never passes the test
  if (!anynan && dx <= xatol && df <= fatol) {
    flags[r] = (flags[r] & ~1) | 2;
    return 0;
  }
#pragma unroll
  for (int i = 0; i < N; i++)
    xr[i] = nm_point(0, nm_centroid(N, [&](int k) { return s[k][i]; }), s[N][i]);
  return 1;
}

// the three other points a step can ask for (cases 1, 2, 3) -> xc
template <int N>
__device__ __forceinline__ void nm_other_points(const double (&s)[N + 1][N],
                                                double (*xc)[NM_MAXN]) {
#pragma unroll
  for (int i = 0; i < N; i++) {
    const double xb = nm_centroid(N, [&](int k) { return s[k][i]; });
    xc[0][i] = nm_point(1, xb, s[N][i]);
    xc[1][i] = nm_point(2, xb, s[N][i]);
    xc[2][i] = nm_point(3, xb, s[N][i]);
  }
}

// begin, one row: does simplex r step this round (xr = its reflection point)?  The
// simplex is read only when its flags let it through.
__device__ __forceinline__ int nm_begin_row(int N, const double *__restrict__ sim,
                                            const double *__restrict__ fsim,
                                            const int32_t *__restrict__ nit,
                                            int32_t *flags, int r, int maxiter,
                                            double xatol, double fatol, double *xr) {
  if (!nm_may_step(flags, r, nit[r], maxiter)) return 0;
  int go = 0;
  nm_with_N(N, [&](auto n) {
    constexpr int NN = decltype(n)::value;
    double s[NN + 1][NN], f[NN + 1];
    nm_load_regs<NN>(sim + (int64_t)r * (NN + 1) * NN, fsim + (int64_t)r * (NN + 1), s, f);
    go = nm_test_regs<NN>(flags, r, s, f, xatol, fatol, xr);
  });
  return go;
}

// decide, one row: case c of the simplex at gs (memory: N at run time, one vertex at a
// time) -> *case_j; the second point the case asks for -> x2 (registers: static
// indices); returns 1 when there is one
__device__ __forceinline__ int nm_decide_row(int N, const double *__restrict__ gs, int c,
                                             int32_t *case_j, double *x2) {
  *case_j = c;
  if (c == 0) return 0;
#pragma unroll
  for (int i = 0; i < NM_MAXN; i++) {
    if (i >= N) break;
    x2[i] = nm_point(c, nm_centroid(N, [&](int k) { return gs[k * N + i]; }),
                     gs[N * N + i]);
  }
  return 1;
}

// update, one row: the point that is taken (xr or x2, values fxr / f2; nfev as scipy
// counts) accepted into the simplex at (gs, gf), one iteration more: returns the new
// iteration count (>= 1; s, f = the ordered simplex), or 0 = the simplex must shrink
template <int N>
__device__ __forceinline__ int nm_update_row(double *gs, double *gf, int32_t *nit_r,
                                             int32_t *nfev_r, int c, double fxr,
                                             double f2, double fn, const double *xr,
                                             const double *x2, double (&s)[N + 1][N],
                                             double (&f)[N + 1]) {
  const int take = nm_take(c, fxr, f2, fn);
  *nfev_r += (c == 0) ? 1 : 2;
  if (take == NM_SHRINK) return 0;
  const bool take2 = (take == NM_TAKE_2);
  nm_accept_regs<N>(gs, gf, take2 ? x2 : xr, take2 ? f2 : fxr, s, f);
  const int nit = *nit_r + 1;
  *nit_r = nit;
  return nit;
}

// The rows j < J that go on move, in order, to the front of (list, X) and are mapped
// (P: nullable): row(j, r, x) says whether row j goes on, and if so leaves its simplex
// and its point (registers).  pos_out[j] = the row's new position or -1 (nullable).
// One block of NT threads, trips of NT rows; returns the count.  A row's new position is
// at or before j: whatever row() reads of the rows of its trip and of later rows is
// read before a position is written, provided the values are in registers by then.
template <int NT, typename ROW>
__device__ __forceinline__ int nm_compact_rows(const MapP *P, int N, int J, ROW row,
                                               int32_t *list, double *X,
                                               int32_t *pos_out,
                                               int *sh /*[NT/64 + 1]*/) {
  int base_out = 0;
  for (int j0 = 0; j0 < J; j0 += NT) {
    const int j = j0 + threadIdx.x;
    int go = 0, r = 0;
    double x[NM_MAXN] = {};
    if (j < J) go = row(j, r, x);
    int tot;
    const int pos = base_out + block_excl_scan<NT>(go, &tot, sh);
    if (pos_out && j < J) pos_out[j] = go ? pos : -1;
    if (go) {
      list[pos] = r;
      nm_put_row(X + (int64_t)pos * N, x, N);
      if (P) map_row_regs(*P, pos, r, x);
    }
    base_out += tot;
  }
  return base_out;
}

// entries [max(n, 1), jbound) of (list, X) <- a copy of entry 0 (simplex 0's best
// vertex when the list is empty)
__device__ __forceinline__ void nm_pad_tail(int n, int jbound, int N, int32_t *list,
                                            double *X, const double *sim) {
  if (n == 0 && threadIdx.x == 0) {
    list[0] = 0;
    for (int i = 0; i < N; i++) X[i] = sim[i];
  }
  __syncthreads();
  for (int j = max(n, 1) + threadIdx.x; j < jbound; j += NM_NT) {
    list[j] = list[0];
    for (int i = 0; i < N; i++) X[(int64_t)j * N + i] = X[i];
  }
}

// ---------------------------------------------------------------------------
// The stand-alone round
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(NM_NT)
    nm_begin_kernel(int S, int N, double xatol, double fatol, int maxiter,
                    const double *__restrict__ sim,
                    const double *__restrict__ fsim,
                    const int32_t *__restrict__ nit, int32_t *__restrict__ flags,
                    int32_t *__restrict__ list1, double *__restrict__ X1,
                    int32_t *__restrict__ counts, int jbound) {
  __shared__ int sh[NM_NT / 64 + 1];
  const int n = nm_compact_rows<NM_NT>(
      nullptr, N, S,
      [&](int j, int &r, double *xr) {
        r = j;
        return nm_begin_row(N, sim, fsim, nit, flags, j, maxiter, xatol, fatol, xr);
      },
      list1, X1, nullptr, sh);
  __syncthreads();
  if (threadIdx.x == 0) {
    counts[0] = n;
    counts[3] = n;
  }
  nm_pad_tail(n, jbound, N, list1, X1, sim);
}

__global__ void __launch_bounds__(NM_NT)
    nm_decide_kernel(int N, const double *__restrict__ sim,
                     const double *__restrict__ fsim,
                     const int32_t *__restrict__ list1,
                     const double *__restrict__ F1, int32_t *__restrict__ cases,
                     int32_t *__restrict__ pos2, int32_t *__restrict__ list2,
                     double *__restrict__ X2, int32_t *__restrict__ counts,
                     int jbound) {
  __shared__ int sh[NM_NT / 64 + 1];
  const int J = min(counts[0], jbound);
  const int n = nm_compact_rows<NM_NT>(
      nullptr, N, J,
      [&](int j, int &r, double *x2) {
        r = list1[j];
        const double *f = fsim + (int64_t)r * (N + 1);
        return nm_decide_row(N, sim + (int64_t)r * (N + 1) * N,
                             nm_case(F1[j], f[0], f[N - 1], f[N]), &cases[j], x2);
      },
      list2, X2, pos2, sh);
  __syncthreads();
  if (threadIdx.x == 0) counts[1] = n;
  nm_pad_tail(n, jbound, N, list2, X2, sim);
}

__global__ void __launch_bounds__(NM_NT)
    nm_update_kernel(int N, double *__restrict__ sim, double *__restrict__ fsim,
                     int32_t *__restrict__ nit, int32_t *__restrict__ nfev,
                     const int32_t *__restrict__ list1,
                     const double *__restrict__ X1,
                     const double *__restrict__ F1,
                     const int32_t *__restrict__ cases,
                     const int32_t *__restrict__ pos2,
                     const double *__restrict__ X2,
                     const double *__restrict__ F2, int32_t *__restrict__ flags,
                     int32_t *__restrict__ counts, int jbound) {
  __shared__ int sh[NM_NT / 64 + 1];
  const int J = min(counts[0], jbound);
  int parked = 0;
  for (int j0 = 0; j0 < J; j0 += NM_NT) {
    const int j = j0 + threadIdx.x;
    int go = 0;
    if (j < J) {
      const int r = list1[j];
      double *gf = fsim + (int64_t)r * (N + 1);
      const int p2 = pos2[j];
      const double f2 = (p2 >= 0) ? F2[p2] : __builtin_inf();
      nm_with_N(N, [&](auto n) {
        constexpr int NN = decltype(n)::value;
        double s[NN + 1][NN], f[NN + 1];
        go = !nm_update_row<NN>(sim + (int64_t)r * (NN + 1) * NN, gf, &nit[r], &nfev[r],
                                cases[j], F1[j], f2, gf[NN], X1 + (int64_t)j * NN,
                                X2 + (int64_t)p2 * NN, s, f);
      });
      // shrink: parked (flag bit 2) until the host runs the shrink
      if (go) flags[r] |= 4;
    }
    int tot;
    block_excl_scan(go, &tot, sh);
    parked += tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) counts[4] += parked;  // simplices waiting to shrink
}

// list3 = simplices with a pending shrink (flag bit 2), counts[2] = how many
__global__ void __launch_bounds__(NM_NT)
    nm_collect_kernel(int S, const int32_t *__restrict__ flags,
                      int32_t *__restrict__ list3,
                      int32_t *__restrict__ counts) {
  __shared__ int sh[NM_NT / 64 + 1];
  int base_out = 0;
  for (int r0 = 0; r0 < S; r0 += NM_NT) {
    const int r = r0 + threadIdx.x;
    const int go = (r < S && (flags[r] & 4)) ? 1 : 0;
    int tot;
    const int pos = base_out + block_excl_scan(go, &tot, sh);
    if (go) list3[pos] = r;
    base_out += tot;
  }
  __syncthreads();
  if (threadIdx.x == 0) counts[2] = base_out;
}

// vertex k (1..N) of every shrinking simplex: sim[k] = sim[0] + 0.5 (sim[k]-sim[0])
__global__ void __launch_bounds__(256)
    nm_shrink_point_kernel(int N, int k, double *__restrict__ sim,
                           const int32_t *__restrict__ list3,
                           double *__restrict__ X3,
                           const int32_t *__restrict__ counts, int jbound) {
  const int J = min(counts[2], jbound);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= jbound) return;
  const int jj = (j < J) ? j : 0;
  const int r = (J > 0) ? list3[jj] : 0;
  double *s = sim + (int64_t)r * (N + 1) * N;
  for (int i = 0; i < N; i++) {
    double v = s[i];
    if (J > 0) {
      v = s[i] + 0.5 * (s[k * N + i] - s[i]);
      if (j < J) s[k * N + i] = v;
    }
    X3[(int64_t)j * N + i] = v;
  }
}

__global__ void __launch_bounds__(256)
    nm_shrink_store_kernel(int N, int k, double *__restrict__ sim,
                           double *__restrict__ fsim,
                           int32_t *__restrict__ nit, int32_t *__restrict__ nfev,
                           int32_t *__restrict__ flags,
                           const int32_t *__restrict__ list3,
                           const double *__restrict__ F3,
                           int32_t *__restrict__ counts, int jbound) {
  const int J = min(counts[2], jbound);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= J) return;
  const int r = list3[j];
  fsim[(int64_t)r * (N + 1) + k] = F3[j];
  if (k == N) {
    nm_order(sim + (int64_t)r * (N + 1) * N, fsim + (int64_t)r * (N + 1), N);
    nit[r] += 1;
    nfev[r] += N;
    flags[r] &= ~4;
    if (j == 0) counts[4] = 0;
  }
}

extern "C" int rvs_nm_begin(int S, int N, double xatol, double fatol,
                            int maxiter, const double *sim, const double *fsim,
                            const int32_t *nit, int32_t *flags, int32_t *list1,
                            double *X1, int32_t *counts, int jbound,
                            void *stream) {
  if (S < 1 || N < 1 || N > NM_MAXN || jbound < 1) return RVS_E_ARG;
  hipLaunchKernelGGL(nm_begin_kernel, dim3(1), dim3(NM_NT), 0,
                     rvs_stream(stream), S, N, xatol, fatol, maxiter, sim, fsim,
                     nit, flags, list1, X1, counts, jbound);
  RVS_LAUNCH_CHECK();
  return 0;
}

extern "C" int rvs_nm_decide(int N, const double *sim, const double *fsim,
                             const int32_t *list1, const double *F1,
                             int32_t *cases, int32_t *pos2, int32_t *list2,
                             double *X2, int32_t *counts, int jbound,
                             void *stream) {
  if (N < 1 || N > NM_MAXN || jbound < 1) return RVS_E_ARG;
  hipLaunchKernelGGL(nm_decide_kernel, dim3(1), dim3(NM_NT), 0,
                     rvs_stream(stream), N, sim, fsim, list1, F1, cases, pos2,
                     list2, X2, counts, jbound);
  RVS_LAUNCH_CHECK();
  return 0;
}

extern "C" int rvs_nm_update(int N, double *sim, double *fsim, int32_t *nit,
                             int32_t *nfev, const int32_t *list1,
                             const double *X1, const double *F1,
                             const int32_t *cases, const int32_t *pos2,
                             const double *X2, const double *F2, int32_t *flags,
                             int32_t *counts, int jbound, void *stream) {
  if (N < 1 || N > NM_MAXN || jbound < 1) return RVS_E_ARG;
  hipLaunchKernelGGL(nm_update_kernel, dim3(1), dim3(NM_NT), 0,
                     rvs_stream(stream), N, sim, fsim, nit, nfev, list1, X1, F1,
                     cases, pos2, X2, F2, flags, counts, jbound);
  RVS_LAUNCH_CHECK();
  return 0;
}

extern "C" int rvs_nm_collect(int S, const int32_t *flags, int32_t *list3,
                              int32_t *counts, void *stream) {
  if (S < 1) return RVS_E_ARG;
  hipLaunchKernelGGL(nm_collect_kernel, dim3(1), dim3(NM_NT), 0,
                     rvs_stream(stream), S, flags, list3, counts);
  RVS_LAUNCH_CHECK();
  return 0;
}

extern "C" int rvs_nm_shrink_point(int N, int k, double *sim,
                                   const int32_t *list3, double *X3,
                                   const int32_t *counts, int jbound,
                                   void *stream) {
  if (N < 1 || N > NM_MAXN || k < 1 || k > N || jbound < 1) return RVS_E_ARG;
  hipLaunchKernelGGL(nm_shrink_point_kernel, dim3((jbound + 255) / 256),
                     dim3(256), 0, rvs_stream(stream), N, k, sim, list3, X3,
                     counts, jbound);
  RVS_LAUNCH_CHECK();
  return 0;
}

extern "C" int rvs_nm_shrink_store(int N, int k, double *sim, double *fsim,
                                   int32_t *nit, int32_t *nfev, int32_t *flags,
                                   const int32_t *list3, const double *F3,
                                   int32_t *counts, int jbound, void *stream) {
  if (N < 1 || N > NM_MAXN || k < 1 || k > N || jbound < 1) return RVS_E_ARG;
  hipLaunchKernelGGL(nm_shrink_store_kernel, dim3((jbound + 255) / 256),
                     dim3(256), 0, rvs_stream(stream), N, k, sim, fsim, nit,
                     nfev, flags, list3, F3, counts, jbound);
  RVS_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// The parameter mapping and the objective around it as launches of their own
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
    proc_map_kernel(int J, const double *__restrict__ X,
                    const int32_t *__restrict__ list, MapP P) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= J) return;
  double xr[NM_MAXN];
  nm_get_row(xr, X + (int64_t)j * P.n, P.n);
  map_row_regs(P, j, list[j], xr);
}

__global__ void __launch_bounds__(256)
    proc_finish_kernel(int J, const int32_t *__restrict__ counts, int cidx,
                       const double *__restrict__ chi,
                       const double *__restrict__ extra,
                       const int32_t *__restrict__ bad,
                       const int32_t *__restrict__ job_spec,
                       const int32_t *__restrict__ job_status,
                       double *__restrict__ F,
                       int32_t *__restrict__ spec_status) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= J) return;
  F[j] = bad[j] ? 1e30 : chi[j] + extra[j];
  const int live = counts ? counts[cidx] : J;
  if (j < live && job_status[j] && !bad[j])
    atomicOr(&spec_status[job_spec[j]], job_status[j]);
}

// the mapping's parameters as the kernels take them (o->n, o->ndim checked by the caller)
static MapP map_params(const rvs_nm_objective *o) {
  MapP P;
  P.n = o->n, P.ndim = o->ndim, P.vsini_col = o->vsini_col;
  for (int i = 0; i < NM_MAXN; i++) P.M.src[i] = (i < o->ndim) ? o->src[i] : -1;
  P.fixed = o->fixed, P.vsini_fixed = o->vsini_fixed, P.safe = o->safe;
  P.prior_mean = o->prior_mean, P.prior_isig = o->prior_isig;
  P.min_vel = o->min_vel, P.max_vel = o->max_vel, P.max_vsini = o->max_vsini;
  P.job_spec = o->job_spec, P.vel = o->vel, P.vsini = o->vsini, P.params = o->params;
  P.extra = o->extra, P.bad = o->bad;
  return P;
}

// rvs_proc_map on an objective's own tables and row buffers (nm_internal.h: what the
// round evaluators of this file, bfgs_grad.hip, bfgs_dev.hip and lm_dev.hip call)
int rvs_internal_proc_map(int J, const double *X, const int32_t *list,
                          const rvs_nm_objective *o, hipStream_t st) {
  if (J < 1 || o->n < 1 || o->n > NM_MAXN || o->ndim < 1 || o->ndim > NM_MAXN)
    return RVS_E_ARG;
  hipLaunchKernelGGL(proc_map_kernel, dim3((J + 255) / 256), dim3(256), 0, st, J, X,
                     list, map_params(o));
  RVS_LAUNCH_CHECK();
  return 0;
}

extern "C" int rvs_proc_map(int J, int n, int ndim, const double *X,
                            const int32_t *list, const int32_t *src,
                            int vsini_col, const double *fixed,
                            const double *vsini_fixed, const double *safe,
                            const double *prior_mean, const double *prior_isig,
                            double min_vel, double max_vel, double max_vsini,
                            int32_t *job_spec, double *vel, double *vsini,
                            double *params, double *extra, int32_t *bad,
                            void *stream) {
  rvs_nm_objective o = {};
  o.n = n, o.ndim = ndim, o.vsini_col = vsini_col;
  for (int i = 0; i < NM_MAXN && i < ndim; i++) o.src[i] = src[i];
  o.fixed = fixed, o.vsini_fixed = vsini_fixed, o.safe = safe;
  o.prior_mean = prior_mean, o.prior_isig = prior_isig;
  o.min_vel = min_vel, o.max_vel = max_vel, o.max_vsini = max_vsini;
  o.job_spec = job_spec, o.vel = vel, o.vsini = vsini, o.params = params;
  o.extra = extra, o.bad = bad;
  return rvs_internal_proc_map(J, X, list, &o, rvs_stream(stream));
}

extern "C" int rvs_proc_finish(int J, const int32_t *counts, int cidx,
                               const double *chi, const double *extra,
                               const int32_t *bad, const int32_t *job_spec,
                               const int32_t *job_status, double *F,
                               int32_t *spec_status, void *stream) {
  if (J < 1) return RVS_E_ARG;
  hipLaunchKernelGGL(proc_finish_kernel, dim3((J + 255) / 256), dim3(256), 0,
                     rvs_stream(stream), J, counts, cidx, chi, extra, bad,
                     job_spec, job_status, F, spec_status);
  RVS_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// The rounds of the lock-step optimiser driven from C: what optimizer.py's
// DeviceNelderMead.minimize + ProcessObjective.eval do per round (begin -> map ->
// objective -> finish -> decide -> map -> objective -> finish -> update, the
// host looking at the counters every `sync_every` rounds, parked shrinks run at
// that look), without ~25 interpreter round trips per round.  The call blocks
// its host thread but not the interpreter (ctypes releases the GIL), so two
// optimiser instances on two streams can be driven by two Python threads.
// ---------------------------------------------------------------------------

// The objective of the rows that are mapped already (o->params, o->vel, ...; J = launch
// bound, `live` = their count on the device, null = all J): the template rows from the
// evaluator where the library builds them, then the objective kernel.  With
// RVS_OBJ_NO_SUM in `flags` the per-arm results stay in o->scratch for the bookkeeping
// kernels (chi, jstatus null); with RVS_OBJ_STATUS_STORE their sum goes to chi / jstatus.
static int nm_objective_rows(const rvs_nm_objective *o, int J, const int32_t *live,
                             int flags, double *chi, int32_t *jstatus, hipStream_t st) {
  if (!o->nn && !o->tri)   // regular grids: the gather happens inside the kernel
    return rvs_objective_fused_n(o->arms, o->narm, o->npoly, o->params, o->vsini,
                                 o->job_spec, J, live, o->vel, o->badchi, flags,
                                 o->scratch, chi, jstatus, st);
  // MLP libraries: the round's template rows and outside flags per arm; Delaunay
  // libraries: find_simplex + blend per arm; then broadening + spline + chi^2 in one
  // kernel (optimizer.py's from_template form)
  const double *tp[8], *op[8];
  if (o->narm > 8) return RVS_E_ARG;
  // (one grouped launch chain for the arms.  Forked onto side streams the
  // per-arm chains overlapped inside one optimiser instance -- Nelder-Mead
  // 2.53 -> 2.36 s per 2000 spectra -- but two instances on two host threads,
  // which is how vel_fit.process runs a large batch, then took 3.5 s for 2.4)
  int rc = o->nn ? rvs_template_nn_arms_n(o->params, J, live, o->ndim, o->narm, o->nn, st)
                 : rvs_internal_template_tri_arms_n(o->params, J, live, o->ndim,
                                                    o->narm, o->tri, st);
  if (rc) return rc;
  for (int a = 0; a < o->narm; a++) {
    tp[a] = o->nn ? o->nn[a].templ : o->tri[a].templ;
    op[a] = o->nn ? o->nn[a].outside : o->tri[a].outside;
  }
  return rvs_objective_from_template_n(o->arms, o->narm, o->npoly, tp, op, o->vsini,
                                       o->job_spec, J, live, o->vel, o->badchi, flags,
                                       o->scratch, chi, jstatus, st);
}

int rvs_internal_nm_eval(const rvs_nm_objective *o, const int32_t *list,
                         const double *X, int J, const int32_t *counts, int cidx,
                         double *F, hipStream_t st) {
  int rc = rvs_internal_proc_map(J, X, list, o, st);
  if (rc) return rc;
  // rows behind the device count (simplices that finished since the host's last look,
  // simplices that need no second point this round) are not evaluated: a quarter of
  // the objective blocks of a run (tools/perf/nm_waste.py).  (Sizing the second
  // launch exactly by one more look per round: 2390-2445 against 2398 spectra/s,
  // no difference -- a block behind the count costs next to nothing.)
  rc = nm_objective_rows(o, J, counts ? counts + cidx : nullptr,
                         1 | RVS_OBJ_STATUS_STORE, o->chi, o->jstatus, st);
  if (rc) return rc;
  return rvs_proc_finish(J, counts, cidx, o->chi, o->extra, o->bad, o->job_spec,
                         o->jstatus, F, o->status, st);
}


// ---------------------------------------------------------------------------
// The round as rvs_nm_run launches it: THREE launches per function evaluation --
// cell search, job order, objective kernel -- and one bookkeeping kernel between two
// evaluations, where a round of the stand-alone entry points (rvs_nm_begin / _decide /
// _update around the objective, as optimizer.py drives them) takes seven (begin |
// decide | update, map, cell search, order, objective, sum over the arms, finish).
// Between two objective kernels of a stream nothing else runs, and late in a run -- a
// few dozen simplices left, an objective launch of 40 us -- that chain of launches WAS
// the round: 141 us of small launches per evaluation (tools/perf/trace_rounds.py).  One
// block does, for all rows, what the stand-alone kernels do (same device functions, same
// order of the arithmetic, lists in the same order):
//   nm_glue_begin     termination test + reflection point of every running simplex,
//                     list1 / X1, and the parameter mapping of those rows
//   nm_glue_decide    F1 = sum over the arms + priors of the rows just evaluated;
//                     branch per simplex; second point -> list2 / X2 + their mapping
//   nm_glue_update    F2 likewise; accept / replace / order / park; then the next
//                     round's termination test + reflection point of the simplices
//                     that keep running (list1 compacted in place) + their mapping
// The function values are formed for ALL rows before any mapped row is written (the
// mapping of the next rows lives in the buffers the evaluated rows are read from).
// ---------------------------------------------------------------------------
struct NmGlue {
  rvs_nm_state m;
  MapP P;
  ObjArmOut AO;           // per-arm results of the evaluation just done
  double badchi, xatol, fatol;
  const double *pen_scale;
  int32_t *spec_status;
  int maxiter;
};

// F of row j of the evaluation just done (objective_sum_kernel + proc_finish_kernel)
__device__ __forceinline__ double glue_value(const NmGlue &G, int j) {
  const int r = G.P.job_spec[j];
  double bc = G.badchi;
  if (G.pen_scale) bc *= G.pen_scale[r];
  double tot;
  int st;
  obj_sum_row(G.AO, j, bc, 1, tot, st);
  const int isbad = G.P.bad[j];
  if (st && !isbad) atomicOr(&G.spec_status[r], st);
  return isbad ? 1e30 : tot + G.P.extra[j];
}

__device__ __forceinline__ int glue_begin_row(const NmGlue &G, int r, double *xr) {
  return nm_begin_row(G.m.N, G.m.sim, G.m.fsim, G.m.nit, G.m.flags, r, G.maxiter,
                      G.xatol, G.fatol, xr);
}

// the value of row j's evaluation -> F1[j], fxr, and the case of its simplex r (fn: the
// worst vertex's value, for the update)
__device__ __forceinline__ int glue_case_row(const NmGlue &G, int j, int r, double &fxr,
                                             double &fn) {
  const int N = G.m.N;
  const double *f = G.m.fsim + (int64_t)r * (N + 1);
  // (the simplex values requested ahead of the evaluation's chain of loads)
  const double f0 = f[0], fn1 = f[N - 1];
  fn = f[N];
  fxr = glue_value(G, j);
  G.m.F1[j] = fxr;
  return nm_case(fxr, f0, fn1, fn);
}

// decide row j: its simplex r, its value, its case (-> cases[j]); 1 = it asks for a
// second point, x2
__device__ __forceinline__ int glue_decide_row(const NmGlue &G, int j, int &r,
                                               double *x2) {
  const int N = G.m.N;
  r = G.m.list1[j];
  double fxr, fn;
  const int c = glue_case_row(G, j, r, fxr, fn);
  return nm_decide_row(N, G.m.sim + (int64_t)r * (N + 1) * N, c, &G.m.cases[j], x2);
}

// update row j of simplex r, case c, with the value f2 of its second point (row p2 of
// X2; none: p2 < 0, f2 = inf): the step's point accepted, or the simplex parked for a
// shrink (counted in *parked); then the next round's test of the simplex on the same
// registers: 1 = it steps, xr = its reflection point (xc: its other points, nullable)
template <int N>
__device__ __forceinline__ int glue_update_row(const NmGlue &G, int j, int r, int c,
                                               double fxr, double f2, double fn,
                                               const double *X2, int p2, int *parked,
                                               double *xr, double (*xc)[NM_MAXN]) {
  double s[N + 1][N], f[N + 1];
  const int nit = nm_update_row<N>(G.m.sim + (int64_t)r * (N + 1) * N,
                                   G.m.fsim + (int64_t)r * (N + 1), &G.m.nit[r],
                                   &G.m.nfev[r], c, fxr, f2, fn, G.m.X1 + (int64_t)j * N,
                                   X2 + (int64_t)p2 * N, s, f);
  if (!nit) {
    G.m.flags[r] |= 4;  // shrink: parked until the host runs the shrink
    atomicAdd(parked, 1);
    return 0;
  }
  if (!nm_may_step(G.m.flags, r, nit, G.maxiter)) return 0;
  if (!nm_test_regs<N>(G.m.flags, r, s, f, G.xatol, G.fatol, xr)) return 0;
  if (xc) nm_other_points<N>(s, xc);
  return 1;
}

// ... of a row whose decision waits in memory (cases, F1, pos2); f2_of(p2): the value of
// its second point
template <typename F2>
__device__ __forceinline__ int glue_update_listed_row(const NmGlue &G, int j, int &r,
                                                      F2 f2_of, int *parked,
                                                      double *xr) {
  const int N = G.m.N;
  r = G.m.list1[j];
  const int c = G.m.cases[j];
  const double fxr = G.m.F1[j];
  const int p2 = G.m.pos2[j];
  // (requested ahead of the evaluation's chain of loads)
  const double fn = G.m.fsim[(int64_t)r * (N + 1) + N];
  const double f2 = (p2 >= 0) ? f2_of(p2) : __builtin_inf();
  int go = 0;
  nm_with_N(N, [&](auto n) {
    go = glue_update_row<decltype(n)::value>(G, j, r, c, fxr, f2, fn, G.m.X2, p2, parked,
                                             xr, nullptr);
  });
  return go;
}

__global__ void __launch_bounds__(NM_UNT) nm_glue_begin_kernel(NmGlue G) {
  __shared__ int sh[NM_UNT / 64 + 1];
  const int n = nm_compact_rows<NM_UNT>(
      &G.P, G.m.N, G.m.S,
      [&](int j, int &r, double *xr) {
        r = j;
        return glue_begin_row(G, j, xr);
      },
      G.m.list1, G.m.X1, nullptr, sh);
  if (threadIdx.x == 0) {
    G.m.counts[0] = n;
    G.m.counts[3] = n;
  }
}

// (a row's own evaluation is read from job slot j: the slots this kernel rewrites for
// the second evaluation lie at or before the rows already read)
__global__ void __launch_bounds__(NM_NT) nm_glue_decide_kernel(NmGlue G, int jbound) {
  __shared__ int sh[NM_NT / 64 + 1];
  const int J = min(G.m.counts[0], jbound);
  const int n = nm_compact_rows<NM_NT>(
      &G.P, G.m.N, J,
      [&](int j, int &r, double *x2) { return glue_decide_row(G, j, r, x2); },
      G.m.list2, G.m.X2, G.m.pos2, sh);
  if (threadIdx.x == 0) G.m.counts[1] = n;
}

__global__ void __launch_bounds__(NM_UNT) nm_glue_update_kernel(NmGlue G, int jbound) {
  __shared__ int sh[NM_UNT / 64 + 1];
  __shared__ int parked;
  const int J = min(G.m.counts[0], jbound), J2 = min(G.m.counts[1], jbound);
  if (threadIdx.x == 0) parked = 0;
  // (all values of the second evaluation first: the rows' new slots below overwrite
  // the job tables glue_value reads -- a later trip's p2 can lie under an earlier
  // trip's packed positions)
  for (int p = threadIdx.x; p < J2; p += NM_UNT) G.m.F2[p] = glue_value(G, p);
  __syncthreads();
  const int n = nm_compact_rows<NM_UNT>(
      &G.P, G.m.N, J,
      [&](int j, int &r, double *xr) {
        return glue_update_listed_row(
            G, j, r, [&](int p2) { return G.m.F2[p2]; }, &parked, xr);
      },
      G.m.list1, G.m.X1, nullptr, sh);
  __syncthreads();
  if (threadIdx.x == 0) {
    G.m.counts[0] = n;
    G.m.counts[3] = n;
    G.m.counts[4] += parked;  // simplices waiting to shrink
  }
}

// ---------------------------------------------------------------------------
// The optimiser's LAST rounds -- a few stragglers stepping, every kernel of a round a
// latency, the chip idle -- as ONE evaluation launch and ONE bookkeeping kernel per
// round: all four points a step can ask for (reflection, expansion, outside and inside
// contraction: functions of the simplex alone) are evaluated together, rows q J + j for
// candidate q of list row j, and this kernel does what decide and update do, reading
// the one second value scipy would have computed.  Same points, same values, same
// updates, nfev counted as scipy counts: the state is the two-launch round's to the
// bit; the status bits of candidates scipy would not have evaluated are not taken.
// One wave (512 VGPRs: a simplex, its next point and the three other candidates in
// registers at any N): the host sends rounds of at most NM_SNT rows here (option
// nm_spec_max).
// ---------------------------------------------------------------------------
#define NM_SNT 64

// rows (q + 1) * J + pos of X1 and of the job tables <- candidate q of simplex r
__device__ __forceinline__ void nm_put_candidates(const NmGlue &G, int J, int pos, int r,
                                                  const double (*xc)[NM_MAXN]) {
  const int N = G.m.N;
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const int row = (q + 1) * J + pos;
    nm_put_row(G.m.X1 + (int64_t)row * N, xc[q], N);
    map_row_regs(G.P, row, r, xc[q]);
  }
}

__global__ void __launch_bounds__(NM_SNT) nm_glue_spec_prep_kernel(NmGlue G, int jbound) {
  const int J = min(G.m.counts[0], jbound);
  const int j = threadIdx.x;
  if (j < J)
    nm_with_N(G.m.N, [&](auto n) {
      constexpr int N = decltype(n)::value;
      const int r = G.m.list1[j];
      double s[N + 1][N], f[N + 1];
      nm_load_regs<N>(G.m.sim + (int64_t)r * (N + 1) * N, G.m.fsim + (int64_t)r * (N + 1),
                      s, f);
      double xc[3][NM_MAXN] = {};
      nm_other_points<N>(s, xc);
      nm_put_candidates(G, J, j, r, xc);
    });
  if (threadIdx.x == 0) G.m.counts[5] = 4 * J;
}

__global__ void __launch_bounds__(NM_SNT) nm_glue_spec_kernel(NmGlue G, int jbound) {
  __shared__ int sh[NM_SNT / 64 + 1];
  __shared__ int parked;
  if (threadIdx.x == 0) parked = 0;
  __syncthreads();
  const int J = min(G.m.counts[0], jbound);
  const int j = threadIdx.x;
  int go = 0, r = 0;
  double xr[NM_MAXN] = {};
  double xc[3][NM_MAXN] = {};
  if (j < J) {
    r = G.m.list1[j];
    double fxr, fn;
    const int c = glue_case_row(G, j, r, fxr, fn);
    // the step's second point: candidate c of this row, or none
    const int p2 = (c == 0) ? -1 : c * J + j;
    const double f2 = (p2 >= 0) ? glue_value(G, p2) : __builtin_inf();
    nm_with_N(G.m.N, [&](auto n) {
      go = glue_update_row<decltype(n)::value>(G, j, r, c, fxr, f2, fn, G.m.X1, p2,
                                               &parked, xr, xc);
    });
  }
  // (every row and value of this round has been read: the barriers of the scan)
  int tot;
  const int pos = block_excl_scan<NM_SNT>(go, &tot, sh);
  if (go) {
    G.m.list1[pos] = r;
    nm_put_row(G.m.X1 + (int64_t)pos * G.m.N, xr, G.m.N);
    map_row_regs(G.P, pos, r, xr);
    nm_put_candidates(G, tot, pos, r, xc);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    G.m.counts[0] = tot;
    G.m.counts[3] = tot;
    G.m.counts[5] = 4 * tot;
    G.m.counts[4] += parked;  // simplices waiting to shrink
  }
}

// ---------------------------------------------------------------------------
// The one-block bookkeeping kernels as TWO kernels each, for rounds of thousands of
// rows: everything a row does for itself -- the value of its evaluation, its case,
// the simplex update and ordering, the next round's test and point -- on as many
// blocks as there are rows (`rows`), and the ordered compaction (lists in simplex
// order, in place, as the one-block kernels leave them) behind it on one block that
// only moves rows (`pack`).  At 5000 rows the one-block kernels take 160 and 75 us --
// a fifth of a half's timeline, hidden only while the other half's objective kernel
// runs.  Same operations per row, same order of the lists: the same state.  A row's
// point waits in ITS OWN row of X1 / X2 (no other row reads that one) and its flag in
// cases[] (non-zero: the row goes on).
// ---------------------------------------------------------------------------
#define NM_ROWS_NT 256

// the rows as the rows kernel left them, compacted: row j of `list_in` (null: j itself)
// goes on when cases[j] is set, its point read back from row j of X
__device__ __forceinline__ int glue_pack_rows(const NmGlue &G, int J,
                                              const int32_t *list_in, int32_t *list_out,
                                              double *X, int32_t *pos_out, int *sh) {
  const int N = G.m.N;
  return nm_compact_rows<NM_NT>(
      &G.P, N, J,
      [&](int j, int &r, double *x) {
        const int go = G.m.cases[j] != 0;
        r = list_in ? list_in[j] : j;
        if (go) nm_get_row(x, X + (int64_t)j * N, N);
        // (a trip's rows are in registers before any thread writes a packed position)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        return go;
      },
      list_out, X, pos_out, sh);
}

// (the start of a run and every return from a shrink test all S simplices: ten trips
// of one block at 5000)
__global__ void __launch_bounds__(NM_ROWS_NT) nm_glue_begin_rows_kernel(NmGlue G) {
  const int r = blockIdx.x * NM_ROWS_NT + threadIdx.x;
  if (r >= G.m.S) return;
  double xr[NM_MAXN] = {};
  const int go = glue_begin_row(G, r, xr);
  G.m.cases[r] = go;   // (no round is in flight: the array is free)
  if (go) nm_put_row(G.m.X1 + (int64_t)r * G.m.N, xr, G.m.N);
}

__global__ void __launch_bounds__(NM_NT) nm_glue_begin_pack_kernel(NmGlue G) {
  __shared__ int sh[NM_NT / 64 + 1];
  const int n = glue_pack_rows(G, G.m.S, nullptr, G.m.list1, G.m.X1, nullptr, sh);
  __syncthreads();
  if (threadIdx.x == 0) {
    G.m.counts[0] = n;
    G.m.counts[3] = n;
  }
}

__global__ void __launch_bounds__(NM_ROWS_NT)
    nm_glue_decide_rows_kernel(NmGlue G, int jbound) {
  const int J = min(G.m.counts[0], jbound);
  const int j = blockIdx.x * NM_ROWS_NT + threadIdx.x;
  if (j >= J) return;
  int r;
  double x2[NM_MAXN] = {};
  if (glue_decide_row(G, j, r, x2)) nm_put_row(G.m.X2 + (int64_t)j * G.m.N, x2, G.m.N);
}

__global__ void __launch_bounds__(NM_NT) nm_glue_decide_pack_kernel(NmGlue G, int jbound) {
  __shared__ int sh[NM_NT / 64 + 1];
  const int J = min(G.m.counts[0], jbound);
  const int n = glue_pack_rows(G, J, G.m.list1, G.m.list2, G.m.X2, G.m.pos2, sh);
  if (threadIdx.x == 0) G.m.counts[1] = n;
}

__global__ void __launch_bounds__(NM_ROWS_NT)
    nm_glue_update_rows_kernel(NmGlue G, int jbound) {
  const int J = min(G.m.counts[0], jbound);
  const int j = blockIdx.x * NM_ROWS_NT + threadIdx.x;
  if (j >= J) return;
  int r;
  double xr[NM_MAXN];
  const int go = glue_update_listed_row(
      G, j, r,
      [&](int p2) {   // (this row's second point: nobody else's)
        const double f2 = glue_value(G, p2);
        G.m.F2[p2] = f2;
        return f2;
      },
      &G.m.counts[4], xr);
  G.m.cases[j] = go;   // (the case is used up: the flag of the pack kernel)
  if (go) nm_put_row(G.m.X1 + (int64_t)j * G.m.N, xr, G.m.N);
}

__global__ void __launch_bounds__(NM_NT) nm_glue_update_pack_kernel(NmGlue G, int jbound) {
  __shared__ int sh[NM_NT / 64 + 1];
  const int J = min(G.m.counts[0], jbound);
  const int n = glue_pack_rows(G, J, G.m.list1, G.m.list1, G.m.X1, nullptr, sh);
  __syncthreads();
  if (threadIdx.x == 0) {
    G.m.counts[0] = n;
    G.m.counts[3] = n;
  }
}

extern "C" int rvs_nm_run(const rvs_nm_state *m, const rvs_nm_objective *o,
                          double xatol, double fatol, int maxiter,
                          int sync_every, int64_t *stats, void *stream) {
  if (!m || !o || m->S < 1 || m->N < 1 || m->N > NM_MAXN || sync_every < 1)
    return RVS_E_ARG;
  hipStream_t st = rvs_stream(stream);
  const int S = m->S, N = m->N;
  int64_t rounds = 0, calls = 0, jobs = 0;
  int32_t c[8];
  NmGlue G;
  G.m = *m;
  G.P = map_params(o);
  G.badchi = o->badchi, G.xatol = xatol, G.fatol = fatol, G.maxiter = maxiter;
  G.pen_scale = o->arms[0].pt.pen_scale;
  G.spec_status = o->status;
  G.AO = obj_arm_out(o->scratch, o->narm, S);
  auto begin = [&]() {   // every simplex tested, the live ones listed and mapped
    if (S >= rvs_opt(RVS_OPT_NM_SPLIT_MIN)) {
      hipLaunchKernelGGL(nm_glue_begin_rows_kernel,
                         dim3((S + NM_ROWS_NT - 1) / NM_ROWS_NT), dim3(NM_ROWS_NT), 0, st,
                         G);
      hipLaunchKernelGGL(nm_glue_begin_pack_kernel, dim3(1), dim3(NM_NT), 0, st, G);
    } else {
      hipLaunchKernelGGL(nm_glue_begin_kernel, dim3(1), dim3(NM_UNT), 0, st, G);
    }
  };
  // the rows the last bookkeeping kernel mapped: their per-arm results stay in o->scratch
  auto evaluate = [&](int J, const int32_t *live) {
    return nm_objective_rows(o, J, live, 1 | RVS_OBJ_NO_SUM, nullptr, nullptr, st);
  };
  begin();
  RVS_LAUNCH_CHECK();
  int rc = 0;
  while (true) {
    if (hipMemcpyAsync(c, m->counts, sizeof(c), hipMemcpyDeviceToHost, st) !=
            hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return RVS_E_LAUNCH;
    const int live = c[0], parked = c[4];
    if (parked > 0) {  // scipy's shrink step for the parked simplices
      rc = rvs_nm_collect(S, m->flags, m->list3, m->counts, st);
      if (rc) return rc;
      for (int k = 1; k <= N; k++) {
        rc = rvs_nm_shrink_point(N, k, m->sim, m->list3, m->X2, m->counts,
                                 parked, st);
        if (rc) return rc;
        rc = rvs_internal_nm_eval(o, m->list3, m->X2, parked, m->counts, 2, m->F2, st);
        if (rc) return rc;
        calls++;
        jobs += parked;
        rc = rvs_nm_shrink_store(N, k, m->sim, m->fsim, m->nit, m->nfev,
                                 m->flags, m->list3, m->F2, m->counts, parked,
                                 st);
        if (rc) return rc;
      }
      begin();
      RVS_LAUNCH_CHECK();
      continue;
    }
    if (live == 0) break;
    // the live count only falls between two looks (finished and parked
    // simplices leave the list), so it bounds the launches of the window
    const int jb = live;
    // (the host looks -- a copy of the counters and a stream synchronisation, then the
    // next launches: ~25 us with nothing queued -- every sync_every rounds while the
    // launch bound matters, and less often in the latency-bound last rounds, where a
    // block behind the live count costs nothing.  A simplex's path does not depend on
    // when the host looks)
    const int window = (jb <= 256) ? max(sync_every, rvs_opt(RVS_OPT_NM_TAIL_WINDOW))
                                   : sync_every;
    // a handful of stragglers: the step's four candidate points in one launch and one
    // bookkeeping kernel per round (nm_glue_spec_kernel)
    if (jb <= rvs_opt(RVS_OPT_NM_SPEC_MAX) && jb <= NM_SNT && 4 * (int64_t)jb <= S) {
      G.AO = obj_arm_out(o->scratch, o->narm, 4 * jb);
      hipLaunchKernelGGL(nm_glue_spec_prep_kernel, dim3(1), dim3(NM_SNT), 0, st, G, jb);
      RVS_LAUNCH_CHECK();
      for (int r = 0; r < window; r++) {
        rc = evaluate(4 * jb, m->counts + 5);
        if (rc) return rc;
        hipLaunchKernelGGL(nm_glue_spec_kernel, dim3(1), dim3(NM_SNT), 0, st, G, jb);
        RVS_LAUNCH_CHECK();
        calls += 1;
        jobs += 4 * (int64_t)jb;
      }
      rounds += window;
      continue;
    }
    G.AO = obj_arm_out(o->scratch, o->narm, jb);
    for (int r = 0; r < window; r++) {
      // (from a few thousand rows up the bookkeeping is row-parallel + pack)
      const bool split = jb >= rvs_opt(RVS_OPT_NM_SPLIT_MIN);
      const dim3 rgrid((jb + NM_ROWS_NT - 1) / NM_ROWS_NT);
      rc = evaluate(jb, m->counts);
      if (rc) return rc;
      if (split) {
        hipLaunchKernelGGL(nm_glue_decide_rows_kernel, rgrid, dim3(NM_ROWS_NT), 0, st,
                           G, jb);
        hipLaunchKernelGGL(nm_glue_decide_pack_kernel, dim3(1), dim3(NM_NT), 0, st, G,
                           jb);
      } else {
        hipLaunchKernelGGL(nm_glue_decide_kernel, dim3(1), dim3(NM_NT), 0, st, G, jb);
      }
      RVS_LAUNCH_CHECK();
      rc = evaluate(jb, m->counts + 1);
      if (rc) return rc;
      if (split) {
        hipLaunchKernelGGL(nm_glue_update_rows_kernel, rgrid, dim3(NM_ROWS_NT), 0, st,
                           G, jb);
        hipLaunchKernelGGL(nm_glue_update_pack_kernel, dim3(1), dim3(NM_NT), 0, st, G,
                           jb);
      } else {
        hipLaunchKernelGGL(nm_glue_update_kernel, dim3(1), dim3(NM_UNT), 0, st, G, jb);
      }
      RVS_LAUNCH_CHECK();
      calls += 2;
      jobs += 2 * (int64_t)jb;
    }
    rounds += window;
  }
  if (stats) {
    stats[0] = rounds;
    stats[1] = calls;
    stats[2] = jobs;
  }
  return 0;
}
