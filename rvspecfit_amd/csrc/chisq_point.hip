// chisq_point.hip -- the continuum-marginalised chi^2 at ONE velocity per job (the
// optimiser's objective), its gradient and its Fisher matrix, with and
// without banded resolution matrices, for gfx950.  The velocity-grid, full and
// continuum forms of the same chi^2 are in chisq.hip.
//
// Reference: py/rvspecfit/spec_fit.py:203-354 (get_chisq0), :797-989 (get_chisq),
// py/rvspecfit/vel_fit.py:205-254, src/spliner.c:71-108 (evaler).
#include "common.h"

// packed lower-triangular index
#define TRI(i, j) ((i) * ((i) + 1) / 2 + (j))

#define GRAD_MAXTAN 6   // the parameters of a regular-grid library (MAXDIM)

// the basis sizes the point kernels are instantiated for, for a switch over npoly
#define POINT_ALL_CASES                                                   \
  RVS_CASE(1) RVS_CASE(2) RVS_CASE(3) RVS_CASE(4) RVS_CASE(5) RVS_CASE(6) \
  RVS_CASE(7) RVS_CASE(8) RVS_CASE(9) RVS_CASE(10) RVS_CASE(11)           \
  RVS_CASE(12) RVS_CASE(13) RVS_CASE(14) RVS_CASE(15) RVS_CASE(16)

// ---------------------------------------------------------------------------
// A11 at ONE velocity per job (the optimiser's objective, vel_fit.py:205-254):
// one 256-thread BLOCK per (job, arm) -- job = (spectrum idx, own template, own
// velocity) -- threads = pixels, all arms in one launch (grid.y).  Every global
// read is coalesced (spectrum row, basis rows, spline records of neighbouring
// pixels); the P(P+1)/2 + P normal-equation sums are kept per lane, folded
// across each wave with 64-lane butterflies and across the four waves through
// LDS in a fixed order (the velocity-grid kernel needs no reduction because a
// lane owns a velocity; with ONE velocity it would run 1 lane of 64).  Wave 0
// factors the P x P matrix, and a second pass over the pixels forms the
// residual norm ||D - a.ST||^2 explicitly (spec_fit.py:249): no D.D - y.y
// cancellation, so the value can be finite-differenced at any S/N.
// ---------------------------------------------------------------------------
struct PointArms {
  rvs_point_arm a[RVS_MAX_ARMS];
  int n;
};

// the grid of spectrum s on an arm: wavelengths, pixel knot coordinates, basis,
// and the base of the per-spectrum blocks of the rvs_chisq_prepare buffer
struct ArmGrid {
  const double *lam, *pix, *polysT, *wbase;
};
__device__ __forceinline__ ArmGrid arm_grid(const rvs_point_arm &T, int s) {
  ArmGrid g;
  const int G = T.G > 1 ? T.G : 1;
  const int64_t gi = (T.G > 1 && T.grid_id) ? T.grid_id[s] : 0;
  g.lam = T.lam + gi * T.npix;
  g.pix = T.work + gi * T.npix;
  g.polysT = T.polysT + gi * T.polys_stride;
  g.wbase = T.work + (int64_t)G * T.npix;   // {1/e^2, s/e^2} [S, npix], then scal [S, 2]
  return g;
}

// ---- steps every point kernel states the same way ---------------------------
// the cubic of a spline record at offset dl into it, and its derivative
__device__ __forceinline__ double cubic(const double4 &c, double dl) {
  return fma(fma(fma(c.w, dl, c.z), dl, c.y), dl, c.x);
}
__device__ __forceinline__ double cubic_deriv(const double4 &c, double dl) {
  return fma(dl, fma(3.0 * c.w, dl, 2.0 * c.z), c.y);
}
// 1 / e of a pixel with the systematic floor in quadrature (sys2 = espec_sys^2)
__device__ __forceinline__ double inv_err(double e, double espec_sys, double sys2) {
  if (espec_sys > 0) e = sqrt(sys2 + e * e);
  return 1.0 / e;
}
// the four waves' partial sums of slot i, added in order
template <int LD>
__device__ __forceinline__ double fold_get(const double (&red)[4][LD], int i) {
  return ((red[0][i] + red[1][i]) + red[2][i]) + red[3][i];
}

// knot lookup: the record of pixel k (returned) and the offset dl into it
__device__ __forceinline__ int point_knot(const rvs_point_arm &T, const ArmGrid &AG, int k,
                                          double f, double shift, double x0,
                                          double lin_inv_step, double &dl) {
  const double x = AG.lam[k] * f;
  int pos = T.log_step ? (int)(AG.pix[k] + shift)
                       : (int)((x - x0) * lin_inv_step);
  pos = min(max(pos, 0), T.ntp - 2);
  dl = x - T.knots[pos];
  return pos;
}

__device__ __forceinline__ double point_tv(const rvs_point_arm &T, const ArmGrid &AG,
                                           const double4 *cf, int k, double f,
                                           double shift, double x0,
                                           double lin_inv_step) {
  double dl;
  const int pos = point_knot(T, AG, k, f, shift, x0, lin_inv_step, dl);
  if (T.fast_interp) {
    // templ_spec[np.searchsorted(templ_lam, x)] (spec_fit.py:913-918): the
    // first knot >= x; form-1 records carry y_i in .x (also the last row)
    const int idx = min(pos + (dl > 0 ? 1 : 0), T.ntp - 1);
    return cf[idx].x;
  }
  const double4 c = cf[pos];
  return cubic(c, dl);
}

// gradient write: thread i < K adds tangent i's four wave sums (red[.][1 + i])
template <int LD>
__device__ __forceinline__ void point_grad_write(const double (&red)[4][LD], int K,
                                                 double chi, double *g) {
  if (threadIdx.x < K) {
    const int i = threadIdx.x;
    const double v = fold_get(red, 1 + i);
    g[i] = (chi == chi) ? v : __builtin_nan("");
  }
}

// Fisher tail: the folded sums of tangent i to bsh[i] (B_.i) and gsh[i] (G_i,i+d) ...
template <int P, int LD>
__device__ __forceinline__ void point_fisher_keep(
    const double (&red)[4][LD], int i, int K, double (&bsh)[1 + GRAD_MAXTAN][P],
    double (&gsh)[1 + GRAD_MAXTAN][1 + GRAD_MAXTAN]) {
  if (threadIdx.x < P + 1 + GRAD_MAXTAN) {
    const int q = threadIdx.x;
    const double v = fold_get(red, q);
    if (q < P)
      bsh[i][q] = v;
    else if (i + q - P < K)
      gsh[i][i + q - P] = v;
  }
}
// ... and F = G - B^T B, formed once and stored to both halves of fo[K][K]
template <int P>
__device__ __forceinline__ void point_fisher_write(
    const double (&bsh)[1 + GRAD_MAXTAN][P],
    const double (&gsh)[1 + GRAD_MAXTAN][1 + GRAD_MAXTAN], int K, double chi, double *fo) {
  constexpr int KM = 1 + GRAD_MAXTAN;
  if (threadIdx.x < KM * KM) {
    const int i = threadIdx.x / KM, l = threadIdx.x % KM;
    if (i <= l && l < K) {
      double bb2 = 0;
#pragma unroll
      for (int p = 0; p < P; p++) bb2 = fma(bsh[i][p], bsh[l][p], bb2);
      const double v = (chi == chi) ? gsh[i][l] - bb2 : __builtin_nan("");
      fo[i * K + l] = v;
      fo[l * K + i] = v;
    }
  }
}

// ---- job prologue: the scalars of block (job, arm) that every step below names.
// KROWS: the spline-record rows per template (1, or 1 + ntan with tangents)
#define POINT_JOB(KROWS)                                                          \
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;                        \
  const int j = blockIdx.x;                                                       \
  const rvs_point_arm &T = A.a[blockIdx.y];                                       \
  const int s = job_spec ? job_spec[j] : j;                                       \
  const int t = job_templ ? job_templ[j] : j;                                     \
  const ArmGrid AG = arm_grid(T, s);                                              \
  const double bb = vel[j] / RVS_C_KMS;                                           \
  const double f = sqrt((1.0 - bb) / (1.0 + bb));                                 \
  /* dx/dvel = lam * df/dvel,  d ln f / d beta = -1 / (1 - beta^2) */             \
  [[maybe_unused]] const double dfdv = -f / (RVS_C_KMS * (1.0 - bb * bb));        \
  const double espec_sys = T.espec_sys;                                           \
  const double sys2 = espec_sys * espec_sys;                                      \
  const int npix = T.npix;                                                        \
  const double *sp = T.spec + (int64_t)s * npix;                                  \
  const double *es = T.espec + (int64_t)s * npix;                                 \
  const double4 *cf = reinterpret_cast<const double4 *>(T.coef) +                 \
                      (int64_t)t * (KROWS) * T.ntp;                               \
  const double x0 = T.knots[0], xlast = T.knots[T.ntp - 1];                       \
  const double shift = T.log_step ? log(f) / log(T.knots[1] / x0) : 0.0;          \
  const double lin_inv_step = T.log_step ? 0.0 : 1.0 / (T.knots[1] - x0);

// ---- normal equations: pixel k with model value tv into A (acc) and v (av)
#define POINT_NORMAL_ADD(k, tv)                                                   \
  {                                                                               \
    const double ie = inv_err(es[k], espec_sys, sys2);                            \
    const double te = (tv) * ie;                                                  \
    const double wt = te * te, u = te * (sp[k] * ie);                             \
    const double *pr = AG.polysT + (int64_t)(k) * P;                              \
    double pv[P], pw[P];                                                          \
    _Pragma("unroll") for (int i = 0; i < P; i++) {                               \
      pv[i] = pr[i];                                                              \
      pw[i] = pv[i] * wt;                                                         \
    }                                                                             \
    _Pragma("unroll") for (int i = 0; i < P; i++) {                               \
      av[i] = fma(pv[i], u, av[i]);                                               \
      _Pragma("unroll") for (int jj = 0; jj <= i; jj++)                           \
        acc[TRI(i, jj)] = fma(pv[i], pw[jj], acc[TRI(i, jj)]);                    \
    }                                                                             \
  }

// ---- fold: lane 63 of each wave leaves the wave's total of a per-lane sum in its row of
// red (ONE: slot I; the other: v[0..N) to OFF + .); behind a barrier fold_get adds the
// four waves in order
#define POINT_FOLD_PUT_ONE(val, I)                                                \
  {                                                                               \
    const double v_ = wave_sum_to63(val);                                         \
    if (lane == 63) red[w][I] = v_;                                               \
  }
#define POINT_FOLD_PUT(N, v, OFF)                                                 \
  _Pragma("unroll") for (int i_ = 0; i_ < (N); i_++)                              \
    POINT_FOLD_PUT_ONE(v[i_], (OFF) + i_)

// ---- factorisation: the four waves' sums (in order) into acc and av, Cholesky
// A = L L^T in place, c = A^-1 v in av by the two substitutions, 1 / L_ii in idg,
// log det L in ldet; ok: every pivot positive
#define POINT_SOLVE()                                                             \
  {                                                                               \
    _Pragma("unroll") for (int i = 0; i < NT; i++) acc[i] = fold_get(red, i);     \
    _Pragma("unroll") for (int i = 0; i < P; i++) av[i] = fold_get(red, NT + i);  \
    _Pragma("unroll") for (int i = 0; i < P; i++) {                               \
      _Pragma("unroll") for (int jj = 0; jj <= i; jj++) {                         \
        double sum = acc[TRI(i, jj)];                                             \
        _Pragma("unroll") for (int q = 0; q < jj; q++)                            \
          sum -= acc[TRI(i, q)] * acc[TRI(jj, q)];                                \
        if (jj == i) {                                                            \
          if (!(sum > 0)) ok = false;                                             \
          const double d = sqrt(sum);                                             \
          acc[TRI(i, i)] = d;                                                     \
          idg[i] = 1.0 / d;                                                       \
          ldet += log(d);                                                         \
        } else {                                                                  \
          acc[TRI(i, jj)] = sum / acc[TRI(jj, jj)];                               \
        }                                                                         \
      }                                                                           \
    }                                                                             \
    _Pragma("unroll") for (int i = 0; i < P; i++) {                               \
      double sum = av[i];                                                         \
      _Pragma("unroll") for (int q = 0; q < i; q++) sum -= acc[TRI(i, q)] * av[q]; \
      av[i] = sum / acc[TRI(i, i)];                                               \
    }                                                                             \
    _Pragma("unroll") for (int i = P - 1; i >= 0; i--) {                          \
      double sum = av[i];                                                         \
      _Pragma("unroll") for (int q = i + 1; q < P; q++)                           \
        sum -= acc[TRI(q, i)] * av[q];                                            \
      av[i] = sum / acc[TRI(i, i)];                                               \
    }                                                                             \
  }

// ---- forward substitution: y = L^-1 phi of the basis row pr, with m = c.phi and
// q = |y|^2 = phi^T A^-1 phi; lmat(p, qq) reads L, idg holds 1 / L_pp
#define POINT_FORWARD()                                                           \
  _Pragma("unroll") for (int i_ = 0; i_ < P; i_++) {                              \
    const double ph = pr[i_];                                                     \
    m = fma(av[i_], ph, m);                                                       \
    double sum = ph;                                                              \
    _Pragma("unroll") for (int qq = 0; qq < i_; qq++)                             \
      sum = fma(-lmat(i_, qq), y[qq], sum);                                       \
    y[i_] = sum * idg[i_];                                                        \
    q = fma(y[i_], y[i_], q);                                                     \
  }

// ---- value and status tail: declares chi, the chi^2 of the (job, arm) from log det L
// (LDET), the spectrum's sum log e and the folded residual norm, and st, its RVS_ST_*
// bits; NaN off the template or where the factorisation failed (!OK)
#define POINT_VALUE(LDET, OK)                                                     \
  const double xa = AG.lam[0] * f, xb = AG.lam[npix - 1] * f;                     \
  const bool range = xa < x0 || xb < x0 || xa >= xlast || xb >= xlast;            \
  rr = fold_get(red, 0);                                                          \
  const double lz = AG.wbase[2ll * T.S * npix + 2 * s];                           \
  double chi = 2.0 * (LDET) + 2.0 * lz + rr;                                      \
  int st = 0;                                                                     \
  if (range) {                                                                    \
    st |= RVS_ST_SPLINE_RANGE;                                                    \
    chi = __builtin_nan("");                                                      \
  }                                                                               \
  if (!(OK)) st |= RVS_ST_CHOL_FALLBACK;                                          \
  if (!(OK) || !(fabs(chi) <= 1.79e308)) {                                        \
    st |= RVS_ST_NONFINITE;                                                       \
    chi = __builtin_nan("");                                                      \
  }

// ---- the per-lane normal-equation sums: A packed lower-triangular (acc) and v (av)
#define POINT_NORMAL_ZERO()                                                       \
  double acc[NT];                                                                 \
  double av[P];                                                                   \
  _Pragma("unroll") for (int i = 0; i < NT; i++) acc[i] = 0;                      \
  _Pragma("unroll") for (int i = 0; i < P; i++) av[i] = 0;

// ---- where L is read from: with the Fisher pass at P = 16 (under resolution matrices
// also without it, the band's accumulators being live beside L in pass 2), L, the job's
// scalars and the sums of a tangent do not all fit a lane's registers: the rows of L from
// PL on then live in LDS, every lane reading the same address (the same numbers, so pass
// 2 gives the same bits).  PL is the caller's constant (the *_LROWS_P16 below, or P)
#define POINT_LROWS()                                                             \
  __shared__ double lsh[PL < P ? NT : 1];                                         \
  if constexpr (PL < P) {                                                         \
    if (threadIdx.x == 0) {                                                       \
      _Pragma("unroll") for (int q = TRI(PL, 0); q < NT; q++) lsh[q] = acc[q];    \
    }                                                                             \
    __syncthreads();                                                              \
  }                                                                               \
  auto lmat = [&](int p, int qq) {                                                \
    return p < PL ? acc[TRI(p, qq)] : lsh[TRI(p, qq)];                            \
  };

template <int P>
__global__ void __launch_bounds__(256)
    point_block_kernel(PointArms A, const int32_t *__restrict__ job_spec,
                       const int32_t *__restrict__ job_templ, int J,
                       const double *__restrict__ vel,
                       double *__restrict__ armchi,
                       int32_t *__restrict__ armst) {
  constexpr int NT = P * (P + 1) / 2;
  constexpr int NV = NT + P;
  __shared__ double red[4][NV + 1];
  __shared__ double coefs[P + 2];
  extern __shared__ double rawsh[];  // [npix] only with a resolution matrix
  POINT_JOB(1)
  // A9: banded resolution matrix on the resampled template (spec_fit.py:920-929)
  const double *tp = T.taps ? T.taps + (int64_t)s * T.taps_stride : nullptr;
  const int nd = T.nd, mres = (T.nd - 1) / 2;
  if (tp) {
    for (int k = threadIdx.x; k < npix; k += 256)
      rawsh[k] = point_tv(T, AG, cf, k, f, shift, x0, lin_inv_step);
    __syncthreads();
  }
  auto tv_at = [&](int k) {
    if (!tp) return point_tv(T, AG, cf, k, f, shift, x0, lin_inv_step);
    double v = 0;
    for (int d = 0; d < nd; d++) {
      const int q = k - mres + d;
      if (q >= 0 && q < npix) v = fma(tp[(int64_t)k * nd + d], rawsh[q], v);
    }
    return v;
  };
  POINT_NORMAL_ZERO()
  for (int k = threadIdx.x; k < npix; k += 256) {
    const double tv = tv_at(k);
    POINT_NORMAL_ADD(k, tv)
  }
  POINT_FOLD_PUT(NT, acc, 0)
  POINT_FOLD_PUT(P, av, NT)
  __syncthreads();
  if (w == 0) {
    // every lane of wave 0 factors the same matrix (waves summed in order)
    bool ok = true;
    double ldet = 0;
    double idg[P];   // (1 / L_ii: not used here)
    POINT_SOLVE()
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < P; i++) coefs[i] = av[i];
      coefs[P] = ldet;
      coefs[P + 1] = ok ? 1.0 : 0.0;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < P; i++) av[i] = coefs[i];
  double rr = 0;
  for (int k = threadIdx.x; k < npix; k += 256) {
    const double tv = tv_at(k);
    const double ie = inv_err(es[k], espec_sys, sys2);
    const double *pr = AG.polysT + (int64_t)k * P;
    double m = 0;
#pragma unroll
    for (int i = 0; i < P; i++) m = fma(av[i], pr[i], m);
    const double r = sp[k] * ie - m * (tv * ie);
    rr = fma(r, r, rr);
  }
  rr = wave_sum(rr);
  __syncthreads();
  if (lane == 0) red[w][0] = rr;
  __syncthreads();
  if (threadIdx.x == 0) {
    POINT_VALUE(coefs[P], coefs[P + 1] != 0.0)
    armchi[(int64_t)blockIdx.y * J + j] = chi;
    armst[(int64_t)blockIdx.y * J + j] = st;
  }
}

// arms summed in order; penalties of A11 (spec_fit.py:888-896)
__global__ void point_sum_kernel(PointArms A, int J, double badchi,
                                 const int32_t *__restrict__ job_spec,
                                 const double *__restrict__ armchi,
                                 const int32_t *__restrict__ armst,
                                 double *__restrict__ out,
                                 int32_t *__restrict__ status) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= J) return;
  if (A.a[0].pen_scale) badchi *= A.a[0].pen_scale[job_spec ? job_spec[j] : j];
  double tot = 0;
  int st = 0;
  for (int ia = 0; ia < A.n; ia++) {
    const double *pp = A.a[ia].penalty;
    const double pen = pp ? pp[j] : 0.0;
    if (!(pen == pen) || isinf(pen)) {
      tot += 1000.0 * badchi;
      continue;
    }
    tot += armchi[(int64_t)ia * J + j] + pen;
    st |= armst[(int64_t)ia * J + j];
  }
  out[j] = tot;
  if (st) atomicOr(&status[j], st);
}

extern "C" int64_t rvs_chisq_point_work_size(int J, int narm) {
  if (J < 1 || narm < 1) return 0;
  return (int64_t)narm * J * (int64_t)(sizeof(double) + sizeof(int32_t));
}

extern "C" int rvs_chisq_point(const rvs_point_arm *arms, int narm, int npoly,
                               const int32_t *job_spec,
                               const int32_t *job_templ, int J,
                               const double *vel, double badchi, void *scratch,
                               double *out, int32_t *status, void *stream) {
  if (J < 1 || narm < 1 || narm > RVS_MAX_ARMS || !arms || !scratch)
    return RVS_E_ARG;
  PointArms A;
  A.n = narm;
  for (int i = 0; i < narm; i++) {
    A.a[i] = arms[i];
    if (arms[i].npix < 1 || arms[i].ntp < 3) return RVS_E_ARG;
  }
  for (int i = narm; i < RVS_MAX_ARMS; i++) A.a[i] = arms[0];
  hipStream_t st = rvs_stream(stream);
  double *armchi = (double *)scratch;
  int32_t *armst = (int32_t *)(armchi + (int64_t)narm * J);
  dim3 grid(J, narm);
  size_t shm = 0;
  for (int i = 0; i < narm; i++)
    if (arms[i].taps) {
      if (arms[i].nd < 1 || (arms[i].nd & 1) == 0) return RVS_E_ARG;
      shm = max(shm, (size_t)arms[i].npix * sizeof(double));
    }
  if (shm > 60 * 1024) return RVS_E_ARG;
#define RVS_CASE(PP)                                                           \
  case PP:                                                                     \
    hipLaunchKernelGGL(point_block_kernel<PP>, grid, dim3(256), shm, st, A,    \
                       job_spec, job_templ, J, vel, armchi, armst);            \
    break;
  switch (npoly) {
    POINT_ALL_CASES
    default:
      return RVS_E_ARG;
  }
#undef RVS_CASE
  hipLaunchKernelGGL(point_sum_kernel, dim3((J + 255) / 256), dim3(256), 0, st,
                     A, J, badchi, job_spec, armchi, armst, out, status);
  RVS_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// The same objective with its gradient (include/rvsgpu.h, rvs_chisq_point_grad).
// Layout as point_block_kernel: one 256-thread block per (job, arm), threads =
// pixels.  Pass 1 accumulates A and v (P(P+1)/2 + P sums per lane, folded per wave
// by DPP and across the four waves through LDS in a fixed order); EVERY wave then
// factors the same matrix, so that the Cholesky factor sits in the registers of
// all 256 lanes for pass 2.  Pass 2 forms per pixel the residual r, s = c.phi and
// q = |L^-1 phi|^2 = phi^T A^-1 phi, i.e. the adjoint of the model value
//     mbar = 2 (m/e^2) q - 2 r s / e
// and accumulates |r|^2 and the 1 + NTAN products mbar * m'_k.  That is
// tr(A^-1 A'_k) + c^T A'_k c - 2 c.v'_k without ever forming A'_k and v'_k: the
// (P(P+1)/2 + P)(1 + K) sums of the tangent normal equations (1216 at P = 16, K = 7:
// more than a lane's registers or a block's LDS slots per lane hold) become 2 + K,
// and the residual enters explicitly, as in the value, instead of as a difference.
//
// The Fisher matrix of the same fit (rvs_chisq_point_fisher) is a third pass behind
// the same two, in the same block: point_grad_block<P, true>.  With J_ki = s_k m'_ki /
// e_k (s = c.phi, the fitted continuum) and the orthonormal rows U = L^-1 ST,
//     F_il = sum_k J_ki J_kl - sum_p B_pi B_pl,   B_pi = sum_k y_p(k) (m_k / e_k) J_ki,
// y = L^-1 phi the forward substitution of pass 2.  The P K + K (K + 1) / 2 sums (140
// at P = 16, K = 7) do not fit beside L in a lane's registers, so the pass loops over
// the tangents: for tangent i the P sums B_.i and the K - i sums G_il, l >= i, with y
// recomputed -- K times the multiply-adds of pass 2 on a path that runs once per
// spectrum.  Sums are folded as everywhere here (DPP per wave, the four waves in order
// through LDS); F_il is formed once and written to both halves.
// ---------------------------------------------------------------------------
// rows of L that stay in registers in point_fisher_block_kernel<16> (the others are read
// from LDS); chosen from the compiler's resource report: 14 and 12 leave scratch, 8 none
#define FISHER_LROWS_P16 8
template <int P, bool FISHER>
__device__ __forceinline__ void
    point_grad_block(const PointArms &A, int ntan,
                     const int32_t *__restrict__ job_spec,
                     const int32_t *__restrict__ job_templ, int J,
                     const double *__restrict__ vel,
                     double *__restrict__ armchi,
                     double *__restrict__ armgrad,
                     double *__restrict__ armfisher,
                     int32_t *__restrict__ armst) {
  constexpr int NT = P * (P + 1) / 2;
  constexpr int NV = NT + P;
  constexpr int KM = 1 + GRAD_MAXTAN;
  constexpr int NG = FISHER && P + KM > 1 + KM ? P + KM : 1 + KM;
  constexpr int NR = NV > NG ? NV : NG;
  __shared__ double red[4][NR + 1];
  const int K = 1 + ntan;
  POINT_JOB(K)
  POINT_NORMAL_ZERO()
  for (int k = threadIdx.x; k < npix; k += 256) {
    const double tv = point_tv(T, AG, cf, k, f, shift, x0, lin_inv_step);
    POINT_NORMAL_ADD(k, tv)
  }
  POINT_FOLD_PUT(NT, acc, 0)
  POINT_FOLD_PUT(P, av, NT)
  __syncthreads();
  // every lane of every wave factors the same matrix (waves summed in order)
  bool ok = true;
  double ldet = 0;
  double idg[P];  // 1 / L_ii
  POINT_SOLVE()
  constexpr int PL = FISHER && P > 15 ? FISHER_LROWS_P16 : P;
  POINT_LROWS()
  double rr = 0;
  double gk[1 + GRAD_MAXTAN];
#pragma unroll
  for (int i = 0; i <= GRAD_MAXTAN; i++) gk[i] = 0;
  for (int k = threadIdx.x; k < npix; k += 256) {
    // the template and its velocity tangent from one record (point_tv's index)
    double dl;
    const int pos = point_knot(T, AG, k, f, shift, x0, lin_inv_step, dl);
    const double4 c0 = cf[pos];
    const double tv = cubic(c0, dl);
    const double dtv = cubic_deriv(c0, dl);
    const double ie = inv_err(es[k], espec_sys, sys2);
    const double *pr = AG.polysT + (int64_t)k * P;
    double y[P], m = 0, q = 0;
    POINT_FORWARD()
    const double r = sp[k] * ie - m * (tv * ie);
    rr = fma(r, r, rr);
    const double mbar = 2.0 * ie * ((tv * ie) * q - r * m);
    gk[0] = fma(mbar, dtv * (AG.lam[k] * dfdv), gk[0]);
#pragma unroll
    for (int i = 1; i <= GRAD_MAXTAN; i++)
      if (i < K) {
        const double4 c = cf[(int64_t)i * T.ntp + pos];
        gk[i] = fma(mbar, cubic(c, dl), gk[i]);
      }
  }
  __syncthreads();   // (red is read above by every wave)
  POINT_FOLD_PUT_ONE(rr, 0)
  POINT_FOLD_PUT(1 + GRAD_MAXTAN, gk, 1)
  __syncthreads();
  const int64_t o = (int64_t)blockIdx.y * J + j;
  POINT_VALUE(ldet, ok)
  if (threadIdx.x == 0) {
    armchi[o] = chi;
    armst[o] = st;
  }
  point_grad_write(red, K, chi, armgrad + o * K);
  if constexpr (FISHER) {
    __shared__ double bsh[KM][P];
    __shared__ double gsh[KM][KM];
    for (int i = 0; i < K; i++) {
      double bp[P], gl[KM];   // B_.i and G_i,i+d
#pragma unroll
      for (int p = 0; p < P; p++) bp[p] = 0;
#pragma unroll
      for (int d = 0; d < KM; d++) gl[d] = 0;
      for (int k = threadIdx.x; k < npix; k += 256) {
        double dl;
        const int pos = point_knot(T, AG, k, f, shift, x0, lin_inv_step, dl);
        const double4 c0 = cf[pos];
        const double tv = cubic(c0, dl);
        const double ie = inv_err(es[k], espec_sys, sys2);
        const double *pr = AG.polysT + (int64_t)k * P;
        double y[P], m = 0;
        [[maybe_unused]] double q = 0;
        POINT_FORWARD()
        const double se = m * ie;   // J_kl = se * m'_kl
        double ti;
        if (i == 0) {
          ti = cubic_deriv(c0, dl) * (AG.lam[k] * dfdv);
        } else {
          const double4 c = cf[(int64_t)i * T.ntp + pos];
          ti = cubic(c, dl);
        }
        const double ji = se * ti;
        const double z = (tv * ie) * ji;
#pragma unroll
        for (int p = 0; p < P; p++) bp[p] = fma(y[p], z, bp[p]);
        gl[0] = fma(ji, ji, gl[0]);
#pragma unroll
        for (int d = 1; d < KM; d++)
          if (i + d < K) {
            const double4 c = cf[(int64_t)(i + d) * T.ntp + pos];
            const double tl = cubic(c, dl);
            gl[d] = fma(ji, se * tl, gl[d]);
          }
      }
      __syncthreads();   // (red: the sums of the pass before are read)
      POINT_FOLD_PUT(P, bp, 0)
      POINT_FOLD_PUT(KM, gl, P)
      __syncthreads();
      point_fisher_keep<P>(red, i, K, bsh, gsh);
    }
    __syncthreads();
    point_fisher_write<P>(bsh, gsh, K, chi, armfisher + o * K * K);
  }
}

template <int P>
__global__ void __launch_bounds__(256)
    point_grad_block_kernel(PointArms A, int ntan,
                            const int32_t *__restrict__ job_spec,
                            const int32_t *__restrict__ job_templ, int J,
                            const double *__restrict__ vel,
                            double *__restrict__ armchi,
                            double *__restrict__ armgrad,
                            int32_t *__restrict__ armst) {
  point_grad_block<P, false>(A, ntan, job_spec, job_templ, J, vel, armchi, armgrad,
                             nullptr, armst);
}

template <int P>
__global__ void __launch_bounds__(256)
    point_fisher_block_kernel(PointArms A, int ntan,
                              const int32_t *__restrict__ job_spec,
                              const int32_t *__restrict__ job_templ, int J,
                              const double *__restrict__ vel,
                              double *__restrict__ armchi,
                              double *__restrict__ armgrad,
                              double *__restrict__ armfisher,
                              int32_t *__restrict__ armst) {
  point_grad_block<P, true>(A, ntan, job_spec, job_templ, J, vel, armchi, armgrad,
                            armfisher, armst);
}

// ---------------------------------------------------------------------------
// point_grad_block under banded resolution matrices (rvs_chisq_point_grad_resol,
// rvs_chisq_point_fisher_resol): the model row is m = R raw and every tangent row
// R raw'_i, R acting after the resampling (point_block_kernel's band: m_k = sum_d
// taps[s][k][d] raw[k - (nd-1)/2 + d], d ascending, pixels outside the arm skipped).
// The pixels are walked in TILES of 256 outputs: the block stages the raw value row
// and the raw tangent rows of the pixels [k0 - mres, k0 + 256 + mres) in LDS
// ((1 + K)(256 + nd - 1) doubles, whatever npix), and after a barrier every thread
// applies the band of its own pixel to the rows it needs.  All three passes go
// through the same tiles -- pass 1 stages the value row only, pass 2 the value and
// the K tangents, the Fisher pass of tangent i the value and the tangents i ... K-1
// (it needs the products J_ki J_kl of CONVOLVED rows, which no adjoint of the band
// gives) -- so no convolved row goes to HBM and none is kept for a whole arm.  The
// tile loops have the same trip count for every thread (a thread past the last pixel
// stages and waits, and accumulates nothing), so every barrier is reached by all 256.
// The raw velocity tangent of pixel q is S'(x_q) lam_q df/dvel: lam of the RAW pixel.
// Sums, the factorisation and the status bits are point_grad_block's, in its order:
// with nd = 1 and a tap of 1 every fma(1, x, 0) is x and the results are its bits.
// An arm without taps among arms with them is such an identity band, taps not read.
// ---------------------------------------------------------------------------
// rows of L in registers in point_grad_resol_block_kernel<16> and
// point_fisher_resol_block_kernel<16> (as FISHER_LROWS_P16, from the compiler's
// resource report with the band's accumulators beside them: the gradient leaves
// scratch with 4 and 0 rows and none with 8, the Fisher form 20 B with 8, none with 4)
#define GRAD_RESOL_LROWS_P16 8
#define FISHER_RESOL_LROWS_P16 4
// (RVS_GRAD_RESOL_LDS_MAX, the most dynamic LDS of the tiles: with the static sums,
// 7.3 KB at P = 16, inside the 64 KB every launch is given)
template <int P, bool FISHER>
__device__ __forceinline__ void
    point_grad_resol_block(const PointArms &A, int ntan,
                           const int32_t *__restrict__ job_spec,
                           const int32_t *__restrict__ job_templ, int J,
                           const double *__restrict__ vel,
                           double *__restrict__ armchi,
                           double *__restrict__ armgrad,
                           double *__restrict__ armfisher,
                           int32_t *__restrict__ armst) {
  constexpr int NT = P * (P + 1) / 2;
  constexpr int NV = NT + P;
  constexpr int KM = 1 + GRAD_MAXTAN;
  constexpr int NG = FISHER && P + KM > 1 + KM ? P + KM : 1 + KM;
  constexpr int NR = NV > NG ? NV : NG;
  __shared__ double red[4][NR + 1];
  extern __shared__ double rowsh[];   // [1 + K][W]: raw rows of a tile and its halo
  const int K = 1 + ntan;
  POINT_JOB(K)
  const double *tp = T.taps ? T.taps + (int64_t)s * T.taps_stride : nullptr;
  const int nd = tp ? T.nd : 1, mres = (nd - 1) / 2;
  const int W = 256 + nd - 1;
  // the raw value row and the raw tangent rows lo <= i < hi of the tile at k0
  auto stage = [&](int k0, int lo, int hi) {
    for (int u = threadIdx.x; u < W; u += 256) {
      const int q = k0 - mres + u;
      if (q < 0 || q >= npix) continue;   // (never read: the band skips them)
      double dl;
      const int pos = point_knot(T, AG, q, f, shift, x0, lin_inv_step, dl);
      const double4 c0 = cf[pos];
      rowsh[u] = cubic(c0, dl);
      for (int i = lo; i < hi; i++) {
        if (i == 0) {
          const double dtv = cubic_deriv(c0, dl);
          rowsh[W + u] = dtv * (AG.lam[q] * dfdv);
        } else {
          const double4 c = cf[(int64_t)i * T.ntp + pos];
          rowsh[(1 + i) * W + u] = cubic(c, dl);
        }
      }
    }
  };
  // the band of pixel k (this thread's, in the staged tile) on the value row ...
  auto band_value = [&](int k) {
    double v = 0;
    for (int d = 0; d < nd; d++) {
      const int q = k - mres + d;
      if (q >= 0 && q < npix)
        v = fma(tp ? tp[(int64_t)k * nd + d] : 1.0, rowsh[threadIdx.x + d], v);
    }
    return v;
  };
  // ... and on the tangent rows lo ... K-1 at once (cv[d]: tangent lo + d)
  auto band_tangents = [&](int k, int lo, double (&cv)[KM]) {
#pragma unroll
    for (int d = 0; d < KM; d++) cv[d] = 0;
    for (int d = 0; d < nd; d++) {
      const int q = k - mres + d;
      if (q < 0 || q >= npix) continue;
      const double tap = tp ? tp[(int64_t)k * nd + d] : 1.0;
      const double *rp = rowsh + (1 + lo) * W + threadIdx.x + d;
#pragma unroll
      for (int i = 0; i < KM; i++)
        if (lo + i < K) cv[i] = fma(tap, rp[i * W], cv[i]);
    }
  };
  POINT_NORMAL_ZERO()
  for (int k0 = 0; k0 < npix; k0 += 256) {
    stage(k0, 0, 0);
    __syncthreads();
    const int k = k0 + threadIdx.x;
    if (k < npix) {
      const double tv = band_value(k);
      POINT_NORMAL_ADD(k, tv)
    }
    __syncthreads();   // (the next tile is staged over this one)
  }
  POINT_FOLD_PUT(NT, acc, 0)
  POINT_FOLD_PUT(P, av, NT)
  __syncthreads();
  // every lane of every wave factors the same matrix (waves summed in order)
  bool ok = true;
  double ldet = 0;
  double idg[P];  // 1 / L_ii
  POINT_SOLVE()
  constexpr int PL = P > 15 ? (FISHER ? FISHER_RESOL_LROWS_P16 : GRAD_RESOL_LROWS_P16) : P;
  POINT_LROWS()
  double rr = 0;
  double gk[KM];
#pragma unroll
  for (int i = 0; i < KM; i++) gk[i] = 0;
  for (int k0 = 0; k0 < npix; k0 += 256) {
    stage(k0, 0, K);
    __syncthreads();
    const int k = k0 + threadIdx.x;
    if (k < npix) {
      const double tv = band_value(k);
      const double ie = inv_err(es[k], espec_sys, sys2);
      const double *pr = AG.polysT + (int64_t)k * P;
      double y[P], m = 0, q = 0;
      POINT_FORWARD()
      const double r = sp[k] * ie - m * (tv * ie);
      rr = fma(r, r, rr);
      const double mbar = 2.0 * ie * ((tv * ie) * q - r * m);
      double cv[KM];
      band_tangents(k, 0, cv);
#pragma unroll
      for (int i = 0; i < KM; i++)
        if (i < K) gk[i] = fma(mbar, cv[i], gk[i]);
    }
    __syncthreads();
  }
  POINT_FOLD_PUT_ONE(rr, 0)
  POINT_FOLD_PUT(KM, gk, 1)
  __syncthreads();
  const int64_t o = (int64_t)blockIdx.y * J + j;
  POINT_VALUE(ldet, ok)
  if (threadIdx.x == 0) {
    armchi[o] = chi;
    armst[o] = st;
  }
  point_grad_write(red, K, chi, armgrad + o * K);
  if constexpr (FISHER) {
    __shared__ double bsh[KM][P];
    __shared__ double gsh[KM][KM];
    for (int i = 0; i < K; i++) {
      double bp[P], gl[KM];   // B_.i and G_i,i+d
#pragma unroll
      for (int p = 0; p < P; p++) bp[p] = 0;
#pragma unroll
      for (int d = 0; d < KM; d++) gl[d] = 0;
      for (int k0 = 0; k0 < npix; k0 += 256) {
        stage(k0, i, K);
        __syncthreads();
        const int k = k0 + threadIdx.x;
        if (k < npix) {
          const double tv = band_value(k);
          double cv[KM];   // the convolved tangents i, i + 1 ...
          band_tangents(k, i, cv);
          const double ie = inv_err(es[k], espec_sys, sys2);
          const double *pr = AG.polysT + (int64_t)k * P;
          double y[P], m = 0;
          [[maybe_unused]] double q = 0;
          POINT_FORWARD()
          const double se = m * ie;   // J_kl = se * m'_kl
          const double ji = se * cv[0];
          const double z = (tv * ie) * ji;
#pragma unroll
          for (int p = 0; p < P; p++) bp[p] = fma(y[p], z, bp[p]);
          gl[0] = fma(ji, ji, gl[0]);
#pragma unroll
          for (int d = 1; d < KM; d++)
            if (i + d < K) gl[d] = fma(ji, se * cv[d], gl[d]);
        }
        __syncthreads();   // (also red: the sums of the pass before are read)
      }
      POINT_FOLD_PUT(P, bp, 0)
      POINT_FOLD_PUT(KM, gl, P)
      __syncthreads();
      point_fisher_keep<P>(red, i, K, bsh, gsh);
    }
    __syncthreads();
    point_fisher_write<P>(bsh, gsh, K, chi, armfisher + o * K * K);
  }
}

template <int P>
__global__ void __launch_bounds__(256)
    point_grad_resol_block_kernel(PointArms A, int ntan,
                                  const int32_t *__restrict__ job_spec,
                                  const int32_t *__restrict__ job_templ, int J,
                                  const double *__restrict__ vel,
                                  double *__restrict__ armchi,
                                  double *__restrict__ armgrad,
                                  int32_t *__restrict__ armst) {
  point_grad_resol_block<P, false>(A, ntan, job_spec, job_templ, J, vel, armchi,
                                   armgrad, nullptr, armst);
}

template <int P>
__global__ void __launch_bounds__(256)
    point_fisher_resol_block_kernel(PointArms A, int ntan,
                                    const int32_t *__restrict__ job_spec,
                                    const int32_t *__restrict__ job_templ, int J,
                                    const double *__restrict__ vel,
                                    double *__restrict__ armchi,
                                    double *__restrict__ armgrad,
                                    double *__restrict__ armfisher,
                                    int32_t *__restrict__ armst) {
  point_grad_resol_block<P, true>(A, ntan, job_spec, job_templ, J, vel, armchi,
                                  armgrad, armfisher, armst);
}

// arms summed in order; penalties of A11 (spec_fit.py:888-896) on the value only
__global__ void point_grad_sum_kernel(PointArms A, int J, int K, double badchi,
                                      double4 bconst,
                                      const int32_t *__restrict__ job_spec,
                                      const double *__restrict__ armchi,
                                      const double *__restrict__ armgrad,
                                      const int32_t *__restrict__ armst,
                                      double *__restrict__ out,
                                      double *__restrict__ grad,
                                      int32_t *__restrict__ status) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= J) return;
  if (A.a[0].pen_scale) badchi *= A.a[0].pen_scale[job_spec ? job_spec[j] : j];
  const double bc[RVS_MAX_ARMS] = {bconst.x, bconst.y, bconst.z, bconst.w};
  double tot = 0;
  double g[1 + GRAD_MAXTAN];
#pragma unroll
  for (int i = 0; i <= GRAD_MAXTAN; i++) g[i] = 0;
  int st = 0;
#pragma unroll
  for (int ia = 0; ia < RVS_MAX_ARMS; ia++) {
    if (ia >= A.n) break;
    const double *pp = A.a[ia].penalty;
    const double pen = pp ? pp[j] : 0.0;
    if (!(pen == pen) || isinf(pen)) {
      tot += 1000.0 * badchi;
      continue;
    }
    const int64_t o = (int64_t)ia * J + j;
    tot += armchi[o] + bc[ia] + pen;
    st |= armst[o];
#pragma unroll
    for (int i = 0; i <= GRAD_MAXTAN; i++)
      if (i < K) g[i] += armgrad[o * K + i];
  }
  out[j] = tot;
#pragma unroll
  for (int i = 0; i <= GRAD_MAXTAN; i++)
    if (i < K) grad[(int64_t)j * K + i] = g[i];
  if (st) atomicOr(&status[j], st);
}

// the arms' Fisher matrices summed in order: the arms point_grad_sum_kernel skips add
// nothing; one thread per (job, entry)
__global__ void point_fisher_sum_kernel(PointArms A, int J, int K,
                                        const double *__restrict__ armfisher,
                                        double *__restrict__ fisher) {
  const int64_t KK = (int64_t)K * K;
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= J * KK) return;
  const int64_t j = idx / KK;
  double tot = 0;
#pragma unroll
  for (int ia = 0; ia < RVS_MAX_ARMS; ia++) {
    if (ia >= A.n) break;
    const double *pp = A.a[ia].penalty;
    const double pen = pp ? pp[j] : 0.0;
    if (!(pen == pen) || isinf(pen)) continue;
    tot += armfisher[(int64_t)ia * J * KK + idx];
  }
  fisher[idx] = tot;
}

// scratch of the gradient call, and of the Fisher call when `fisher`
static int64_t point_grad_work(int J, int narm, int ntan, bool fisher) {
  if (J < 1 || narm < 1 || ntan < 0 || ntan > GRAD_MAXTAN) return 0;
  const int K = 1 + ntan;
  return (int64_t)narm * J *
         (int64_t)((1 + K + (fisher ? K * K : 0)) * sizeof(double) +
                   sizeof(int32_t));
}

extern "C" int64_t rvs_chisq_point_grad_work_size(int J, int narm, int ntan) {
  return point_grad_work(J, narm, ntan, false);
}

extern "C" int64_t rvs_chisq_point_fisher_work_size(int J, int narm, int ntan) {
  return point_grad_work(J, narm, ntan, true);
}

// rvs_chisq_point_grad, and rvs_chisq_point_fisher where `fisher` is given
static int point_grad_launch(const rvs_point_arm *arms, int narm, int npoly,
                             int ntan, const int32_t *job_spec,
                             const int32_t *job_templ, int J, const double *vel,
                             double badchi, const double *basis_const,
                             void *scratch, double *out, double *grad,
                             double *fisher, int32_t *status, void *stream,
                             bool resol = false) {
  if (J < 1 || narm < 1 || narm > RVS_MAX_ARMS || !arms || !scratch ||
      ntan < 0 || ntan > GRAD_MAXTAN)
    return RVS_E_ARG;
  static_assert(RVS_MAX_ARMS == 4, "basis constants travel as a double4");
  PointArms A;
  A.n = narm;
  double bc[RVS_MAX_ARMS] = {0, 0, 0, 0};
  for (int i = 0; i < narm; i++) {
    A.a[i] = arms[i];
    if (arms[i].npix < 1 || arms[i].ntp < 3 || arms[i].G > 1 ||
        (arms[i].taps && !resol) || arms[i].fast_interp)
      return RVS_E_ARG;
    if (basis_const) bc[i] = basis_const[i];
  }
  // the tiles of point_grad_resol_block: (1 + K) rows of 256 + nd - 1 doubles
  size_t shm = 0;
  for (int i = 0; i < narm; i++)
    if (arms[i].taps) {
      if (arms[i].nd < 1 || (arms[i].nd & 1) == 0) return RVS_E_ARG;
      shm = max(shm, (size_t)RVS_GRAD_RESOL_LDS(ntan, arms[i].nd));
    }
  if (shm > RVS_GRAD_RESOL_LDS_MAX) return RVS_E_ARG;
  for (int i = narm; i < RVS_MAX_ARMS; i++) A.a[i] = arms[0];
  hipStream_t st = rvs_stream(stream);
  const int K = 1 + ntan;
  double *armchi = (double *)scratch;
  double *armgrad = armchi + (int64_t)narm * J;
  double *armfisher = armgrad + (int64_t)narm * J * K;
  int32_t *armst =
      (int32_t *)(armfisher + (fisher ? (int64_t)narm * J * K * K : 0));
  dim3 grid(J, narm);
#define RVS_CASE(PP)                                                           \
  case PP:                                                                     \
    if (shm && fisher)                                                         \
      hipLaunchKernelGGL(point_fisher_resol_block_kernel<PP>, grid, dim3(256), \
                         shm, st, A, ntan, job_spec, job_templ, J, vel,        \
                         armchi, armgrad, armfisher, armst);                   \
    else if (shm)                                                              \
      hipLaunchKernelGGL(point_grad_resol_block_kernel<PP>, grid, dim3(256),   \
                         shm, st, A, ntan, job_spec, job_templ, J, vel,        \
                         armchi, armgrad, armst);                              \
    else if (fisher)                                                           \
      hipLaunchKernelGGL(point_fisher_block_kernel<PP>, grid, dim3(256), 0,    \
                         st, A, ntan, job_spec, job_templ, J, vel, armchi,     \
                         armgrad, armfisher, armst);                           \
    else                                                                       \
      hipLaunchKernelGGL(point_grad_block_kernel<PP>, grid, dim3(256), 0, st,  \
                         A, ntan, job_spec, job_templ, J, vel, armchi,         \
                         armgrad, armst);                                      \
    break;
  switch (npoly) {
    POINT_ALL_CASES
    default:
      return RVS_E_ARG;
  }
#undef RVS_CASE
  hipLaunchKernelGGL(point_grad_sum_kernel, dim3((J + 255) / 256), dim3(256), 0,
                     st, A, J, K, badchi, make_double4(bc[0], bc[1], bc[2], bc[3]),
                     job_spec, armchi, armgrad, armst, out, grad, status);
  if (fisher) {
    const int64_t n = (int64_t)J * K * K;
    hipLaunchKernelGGL(point_fisher_sum_kernel, dim3((unsigned)((n + 255) / 256)),
                       dim3(256), 0, st, A, J, K, armfisher, fisher);
  }
  RVS_LAUNCH_CHECK();
  return 0;
}

extern "C" int rvs_chisq_point_grad(const rvs_point_arm *arms, int narm, int npoly,
                                    int ntan, const int32_t *job_spec,
                                    const int32_t *job_templ, int J,
                                    const double *vel, double badchi,
                                    const double *basis_const, void *scratch,
                                    double *out, double *grad, int32_t *status,
                                    void *stream) {
  return point_grad_launch(arms, narm, npoly, ntan, job_spec, job_templ, J, vel,
                           badchi, basis_const, scratch, out, grad, nullptr,
                           status, stream);
}

extern "C" int rvs_chisq_point_fisher(const rvs_point_arm *arms, int narm,
                                      int npoly, int ntan, const int32_t *job_spec,
                                      const int32_t *job_templ, int J,
                                      const double *vel, double badchi,
                                      const double *basis_const, void *scratch,
                                      double *out, double *grad, double *fisher,
                                      int32_t *status, void *stream) {
  if (!fisher) return RVS_E_ARG;
  return point_grad_launch(arms, narm, npoly, ntan, job_spec, job_templ, J, vel,
                           badchi, basis_const, scratch, out, grad, fisher, status,
                           stream);
}

// The same two with arms that carry a resolution matrix (point_grad_resol_block);
// a call in which no arm has one runs the kernels, and gives the bits, of the pair above
extern "C" int64_t rvs_chisq_point_grad_resol_work_size(int J, int narm, int ntan) {
  return point_grad_work(J, narm, ntan, false);
}

extern "C" int64_t rvs_chisq_point_fisher_resol_work_size(int J, int narm, int ntan) {
  return point_grad_work(J, narm, ntan, true);
}

extern "C" int rvs_chisq_point_grad_resol(
    const rvs_point_arm *arms, int narm, int npoly, int ntan, const int32_t *job_spec,
    const int32_t *job_templ, int J, const double *vel, double badchi,
    const double *basis_const, void *scratch, double *out, double *grad,
    int32_t *status, void *stream) {
  return point_grad_launch(arms, narm, npoly, ntan, job_spec, job_templ, J, vel,
                           badchi, basis_const, scratch, out, grad, nullptr,
                           status, stream, true);
}

extern "C" int rvs_chisq_point_fisher_resol(
    const rvs_point_arm *arms, int narm, int npoly, int ntan, const int32_t *job_spec,
    const int32_t *job_templ, int J, const double *vel, double badchi,
    const double *basis_const, void *scratch, double *out, double *grad,
    double *fisher, int32_t *status, void *stream) {
  if (!fisher) return RVS_E_ARG;
  return point_grad_launch(arms, narm, npoly, ntan, job_spec, job_templ, J, vel,
                           badchi, basis_const, scratch, out, grad, fisher, status,
                           stream, true);
}
