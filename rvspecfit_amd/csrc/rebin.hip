// Template libraries from high-resolution models: the band of read_grid.make_rebinner
// (rvs_rebin_weights), its product with a chunk of models (rvs_rebin_apply) and
// make_interpol.extract_spectrum's continuum / log / cast (rvs_template_normalize).
// fp64 throughout; ordinary vector loads and stores only.
#include "common.h"

// ---------------------------------------------------------------------------
// Weights.  The input spectrum is the linear interpolant of its samples, the LSF a
// Gaussian of sigma s, the output pixel the interval [l1, l2].  Integrating the
// convolved interpolant over the pixel and exchanging the integrals gives, for the
// segment [x1, x2] (h = x2 - x1) with values (y1, y2),
//     y1 c1 + y2 c2,   c2 = (1/h) int_{x1}^{x2} (x - x1) K(x) dx,  c1 + c2 = int K dx,
//     K(x) = Phi((l2 - x)/s) - Phi((l1 - x)/s).
// With u = (l - x)/s, c = (l - x1)/s, r = h/s, d = c - r, and the antiderivatives
//     F0(u) = int Phi   = u Phi(u) + phi(u)
//     F1(u) = int u Phi = ((u^2 - 1) Phi(u) + u phi(u)) / 2
// one edge l contributes
//     J0(l) = F0(c) - F0(d)                         (int Phi dx = s J0)
//     J1(l) = c J0(l) - (F1(c) - F1(d))             (int (x - x1) Phi dx = s^2 J1)
// and the segment c2 = s (J1(l2) - J1(l1)) / r, c1 = s (J0(l2) - J0(l1)) - c2.
// F0 and F1 grow like u and u^2 / 2 for u -> +inf (input pixels far to the blue of the
// output pixel), where the edges' contributions cancel.  They are therefore split into
// a polynomial part, which is summed in closed form (for c, d > 0 it is r resp. r^2 / 2
// for EITHER edge and cancels exactly), and a remainder that decays in both tails and
// is evaluated with erfc:
//     F0(u) = G0(u) + max(u, 0),          G0(u) = phi(u) - |u| Phi(-|u|)
//     F1(u) = H1(u) + [u > 0] (u^2 - 1)/2, H1(u) = -sign(u) E(|u|),
//     E(t)  = F1(-t) = ((t^2 - 1) Phi(-t) - t phi(t)) / 2.
// ---------------------------------------------------------------------------
#define RB_ISQRT2 0.70710678118654752440
#define RB_ISQRT2PI 0.39894228040143267794

struct rb_edge {
  double j0, j1;
};

__device__ __forceinline__ void rb_tail(double u, double &g0, double &h1) {
  const double t = fabs(u);
  const double q = 0.5 * erfc(t * RB_ISQRT2);           // Phi(-t)
  const double p = RB_ISQRT2PI * exp(-0.5 * t * t);     // phi(t)
  g0 = p - t * q;
  const double e = 0.5 * ((t * t - 1.0) * q - t * p);
  h1 = u > 0 ? -e : e;
}

__device__ __forceinline__ rb_edge rb_edge_terms(double c, double r) {
  const double d = c - r;
  double g0c, h1c, g0d, h1d;
  rb_tail(c, g0c, h1c);
  rb_tail(d, g0d, h1d);
  double p0, p1;   // polynomial parts of J0, J1
  if (d > 0) {
    p0 = r;
    p1 = 0.5 * r * r;
  } else if (c > 0) {
    p0 = c;
    p1 = 0.5 * c * c + 0.5;
  } else {
    p0 = 0;
    p1 = 0;
  }
  const double dg = g0c - g0d;
  rb_edge e;
  e.j0 = dg + p0;
  e.j1 = c * dg - (h1c - h1d) + p1;
  return e;
}

// Where the input step is not larger than sigma (r <= 1: every real case, PHOENIX has
// r of 0.01) the differences above are of second order in r and lose digits to
// cancellation (eps / r^2).  There the segment's integrals are taken in v = (x - x1)/s,
//     c1 = s int_0^r (1 - v/r) K dv,  c2 = s int_0^r (v/r) K dv,
//     K(v) = Phi(c(l2) - v) - Phi(c(l1) - v),
// by 8-point Gauss-Legendre: the integrand is smooth on the scale 1, every term is
// positive, and the kernel's difference is taken on the side where it does not cancel.
// Asserted: read_grid.pix_integrator, the numpy statement of both branches, against a
// 48-point quadrature to 1e-12 of the pixel width for r = 0.02 .. 200
// (tests/test_make_interpol_cpu.py); this kernel against the same quadrature to 1e-12
// of the row sum for r = 0.006 .. 60 (tests/test_make_interpol_gpu.py; measured 3e-16
// for r <= 1).
__device__ __forceinline__ double rb_kernel(double a, double b) {   // Phi(b) - Phi(a)
  if (a > 0) return 0.5 * (erfc(a * RB_ISQRT2) - erfc(b * RB_ISQRT2));
  if (b < 0) return 0.5 * (erfc(-b * RB_ISQRT2) - erfc(-a * RB_ISQRT2));
  return 1.0 - 0.5 * erfc(b * RB_ISQRT2) - 0.5 * erfc(-a * RB_ISQRT2);
}

// (c1, c2) of the segment [x1, x2] for the pixel [l1, l2] and sigma s
__device__ __forceinline__ void rb_segment(double x1, double x2, double l1, double l2,
                                           double s, double &c1, double &c2) {
  const double r = (x2 - x1) / s;
  const double ca = (l1 - x1) / s, cb = (l2 - x1) / s;
  if (r <= 1.0) {
    const double gx[4] = {0.1834346424956498, 0.5255324099163290, 0.7966664774136267,
                          0.9602898564975363};
    const double gw[4] = {0.3626837833783620, 0.3137066458778873, 0.2223810344533745,
                          0.1012285362903763};
    double s1 = 0, s2 = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
      const double t = 0.5 * (q < 4 ? 1.0 - gx[3 - q] : 1.0 + gx[q - 4]);  // v / r
      const double k = gw[q < 4 ? 3 - q : q - 4] * rb_kernel(ca - t * r, cb - t * r);
      s1 += (1.0 - t) * k;
      s2 += t * k;
    }
    c1 = 0.5 * (x2 - x1) * s1;
    c2 = 0.5 * (x2 - x1) * s2;
    return;
  }
  const rb_edge a = rb_edge_terms(ca, r);
  const rb_edge b = rb_edge_terms(cb, r);
  c2 = s * (b.j1 - a.j1) / r;
  c1 = s * (b.j0 - a.j0) - c2;
}

__global__ void __launch_bounds__(256)
rebin_weights_kernel(const double *__restrict__ lam0, int n0,
                     const double *__restrict__ lam, const double *__restrict__ sigs,
                     const int32_t *__restrict__ left, const int32_t *__restrict__ right,
                     int npix, int K, double *__restrict__ W) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const int i = blockIdx.y;
  if (k >= K) return;
  const int lo = min(max(left[i], 0), n0 - 1), hi = min(right[i], n0 - 2);  // segments
  double w = 0;
  if (k <= hi - lo + 1) {
    const double cur = lam[i];
    const double ls = i > 0 ? 0.5 * (cur - lam[i - 1]) : 0.5 * (lam[1] - cur);
    const double rs = i < npix - 1 ? 0.5 * (lam[i + 1] - cur) : ls;
    const double l1 = cur - ls, l2 = cur + rs, s = sigs[i];
    const int j = lo + k;             // the input pixel
    double c1, c2;
    if (j <= hi) {                    // left end of segment j
      rb_segment(lam0[j], lam0[j + 1], l1, l2, s, c1, c2);
      w += c1;
    }
    if (k > 0) {                      // right end of segment j - 1
      rb_segment(lam0[j - 1], lam0[j], l1, l2, s, c1, c2);
      w += c2;
    }
    w /= (ls + rs);
  }
  W[(int64_t)i * K + k] = w;
}

extern "C" int rvs_rebin_weights(const double *lam0, int n0, const double *lam,
                                 const double *sigs, const int32_t *left,
                                 const int32_t *right, int npix, int K, double *W,
                                 void *stream) {
  if (!lam0 || !lam || !sigs || !left || !right || !W) return RVS_E_ARG;
  if (n0 < 2 || npix < 2 || K < 2 || npix > 65535) return RVS_E_ARG;
  hipLaunchKernelGGL(rebin_weights_kernel, dim3((K + 255) / 256, npix), dim3(256), 0,
                     rvs_stream(stream), lam0, n0, lam, sigs, left, right, npix, K, W);
  RVS_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// Apply.  A block takes RB_PIX output pixels x RB_TT models and walks the union of
// the pixels' windows in chunks of RB_C input pixels, staged in LDS as photons
// (hr * lam0, make_interpol.py:152, when `photons`).  A wave owns 16 consecutive pixels; a lane one
// of them and 8 of the 32 models (models r * 4 + g for lane group g), so the wave
// walks only its own 16 windows' union and a lane outside its window sits a step out.
// LDS reads: the 16 lanes of a group read one address, the two groups of a half wave
// rows RB_LD doubles apart (2 RB_LD mod 64 = 52 banks: no conflict).  Each sum runs in
// ascending input pixel whatever the tile or chunk: splitting the models differently
// gives the same bits.
// ---------------------------------------------------------------------------
#define RB_PIX 64
#define RB_TT 32
#define RB_C 248
#define RB_LD (RB_C + 2)

template <typename HT>
__global__ void __launch_bounds__(256)
rebin_apply_kernel(const HT *__restrict__ hr, int64_t hr_stride, int T, int n0,
                   const double *__restrict__ lam0, const double *__restrict__ W, int K,
                   const int32_t *__restrict__ left, const int32_t *__restrict__ right,
                   const double *__restrict__ lam, int npix, int photons,
                   double *__restrict__ out) {
  __shared__ double xs[RB_TT * RB_LD];
  __shared__ int s_lo, s_hi;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int pl = lane & 15, g = lane >> 4;
  const int i = blockIdx.x * RB_PIX + wv * 16 + pl;
  const int t0 = blockIdx.y * RB_TT;
  const bool live = i < npix;
  // the lane's window: input pixels my_lo .. my_hi - 1
  int my_lo = 0x7fffffff, my_hi = 0;
  if (live) {
    const int lo = min(max(left[i], 0), n0 - 1), hi = min(right[i], n0 - 2);
    my_lo = lo;
    my_hi = min(hi + 2, lo + K);
  }
  int w_lo = my_lo, w_hi = my_hi;
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    w_lo = min(w_lo, __shfl_xor(w_lo, o, 64));
    w_hi = max(w_hi, __shfl_xor(w_hi, o, 64));
  }
  if (tid == 0) {
    s_lo = 0x7fffffff;
    s_hi = 0;
  }
  __syncthreads();
  if (lane == 0 && w_hi > w_lo) {
    atomicMin(&s_lo, w_lo);
    atomicMax(&s_hi, w_hi);
  }
  __syncthreads();
  const int b_lo = s_lo, b_hi = s_hi;
  const double *wrow = W + (int64_t)(live ? i : 0) * K;
  double acc[8];
#pragma unroll
  for (int r = 0; r < 8; r++) acc[r] = 0;
  for (int c0 = b_lo; c0 < b_hi; c0 += RB_C) {
    __syncthreads();
    for (int e = tid; e < RB_TT * RB_C; e += 256) {
      const int t = e / RB_C, c = e - t * RB_C, col = c0 + c;
      double v = 0;
      if (col < b_hi && t0 + t < T) {
        v = (double)hr[(int64_t)(t0 + t) * hr_stride + col];
        if (photons) v *= lam0[col];
      }
      xs[t * RB_LD + c] = v;
    }
    __syncthreads();
    const int j0 = max(w_lo, c0), j1 = min(w_hi, c0 + RB_C);
    // eight weights in flight per lane before their products: the loads are what a
    // step waits for
    for (int cb = j0; cb < j1; cb += 8) {
      double w[8];
      bool in[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int col = cb + u;
        in[u] = col < j1 && col >= my_lo && col < my_hi;
        w[u] = in[u] ? wrow[col - my_lo] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) {
        if (in[u]) {
          const double *x = xs + g * RB_LD + (cb + u - c0);
#pragma unroll
          for (int r = 0; r < 8; r++) acc[r] = fma(w[u], x[r * 4 * RB_LD], acc[r]);
        }
      }
    }
  }
  if (live) {
    const double li = photons ? lam[i] : 1.0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
      const int t = t0 + r * 4 + g;
      if (t < T) out[(int64_t)t * npix + i] = photons ? acc[r] / li : acc[r];
    }
  }
}

extern "C" int rvs_rebin_apply(const void *hr, int hr_f32, int64_t hr_stride, int T,
                               int n0, const double *lam0, const double *W, int K,
                               const int32_t *left, const int32_t *right,
                               const double *lam, int npix, int photons, double *out,
                               void *stream) {
  if (!hr || !W || !left || !right || !out) return RVS_E_ARG;
  if (photons && (!lam0 || !lam)) return RVS_E_ARG;
  if (T < 1 || n0 < 2 || npix < 2 || K < 2 || hr_stride < n0) return RVS_E_ARG;
  const int by = (T + RB_TT - 1) / RB_TT;
  if (by > 65535) return RVS_E_ARG;
  const dim3 grid((npix + RB_PIX - 1) / RB_PIX, by);
  if (hr_f32)
    hipLaunchKernelGGL(rebin_apply_kernel<float>, grid, dim3(256), 0, rvs_stream(stream),
                       (const float *)hr, hr_stride, T, n0, lam0, W, K, left, right, lam,
                       npix, photons, out);
  else
    hipLaunchKernelGGL(rebin_apply_kernel<double>, grid, dim3(256), 0,
                       rvs_stream(stream), (const double *)hr, hr_stride, T, n0, lam0, W,
                       K, left, right, lam, npix, photons, out);
  RVS_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// Normalise.  One block of 512 threads per row, the row's values (as order-preserving
// integer keys) in registers: 18 per thread cover RVS_REBIN_MAX_NPIX = 9216.  A median
// is a selection by rank: the largest key v with #{key < v} <= k is the k-th smallest,
// found bit by bit from the top (64 block-wide counts); both middle ranks of an even
// count go through the same passes.
// ---------------------------------------------------------------------------
#define NZ_NT 512
#define NZ_PER 18

__device__ __forceinline__ uint64_t nz_key(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double nz_unkey(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// np.median of row[a .. a + n): the mean of the two middle values for an even n, NaN
// if the segment holds one.  All threads call it and receive the result.
__device__ double nz_median(const double *__restrict__ row, int a, int n, int *red) {
  const int tid = threadIdx.x;
  uint64_t key[NZ_PER];
  int anynan = 0;
#pragma unroll
  for (int q = 0; q < NZ_PER; q++) {
    const int e = tid + q * NZ_NT;
    key[q] = ~0ull;                       // beyond the segment: above every rank asked
    if (e < n) {
      const double v = row[a + e];
      anynan |= (v != v);
      key[q] = nz_key(v);
    }
  }
  const int k1 = n / 2, k0 = (n & 1) ? k1 : k1 - 1;
  uint64_t r0 = 0, r1 = 0;
  for (int bit = 63; bit >= 0; bit--) {
    const uint64_t c0 = r0 | (1ull << bit), c1 = r1 | (1ull << bit);
    int n0 = 0, n1 = 0;
#pragma unroll
    for (int q = 0; q < NZ_PER; q++) {
      n0 += key[q] < c0;
      n1 += key[q] < c1;
    }
    n0 = wave_sum_i(n0);
    n1 = wave_sum_i(n1);
    __syncthreads();
    if ((tid & 63) == 0) {
      red[(tid >> 6) * 2] = n0;
      red[(tid >> 6) * 2 + 1] = n1;
    }
    __syncthreads();
    n0 = n1 = 0;
#pragma unroll
    for (int w = 0; w < NZ_NT / 64; w++) {
      n0 += red[2 * w];
      n1 += red[2 * w + 1];
    }
    if (n0 <= k0) r0 = c0;
    if (n1 <= k1) r1 = c1;
  }
  anynan = wave_sum_i(anynan);
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = anynan;
  __syncthreads();
  anynan = 0;
#pragma unroll
  for (int w = 0; w < NZ_NT / 64; w++) anynan += red[w];
  if (anynan) return __longlong_as_double(0x7ff8000000000000ll);
  const double v0 = nz_unkey(r0), v1 = nz_unkey(r1);
  return (n & 1) ? v1 : 0.5 * (v0 + v1);
}

__global__ void __launch_bounds__(NZ_NT)
template_normalize_kernel(const double *__restrict__ rows, int npix,
                          const double *__restrict__ lam, int mode, double lam1,
                          double lam2, int log_spec, int float_bits,
                          void *__restrict__ out, double *__restrict__ lognorms,
                          int32_t *__restrict__ status) {
  __shared__ int red[2 * NZ_NT / 64];
  __shared__ int s_bad;
  const int t = blockIdx.x, tid = threadIdx.x;
  const double *row = rows + (int64_t)t * npix;
  if (tid == 0) s_bad = 0;
  double y1 = 0, y2 = 0, f = 0, norm = 1.0;
  if (mode == RVS_NORM_LINEAR_CONTINUUM) {
    // get_line_continuum: the medians of the two halves, the line through their logs
    // in the degree-1 B-spline's form y1 f (lam2 - x) + y2 f (x - lam1), extrapolated
    const int h = npix / 2;
    y1 = log(nz_median(row, 0, h, red));
    y2 = log(nz_median(row, h, npix - h, red));
    f = 1.0 / (lam2 - lam1);
  } else if (mode == RVS_NORM_MEDIAN) {
    norm = nz_median(row, 0, npix, red);
  }
  __syncthreads();
  int bad = 0;
  for (int i = tid; i < npix; i += NZ_NT) {
    double v = row[i];
    if (mode == RVS_NORM_LINEAR_CONTINUUM) {
      const double x = lam[i];
      v = v / exp(y1 * (f * (lam2 - x)) + y2 * (f * (x - lam1)));
    } else if (mode == RVS_NORM_MEDIAN) {
      v = v / norm;
    }
    if (log_spec) v = log(v);
    bad |= !isfinite(v);
    if (float_bits == 32)
      ((float *)out)[(int64_t)t * npix + i] = (float)v;
    else
      ((double *)out)[(int64_t)t * npix + i] = v;
  }
  if (bad) s_bad = 1;
  __syncthreads();
  if (tid == 0) {
    if (lognorms) lognorms[t] = log(norm);
    status[t] = s_bad ? RVS_ST_NONFINITE : 0;
  }
}

extern "C" int rvs_template_normalize(const double *rows, int T, int npix,
                                      const double *lam, int mode, double lam1,
                                      double lam2, int log_spec, int float_bits,
                                      void *out, double *lognorms, int32_t *status,
                                      void *stream) {
  if (!rows || !lam || !out || !status) return RVS_E_ARG;
  if (T < 1 || npix < 2 || npix > RVS_REBIN_MAX_NPIX) return RVS_E_ARG;
  if (mode != RVS_NORM_NONE && mode != RVS_NORM_MEDIAN &&
      mode != RVS_NORM_LINEAR_CONTINUUM)
    return RVS_E_ARG;
  if (float_bits != 32 && float_bits != 64) return RVS_E_ARG;
  if (mode == RVS_NORM_LINEAR_CONTINUUM && !(lam2 > lam1)) return RVS_E_ARG;
  hipLaunchKernelGGL(template_normalize_kernel, dim3(T), dim3(NZ_NT), 0,
                     rvs_stream(stream), rows, npix, lam, mode, lam1, lam2, log_spec,
                     float_bits, out, lognorms, status);
  RVS_LAUNCH_CHECK();
  return 0;
}
