// objective_grad.hip -- the optimiser's objective AND its gradient at one (template
// parameters, vsini, velocity) point per job, as a single kernel: the adjoint of
// objective.hip's template path.
//
// The gradient chain (bfgs_grad.hip) pushes 1 + ntan template rows through gather,
// FIR and spline solve and leaves 32 (1 + ntan) ntp bytes of spline records per (job,
// arm) in HBM for rvs_chisq_point_grad.  That path is LINEAR in the template row, so
// its transpose carries ONE row back from the pixels to the knots, whatever ntan is,
// and that row fits the three buffers of ntp doubles the value already uses.  One
// 512-thread block owns a (job, arm):
//   B0 <- t      polylinear gather of the 2^ndim float32 rows + exp          (A3, A5)
//   Y  <- y      rotational-broadening FIR of t (taps staged in the other two)  (A6)
//   Z  <- z      natural spline of y: chunked Thomas sweeps over the factors of
//                rvs_spline_factors, chunks joined by their transfer coefficients (A7)
//   pass 1       threads = pixels: spline value, normal equations; {m/e, D/e} -> F
//   factor       every lane factors the folded matrix (the Cholesky factor stays in
//                its registers, as in point_grad_block)
//   pass 2       residual, q = |L^-1 phi|^2, s = c.phi: the pixel adjoint
//                mbar = 2 (m/e^2) q - 2 r s/e -> F[0, npix); the velocity component
//   (t, y, z are dead from here on)
//   first[]      first pixel of every knot interval (int32, behind mbar in F)
//   gather       threads = knots: ybar, zbar from the pixels of the two intervals a
//                knot touches, in pixel order                      (resampling^T)
//   solve        M u = zbar, M symmetric: the sweeps of the value     (spline^T)
//   ybar +=      (sl_{n-1} / h_{n-1} - sl_n / h_n), sl_j = 6 (u_{j-1} - u_j)
//   tbar <- w (*) ybar: the taps are symmetric and the ends zero padded   (FIR^T)
//   contract     threads = knots: the vertex rows are read AGAIN, t_n and the tangents
//                t_n sum_v (dw_v/dp_d) L_vn are formed per knot as polylinear_kernel<true>
//                forms them and contracted with tbar at once; with vsini fitted
//                vbar_n = (dw/dvsini (*) ybar)_n is formed on the fly and contracted
//                with t_n
// No template row, spline record or adjoint row goes to HBM.  There is no floating
// point atomic: every sum has a fixed order (lanes by butterfly, waves in order), so
// repeated runs and permuted job lists agree to the bit.  The value phases repeat the
// arithmetic of the stand-alone kernels they replace.
#include "objective_dev.h"

#define OG_NT RVS_OBJ_NT
#define OG_NW (OG_NT / 64)
#define OG_CHMAX RVS_OBJ_CHMAX
#define OG_MAXP 10     // beyond: the value kernel's wave totals live in the template buffer
#define OG_MAXDIM 4    // the bound of the cell record (OBJ_LOC_NV vertices)
#define OG_MAXK (2 + OG_MAXDIM)   // vel, parameters, vsini
// upper bound of the kernel's static LDS (OgShared): what rvs_objective_grad_ok, host
// arithmetic only, counts beside the three template buffers
#define OG_STATIC_MAX 8192
#define OG_LDS_MAX (160 * 1024)

namespace {

template <int P>
struct OgShared {
  static constexpr int NV = P * (P + 1) / 2 + P;
  PolyLoc PL;
  double dw[OG_MAXDIM << OG_MAXDIM];   // dw_v/dp_d [d][v] (polylinear_kernel<true>)
  double red[OG_NW][(NV > OG_MAXK + 1 ? NV : OG_MAXK + 1) + 1];
  double edge[2][OG_NW][6];   // chunk coefficients across wave boundaries
  double red8[2 * OG_NW];
  double fact[2];             // log det L, 1: every pivot positive
  double jobsc[3];            // obj_job_scalars
};

template <int P>
__global__ void __launch_bounds__(OG_NT)
    objective_grad_kernel(ObjArms A, const double *__restrict__ params,
                          const double *__restrict__ vsini, int vsini_grad,
                          const int32_t *__restrict__ job_spec, int J,
                          const double *__restrict__ vel, double eps_ld,
                          double *__restrict__ armchi, double *__restrict__ armgrad,
                          int32_t *__restrict__ armst, double *__restrict__ armout) {
  constexpr int NTR = P * (P + 1) / 2;
  constexpr int NV = NTR + P;
  static_assert(sizeof(OgShared<P>) <= OG_STATIC_MAX, "rvs_objective_grad_ok's bound");
  extern __shared__ double lds[];
  __shared__ OgShared<P> sh;
  const rvs_objective_arm &T = A.a[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j = blockIdx.x;
  const int N = T.ntp, m = N - 2;
  const int nd = T.ndim, nv = 1 << nd;
  const int K = 1 + nd + (vsini_grad ? 1 : 0);
  const int64_t o = (int64_t)blockIdx.y * J + j;
  double *B0 = lds, *B1 = lds + N, *B2 = lds + 2 * (int64_t)N;
  PolyLoc &PL = sh.PL;

  // ---- cell search, dw/dp, the job's Doppler scalars ----------------------------
  const GridDesc G = obj_grid_desc(T);
  const double *prow = params + (int64_t)j * nd;
  poly_locate<OG_NT>(PL, G, prow, T.idgrid, T.uvecs, T.vecs_s, T.ngrid);
  const int mode = PL.mode;
  if (mode == 0) {
    // the weight's factor of dimension d replaced by -+1 / (cell width), per PHYSICAL
    // unit of p_d (the chain through log10 of a log_mask parameter included)
    for (int i = tid; i < nd * nv; i += OG_NT) {
      const int d = i >> nd, v = i & (nv - 1);
      const double *u = T.uvecs + sel_dim(G.uoff, d);
      const int p = PL.pos[d];
      double wd = 1.0 / (u[p + 1] - u[p]);
      if (G.log_mask & (1u << d)) wd /= prow[d] * 2.302585092994046;
      if (!((v >> (nd - 1 - d)) & 1)) wd = -wd;
      for (int e = 0; e < nd; e++)
        if (e != d) wd *= ((v >> (nd - 1 - e)) & 1) ? PL.x[e] : (1 - PL.x[e]);
      sh.dw[d * nv + v] = wd;
    }
  }
  if (tid == 64) obj_job_scalars(T.pt, vel[j], sh.jobsc);
  __syncthreads();

  // ---- A3/A5: the template into B0 ------------------------------------------------
  const float *nrow = T.dats + (int64_t)(mode == 0 ? 0 : PL.nearest) * N;
  double outside = 0.0;
  if (mode == 0) {
    for (int k = tid; k < N; k += OG_NT) {
      double acc = 0;
      for (int v = 0; v < nv; v++)
        acc = fma(PL.w[v], (double)T.dats[PL.id[v] * N + k], acc);
      B0[k] = T.exp_flag ? exp(acc) : acc;
    }
  } else {
    double mx = 0;
    bool anynan = false;
    for (int k = tid; k < N; k += OG_NT) {
      const double val = T.exp_flag ? (double)np_expf(nrow[k]) : (double)nrow[k];
      B0[k] = val;
      if (!(val == val)) anynan = true;
      mx = fmax(mx, fabs(val));
    }
    // MAX_VAL guard of getCurTempl (spec_fit.py:392-397)
    mx = wave_max(mx);
    const double nanf = wave_sum(anynan ? 1.0 : 0.0);
    if (lane == 0) {
      sh.red8[w] = mx;
      sh.red8[OG_NW + w] = nanf;
    }
    __syncthreads();
    double mm = 0, nn = 0;
    for (int i = 0; i < OG_NW; i++) {
      mm = fmax(mm, sh.red8[i]);
      nn += sh.red8[OG_NW + i];
    }
    outside = PL.dist;
    if (outside > 0 && (mm > 1e100 || nn > 0 || isinf(mm))) outside = __builtin_nan("");
  }
  __syncthreads();
  if (!(fabs(outside) <= 1.79e308)) {   // unusable template: the arm is skipped
    if (tid == 0) {
      armout[o] = __builtin_nan("");
      armchi[o] = 0.0;
      armst[o] = 0;
    }
    if (tid < K) armgrad[o * K + tid] = 0.0;
    return;
  }

  // ---- the rotational kernel ------------------------------------------------------
  bool refused = false;
  int kmax = 0;
  if (vsini) {
    double R_;
    kmax = obj_rot_kmax(T, vsini[j], R_, refused);
  }
  const bool copy = kmax == 0;
  const int st_extra = refused ? RVS_ST_NONFINITE : 0;
  // normalised taps 0 .. kmax into wt and, with dwt, their derivatives by vsini
  // (vsini_kernel<true>: W' over the clipped legs of the value, dw = (W' - w S') / S /
  // (c lnstep)); `stage` holds the primitives at x_j = clip(j / R), j = -1 .. kmax + 1,
  // as two runs of kmax + 3 doubles.  Called by the whole block.
  auto build_taps = [&](double *stage, double *wt, double *dwt) {
    const double R = (vsini[j] / RVS_C_KMS) / T.lnstep;   // (obj_rot_kmax's)
    double *pk0 = stage, *pk1 = stage + (kmax + 3);
    for (int jj = tid; jj <= kmax + 2; jj += OG_NT) {
      const double x = fmin(fmax((jj - 1) / R, -1.0), 1.0);
      double k0, k1;
      rot_prim(x, eps_ld, k0, k1);
      pk0[jj] = k0;
      pk1[jj] = k1;
    }
    __syncthreads();
    double psum = 0, dsum = 0;
    for (int k = tid; k <= kmax; k += OG_NT) {
      const double ww = obj_rot_tap_raw(k, R, pk0, pk1);
      wt[k] = ww;
      psum += (k == 0) ? ww : 2 * ww;
      if (dwt) {
        double d = 0;
        double lo = fmin(fmax(k / R, -1.0), 1.0), hi = fmin(fmax((k + 1) / R, -1.0), 1.0);
        if (hi > lo) d += -1.0 * (pk1[k + 2] - pk1[k + 1]);   // rot_segment(lo, hi, -1, 0)
        lo = fmin(fmax((k - 1) / R, -1.0), 1.0);
        hi = fmin(fmax(k / R, -1.0), 1.0);
        if (hi > lo) d += 1.0 * (pk1[k + 1] - pk1[k]);        // rot_segment(lo, hi, 1, 0)
        dwt[k] = d;
        dsum += (k == 0) ? d : 2 * d;
      }
    }
    psum = block_sum<OG_NW>(psum, sh.red8);
    if (dwt) dsum = block_sum<OG_NW>(dsum, sh.red8);
    const double inv = 1.0 / psum;
    const double dscale = inv / (RVS_C_KMS * T.lnstep);
    for (int k = tid; k <= kmax; k += OG_NT) {
      const double ww = wt[k];
      if (dwt) dwt[k] = (dwt[k] - ww * inv * dsum) * dscale;
      wt[k] = ww * inv;
    }
    __syncthreads();
  };
  // 'same' convolution with zero padding and the symmetric taps tp[|m|], ascending
  // input index (vsini_fir)
  auto fir_at = [&](const double *in, const double *tp, int i) {
    double acc = 0;
    const int q0 = max(i - kmax, 0), q1 = min(i + kmax, N - 1);
    for (int q = q0; q <= q1; q++) {
      const int mm = q - i;
      acc = fma(in[q], tp[mm < 0 ? -mm : mm], acc);
    }
    return acc;
  };

  // ---- A6: y = w (*) t ------------------------------------------------------------
  // Y, Z: the buffers of y and z; F: the third one (taps, then the pixel pair)
  double *Y = B0, *Z = B1, *F = B2;
  if (!copy) {
    build_taps(B1, B2, nullptr);
    for (int i = tid; i < N; i += OG_NT) B1[i] = fir_at(B0, B2, i);
    Y = B1;
    Z = B0;
    __syncthreads();
  }

  // ---- A7 construct: the natural spline's tridiagonal solve ------------------------
  // Thread t owns the rows [a0, a1) (CH of them) of the m unknowns; both sweeps are
  // linear in the value that enters the chunk, d_i = d0_i + P_i d_in, so one pass over
  // the chunk yields (alpha, beta) at its last row and
  //   d_in(t) = alpha(t-1) + beta(t-1) (alpha(t-2) + beta(t-2) alpha(t-3))
  // to |beta|^3 <= (0.268^12)^3 (objective.hip).  The factors are the chunk-ordered
  // copy of rvs_spline_factors: record {1/h_u, 1/h_{u+1}, g_u, e_u} of row t CH + q at
  // [q][t], then the backward multipliers in pairs.
  const int CH = rvs_obj_chunk_len(m);
  const int a0 = min(m, tid * CH), a1 = min(m, a0 + CH);
  const double *FT = T.factors + 5 * (int64_t)N;
  const double *FC = FT + 4 * (int64_t)OG_NT * OG_CHMAX;
  auto chain3 = [&](double al, double be, int dir) -> double {
    double (*eds)[6] = sh.edge[dir < 0 ? 0 : 1];
    double av3[3], bv3[3];
#pragma unroll
    for (int k = 1; k <= 3; k++) {
      av3[k - 1] = (dir < 0) ? __shfl_up(al, k, 64) : __shfl_down(al, k, 64);
      bv3[k - 1] = (dir < 0) ? __shfl_up(be, k, 64) : __shfl_down(be, k, 64);
    }
    const int edge = (dir < 0) ? (63 - lane) : lane;   // 0..2: published lanes
    if (edge < 3) {   // (one array per direction; barriers between the two solves)
      eds[w][2 * edge] = al;
      eds[w][2 * edge + 1] = be;
    }
    __syncthreads();
    const int mine = (dir < 0) ? lane : (63 - lane);   // distance to the boundary
#pragma unroll
    for (int k = 1; k <= 3; k++) {
      if (mine < k) {   // neighbour k lives in the adjacent wave
        const int ww = w + dir;
        const int sl = k - 1 - mine;   // its distance from that wave's boundary
        const bool have = (ww >= 0 && ww < OG_NW);
        av3[k - 1] = have ? eds[ww][2 * sl] : 0.0;
        bv3[k - 1] = have ? eds[ww][2 * sl + 1] : 0.0;
      }
    }
    return av3[0] + bv3[0] * (av3[1] + bv3[1] * av3[2]);
  };
  // M x = rhs: rhs(u, 1/h_u, 1/h_{u+1}) is read by the row's owner ahead of every
  // barrier and x written behind them, so `out` may be the buffer rhs reads
  auto tri_solve = [&](auto rhs, double *out) {
    double loc[OG_CHMAX], pr[OG_CHMAX];
    double d = 0, pb = 1;
#pragma unroll
    for (int q = 0; q < OG_CHMAX; q++)
      if (q < CH && a0 + q < a1) {
        const double *rec = FT + ((int64_t)q * OG_NT + tid) * 4;
        const double ei = rec[3];
        d = rhs(a0 + q, rec[0], rec[1]) * rec[2] - ei * d;
        pb = -ei * pb;
        loc[q] = d;
        pr[q] = pb;
      }
    const double d_in = chain3(d, pb, -1);
    double z = 0;
    pb = 1;
#pragma unroll
    for (int q = OG_CHMAX - 1; q >= 0; q--)
      if (q < CH && a0 + q < a1) {
        const double ci = FC[((int64_t)(q >> 1) * OG_NT + tid) * 2 + (q & 1)];
        z = (loc[q] + pr[q] * d_in) - ci * z;   // d of the forward sweep, then z
        pb = -ci * pb;
        loc[q] = z;
        pr[q] = pb;
      }
    const double z_in = chain3(z, pb, +1);
#pragma unroll
    for (int q = 0; q < OG_CHMAX; q++)
      if (q < CH && a0 + q < a1) out[a0 + q] = loc[q] + pr[q] * z_in;
  };
  // right-hand sides 6 ((y_{u+2} - y_{u+1}) / h_{u+1} - (y_{u+1} - y_u) / h_u); Z[u] =
  // z at knot u + 1
  tri_solve([&](int u, double ih0, double ih1) {
    const double s0 = (Y[u + 1] - Y[u]) * ih0, s1 = (Y[u + 2] - Y[u + 1]) * ih1;
    return 6 * (s1 - s0);
  }, Z);
  __syncthreads();

  // ---- the pixels -----------------------------------------------------------------
  const rvs_point_arm &S = T.pt;
  const int npix = S.npix;
  const int s = job_spec ? job_spec[j] : j;
  const ObjArmGrid AG = obj_arm_grid(S, s);
  // {1/e, D/e} of the spectrum's pixels (rvs_chisq_prepare)
  const double2 *sig = reinterpret_cast<const double2 *>(
                           AG.wbase + 2ll * S.S * npix + 2ll * S.S) + (int64_t)s * npix;
  const double x0 = S.knots[0], xlast = S.knots[N - 1];
  const double *hh = T.factors + 3 * (int64_t)N, *ih = T.factors + 4 * (int64_t)N;
  const double f = sh.jobsc[0], shift = sh.jobsc[1], lin_inv_step = sh.jobsc[2];
  auto pix_pos = [&](int k) {   // the knot interval of pixel k (point_knot)
    int pos = S.log_step ? (int)(AG.pix[k] + shift)
                         : (int)((AG.lam[k] * f - x0) * lin_inv_step);
    return min(max(pos, 0), N - 2);
  };
  // spline piece of the interval in powers of dl, as rvs_spline_construct(form 1)
  auto piece = [&](int pos, double &yi, double &cb, double &c2, double &c3) {
    const double h = hh[pos], hinv = ih[pos];
    const double zi = (pos == 0) ? 0.0 : Z[pos - 1];
    const double zi1 = (pos + 1 == N - 1) ? 0.0 : Z[pos];
    const double yi1 = Y[pos + 1];
    yi = Y[pos];
    const double t1 = hinv * (1.0 / 6), t2 = h * (1.0 / 6);
    cb = (yi1 - yi) * hinv - t2 * (2 * zi + zi1);
    c2 = 0.5 * zi;
    c3 = (zi1 - zi) * t1;
  };
  // pass 1: model and data in units of sigma into F ([npix] m/e, [npix] D/e), the
  // normal equations per lane
  // (a loop of its own, which holds no accumulators, as in objective_kernel)
  for (int k = tid; k < npix; k += OG_NT) {
    const int pos = pix_pos(k);
    const double dl = AG.lam[k] * f - S.knots[pos];
    double yi, cb, c2, c3;
    piece(pos, yi, cb, c2, c3);
    const double tv = fma(fma(fma(c3, dl, c2), dl, cb), dl, yi);
    const double2 sg = sig[k];
    F[k] = tv * sg.x;
    F[npix + k] = sg.y;
  }
  {
    double vals[NV];   // [NTR] packed lower triangle, then [P] right-hand sides
#pragma unroll
    for (int i = 0; i < NV; i++) vals[i] = 0;
    for (int k = tid; k < npix; k += OG_NT) {
      const double te = F[k], dk = F[npix + k];   // (written by this same thread)
      // (the rows ST = phi m/e themselves: one register row where the value kernel
      // keeps phi and phi (m/e)^2 -- this kernel has the adjoint's state beside it)
      const double *pr = AG.polysT + (int64_t)k * P;
      double sv[P];
#pragma unroll
      for (int i = 0; i < P; i++) sv[i] = pr[i] * te;
#pragma unroll
      for (int i = 0; i < P; i++) {
        vals[NTR + i] = fma(sv[i], dk, vals[NTR + i]);
#pragma unroll
        for (int jj = 0; jj <= i; jj++)
          vals[TRI(i, jj)] = fma(sv[i], sv[jj], vals[TRI(i, jj)]);
      }
    }
    // slot i of a lane stands for sum number base + i (wave_halve)
    int cnt, base, lim;
    wave_halve<NV>(vals, lane, cnt, base, lim);
#pragma unroll
    for (int i = 0; i < (NV + 63) / 64 + 1; i++)
      if (i < cnt && base + i < lim) sh.red[w][base + i] = vals[i];
  }
  __syncthreads();
  if (tid < NV) {   // the waves' totals in wave order, one sum per thread
    double v = sh.red[0][tid];
#pragma unroll
    for (int q = 1; q < OG_NW; q++) v += sh.red[q][tid];
    sh.red[0][tid] = v;
  }
  __syncthreads();
  // every lane factors the same matrix: A = L L^T in place with 1 / L_ii on the diagonal
  // (the only form the substitutions need), c = A^-1 v by the two substitutions
  // (point_grad_block)
  double acc[NTR], av[P];
  bool okl = true;
  double ldet = 0;
#pragma unroll
  for (int i = 0; i < NTR; i++) acc[i] = sh.red[0][i];
#pragma unroll
  for (int i = 0; i < P; i++) av[i] = sh.red[0][NTR + i];
#pragma unroll
  for (int i = 0; i < P; i++) {
#pragma unroll
    for (int jj = 0; jj <= i; jj++) {
      double sum = acc[TRI(i, jj)];
#pragma unroll
      for (int q = 0; q < jj; q++) sum -= acc[TRI(i, q)] * acc[TRI(jj, q)];
      if (jj == i) {
        if (!(sum > 0)) okl = false;
        const double d = sqrt(sum);
        acc[TRI(i, i)] = 1.0 / d;
        ldet += log(d);
      } else {
        acc[TRI(i, jj)] = sum * acc[TRI(jj, jj)];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < P; i++) {
    double sum = av[i];
#pragma unroll
    for (int q = 0; q < i; q++) sum -= acc[TRI(i, q)] * av[q];
    av[i] = sum * acc[TRI(i, i)];
  }
#pragma unroll
  for (int i = P - 1; i >= 0; i--) {
    double sum = av[i];
#pragma unroll
    for (int q = i + 1; q < P; q++) sum -= acc[TRI(q, i)] * av[q];
    av[i] = sum * acc[TRI(i, i)];
  }
  // log det L and the pivots' verdict, every lane's the same, wait in LDS for the tail:
  // L, the coefficients, a row of the basis and y = L^-1 phi fill a lane's registers at
  // P = 10 (with these three values live across the pass: 28 B of scratch per lane)
  if (tid == 0) {
    sh.fact[0] = ldet;
    sh.fact[1] = okl ? 1.0 : 0.0;
  }
  // pass 2: residual, the pixel adjoint into F[0, npix), the velocity component
  //   d chi^2 / d vel = sum_k mbar_k S'(x_k) lam_k df/dvel
  const double bb = vel[j] / RVS_C_KMS;
  const double dfdv = -f / (RVS_C_KMS * (1.0 - bb * bb));
  double rr = 0, gvel = 0;
  for (int k = tid; k < npix; k += OG_NT) {
    const double te = F[k], dk = F[npix + k];
    const double ie = sig[k].x;
    const double *pr = AG.polysT + (int64_t)k * P;
    double yv[P], mk = 0, qk = 0;
#pragma unroll
    for (int i = 0; i < P; i++) {
      const double ph = pr[i];
      mk = fma(av[i], ph, mk);
      double sum = ph;
#pragma unroll
      for (int qq = 0; qq < i; qq++) sum = fma(-acc[TRI(i, qq)], yv[qq], sum);
      yv[i] = sum * acc[TRI(i, i)];
      qk = fma(yv[i], yv[i], qk);
    }
    const double r = dk - mk * te;
    rr = fma(r, r, rr);
    const double mbar = 2.0 * ie * (te * qk - r * mk);
    const int pos = pix_pos(k);
    const double lamk = AG.lam[k];
    const double dl = lamk * f - S.knots[pos];
    double yi, cb, c2, c3;
    piece(pos, yi, cb, c2, c3);
    const double dtv = fma(dl, fma(3.0 * c3, dl, 2.0 * c2), cb);
    gvel = fma(mbar, dtv * (lamk * dfdv), gvel);
    F[k] = mbar;
  }
  __syncthreads();   // y, z and the data column of F are dead

  // ---- resampling, transposed -------------------------------------------------------
  // first[n] = the number of pixels in intervals below n (pixels ascend in wavelength,
  // so the pixels of interval n are [first[n], first[n + 1])); every entry is written
  // once, by the first pixel at or behind it
  int32_t *first = reinterpret_cast<int32_t *>(F + npix);
  for (int k = tid; k <= npix; k += OG_NT) {
    const int lo = (k == 0) ? 0 : pix_pos(k - 1) + 1;
    const int hi = (k == npix) ? N - 1 : pix_pos(k);
    for (int n = lo; n <= hi; n++) first[n] = k;
  }
  __syncthreads();
  // the thread of knot n adds, in pixel order, the pixels of intervals n - 1 and n;
  // the boundary entries of zbar are dropped (natural ends); Z[u] = zbar at knot u + 1
  // (clamped: were the pixels not ascending, entries of the table would be unwritten)
  auto first_at = [&](int n) { return min(max(first[n], 0), npix); };
  double *Yb = Y, *Zb = Z;
  for (int n = tid; n < N; n += OG_NT) {
    double yb = 0, zb = 0;
    if (n >= 1) {
      const double kn = S.knots[n - 1], h = hh[n - 1], hinv = ih[n - 1];
      const int k1 = first_at(n);
      for (int k = first_at(n - 1); k < k1; k++) {
        const double dl = AG.lam[k] * f - kn, mb = F[k];
        const double dl3 = dl * dl * dl * hinv * (1.0 / 6);
        yb = fma(mb, dl * hinv, yb);
        zb = fma(mb, dl3 - dl * h * (1.0 / 6), zb);
      }
    }
    if (n <= N - 2) {
      const double kn = S.knots[n], h = hh[n], hinv = ih[n];
      const int k1 = first_at(n + 1);
      for (int k = first_at(n); k < k1; k++) {
        const double dl = AG.lam[k] * f - kn, mb = F[k];
        const double dl3 = dl * dl * dl * hinv * (1.0 / 6);
        yb = fma(mb, 1.0 - dl * hinv, yb);
        zb = fma(mb, 0.5 * dl * dl - dl * h * (1.0 / 3) - dl3, zb);
      }
    }
    Yb[n] = yb;
    if (n >= 1 && n <= N - 2) Zb[n - 1] = zb;
  }
  __syncthreads();

  // ---- spline, transposed: M u = zbar (M is symmetric: the sweeps of the value) ----
  tri_solve([&](int u, double, double) { return Zb[u]; }, Zb);
  __syncthreads();
  // sl_j = 6 (u_{j-1} - u_j), u_j at knot j + 1, 0 beyond both ends;
  // ybar_{j+1} += sl_j / h_j, ybar_j -= sl_j / h_j
  {
    auto U = [&](int i) { return (i >= 0 && i < m) ? Zb[i] : 0.0; };
    for (int n = tid; n < N; n += OG_NT) {
      double add = 0;
      if (n >= 1) add = 6 * (U(n - 2) - U(n - 1)) * ih[n - 1];
      if (n <= N - 2) add -= 6 * (U(n - 1) - U(n)) * ih[n];
      Yb[n] += add;
    }
  }
  __syncthreads();

  // ---- FIR, transposed: tbar = w (*) ybar -------------------------------------------
  const bool vs_grad = vsini_grad && !copy;
  double *tbar = Yb;
  const double *dwt = nullptr;
  if (!copy) {
    build_taps(Zb, F, vs_grad ? F + kmax + 1 : nullptr);
    for (int i = tid; i < N; i += OG_NT) Zb[i] = fir_at(Yb, F, i);
    tbar = Zb;
    dwt = F + kmax + 1;
    __syncthreads();
  }

  // ---- contraction at the knots -----------------------------------------------------
  double gp[OG_MAXDIM], gvs = 0;
#pragma unroll
  for (int d = 0; d < OG_MAXDIM; d++) gp[d] = 0;
  for (int n = tid; n < N; n += OG_NT) {
    double tn;
    if (mode == 0) {
      double a = 0, g[OG_MAXDIM];
#pragma unroll
      for (int d = 0; d < OG_MAXDIM; d++) g[d] = 0;
      for (int v = 0; v < nv; v++) {
        const double Lv = (double)T.dats[PL.id[v] * N + n];
        a = fma(PL.w[v], Lv, a);
#pragma unroll
        for (int d = 0; d < OG_MAXDIM; d++)
          if (d < nd) g[d] = fma(sh.dw[d * nv + v], Lv, g[d]);
      }
      tn = T.exp_flag ? exp(a) : a;
      const double tb = tbar[n];
#pragma unroll
      for (int d = 0; d < OG_MAXDIM; d++)
        if (d < nd) gp[d] = fma(tb, T.exp_flag ? tn * g[d] : g[d], gp[d]);
    } else {
      tn = T.exp_flag ? (double)np_expf(nrow[n]) : (double)nrow[n];
    }
    if (vs_grad) gvs = fma(fir_at(Yb, dwt, n), tn, gvs);
  }

  // ---- the block's sums: lanes by butterfly, waves in order ---------------------------
  {
    double fin[OG_MAXK + 1];
    fin[0] = rr;
    fin[1] = gvel;
#pragma unroll
    for (int d = 0; d < OG_MAXDIM; d++) fin[2 + d] = gp[d];
    fin[2 + OG_MAXDIM] = gvs;
#pragma unroll
    for (int i = 0; i <= OG_MAXK; i++) {
      const double v = wave_sum(fin[i]);
      if (lane == 0) sh.red[w][i] = v;
    }
  }
  __syncthreads();
  if (tid <= OG_MAXK) {
    double v = sh.red[0][tid];
#pragma unroll
    for (int q = 1; q < OG_NW; q++) v += sh.red[q][tid];
    sh.red[0][tid] = v;
  }
  __syncthreads();
  // value and status as rvs_chisq_point forms them
  const double lz = AG.wbase[2ll * S.S * npix + 2 * s];
  const bool ok = sh.fact[1] != 0.0;
  double chi = 2.0 * sh.fact[0] + 2.0 * lz + sh.red[0][0];
  int st = st_extra;
  const double xa = AG.lam[0] * f, xb = AG.lam[npix - 1] * f;
  if (xa < x0 || xb < x0 || xa >= xlast || xb >= xlast) {
    st |= RVS_ST_SPLINE_RANGE;
    chi = __builtin_nan("");
  }
  if (!ok) st |= RVS_ST_CHOL_FALLBACK;
  if (!ok || !(fabs(chi) <= 1.79e308)) {
    st |= RVS_ST_NONFINITE;
    chi = __builtin_nan("");
  }
  if (tid == 0) {
    armchi[o] = chi;
    armst[o] = st;
    armout[o] = outside;
  }
  if (tid < K) {
    // columns: vel, the parameters in library order (exactly 0 in the nearest-neighbour
    // modes), vsini (exactly 0 in the FIR's copy branches)
    const int src = (tid == 0) ? 1 : (tid <= nd ? 1 + tid : 2 + OG_MAXDIM);
    armgrad[o * K + tid] = (chi == chi) ? sh.red[0][src] : __builtin_nan("");
  }
}

// arms summed in order; the penalties of A11 (spec_fit.py:888-896) on the value only
__global__ void objective_grad_sum_kernel(int narm, int J, int K, double badchi,
                                          double4 bconst,
                                          const double *__restrict__ pen_scale,
                                          const int32_t *__restrict__ job_spec,
                                          const double *__restrict__ armchi,
                                          const double *__restrict__ armgrad,
                                          const int32_t *__restrict__ armst,
                                          const double *__restrict__ armout,
                                          double *__restrict__ out,
                                          double *__restrict__ grad,
                                          int32_t *__restrict__ status) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= J) return;
  if (pen_scale) badchi *= pen_scale[job_spec ? job_spec[j] : j];
  const double bc[RVS_MAX_ARMS] = {bconst.x, bconst.y, bconst.z, bconst.w};
  double tot = 0;
  double g[OG_MAXK];
#pragma unroll
  for (int i = 0; i < OG_MAXK; i++) g[i] = 0;
  int st = 0;
#pragma unroll
  for (int ia = 0; ia < RVS_MAX_ARMS; ia++) {
    if (ia >= narm) break;
    const int64_t o = (int64_t)ia * J + j;
    const double ov = armout[o];
    if (!(fabs(ov) <= 1.79e308)) {
      tot += 1000.0 * badchi;
      continue;
    }
    tot += armchi[o] + bc[ia] + ov * badchi;
    st |= armst[o];
#pragma unroll
    for (int i = 0; i < OG_MAXK; i++)
      if (i < K) g[i] += armgrad[o * K + i];
  }
  out[j] = tot;
#pragma unroll
  for (int i = 0; i < OG_MAXK; i++)
    if (i < K) grad[(int64_t)j * K + i] = g[i];
  if (st) atomicOr(&status[j], st);
}

}  // namespace

// What the kernel covers, in host arithmetic only: npoly 1..10 (beyond, the value
// kernel's wave totals live in the template buffer), grids of up to 4 dimensions, a
// template grid whose three buffers fit LDS beside the kernel's static part, and the
// pixels twice in one buffer (the sigma-scaled pair; then the pixel adjoint with the
// first-pixel table of ntp int32 behind it: npix + ntp / 2 <= ntp).
extern "C" int rvs_objective_grad_ok(int npoly, int npix, int ntp, int ndim,
                                     int vsini_grad) {
  if (npoly < 1 || npoly > OG_MAXP || npix < 1 || ntp < 32 ||
      ntp > RVS_OBJ_FT_MAX_NTP)
    return 0;
  if (ndim < 1 || ndim > OG_MAXDIM || vsini_grad < 0 || vsini_grad > 1) return 0;
  if (2 * (int64_t)npix > ntp) return 0;
  if (3 * (int64_t)ntp * (int64_t)sizeof(double) + OG_STATIC_MAX > OG_LDS_MAX) return 0;
  return 1;
}

// per (arm, job): chi^2, outside, 1 + ntan gradient entries, status (padded to 8 bytes)
extern "C" int64_t rvs_objective_grad_work_size(int J, int narm, int ntan) {
  if (J < 1 || narm < 1 || narm > RVS_MAX_ARMS || ntan < 1 || ntan > OG_MAXDIM + 1)
    return 0;
  return (int64_t)narm * J * (int64_t)((4 + ntan) * sizeof(double));
}

extern "C" int rvs_objective_grad(const rvs_objective_arm *arms, int narm, int npoly,
                                  int ntan, const double *params, const double *vsini,
                                  const int32_t *job_spec, int J, const double *vel,
                                  double badchi, const double *basis_const,
                                  void *scratch, double *out, double *grad,
                                  int32_t *status, void *stream) {
  if (J < 1 || narm < 1 || narm > RVS_MAX_ARMS || !arms || !params || !vel ||
      !scratch || !out || !grad || !status || npoly < 1 || npoly > OG_MAXP ||
      ntan < 1 || ntan > OG_MAXDIM + 1)
    return RVS_E_ARG;
  static_assert(RVS_MAX_ARMS == 4, "basis constants travel as a double4");
  const int ndim = arms[0].ndim;
  // ntan = ndim: vel and the parameters; ndim + 1: vsini fitted, its column last
  const int vsini_grad = (ntan == ndim + 1) ? 1 : 0;
  if (ntan != ndim + vsini_grad || (vsini_grad && !vsini)) return RVS_E_ARG;
  ObjArms A;
  A.n = narm;
  double bc[RVS_MAX_ARMS] = {0, 0, 0, 0};
  size_t shm = 0;
  for (int i = 0; i < narm; i++) {
    const rvs_objective_arm &a = arms[i];
    if (a.ndim != ndim || a.pt.fast_interp || a.pt.taps || a.pt.G > 1 || !a.factors ||
        !a.dats || !a.idgrid || !a.uvecs || !a.vecs_s || a.pt.ntp != a.ntp ||
        !rvs_objective_grad_ok(npoly, a.pt.npix, a.ntp, ndim, vsini_grad))
      return RVS_E_ARG;
    A.a[i] = a;
    if (basis_const) bc[i] = basis_const[i];
    shm = max(shm, (size_t)3 * a.ntp * sizeof(double));
  }
  for (int i = narm; i < RVS_MAX_ARMS; i++) A.a[i] = arms[0];
  hipStream_t st = rvs_stream(stream);
  const int K = 1 + ntan;
  double *armchi = (double *)scratch;
  double *armout = armchi + (int64_t)narm * J;
  double *armgrad = armout + (int64_t)narm * J;
  int32_t *armst = (int32_t *)(armgrad + (int64_t)narm * J * K);
  dim3 grid(J, narm);
#define RVS_CASE(PP)                                                              \
  case PP: {                                                                      \
    static bool attr_set = false;                                                 \
    if (!attr_set) {                                                              \
      (void)hipFuncSetAttribute((const void *)objective_grad_kernel<PP>,          \
                                hipFuncAttributeMaxDynamicSharedMemorySize,       \
                                OG_LDS_MAX - (int)sizeof(OgShared<PP>));          \
      (void)hipGetLastError();                                                    \
      attr_set = true;                                                            \
    }                                                                             \
    hipLaunchKernelGGL(objective_grad_kernel<PP>, grid, dim3(OG_NT), shm, st, A,  \
                       params, vsini, vsini_grad, job_spec, J, vel, 0.6, armchi,  \
                       armgrad, armst, armout);                                   \
  } break;
  switch (npoly) {
    RVS_CASE(1) RVS_CASE(2) RVS_CASE(3) RVS_CASE(4) RVS_CASE(5)
    RVS_CASE(6) RVS_CASE(7) RVS_CASE(8) RVS_CASE(9) RVS_CASE(10)
    default:
      return RVS_E_ARG;
  }
#undef RVS_CASE
  hipLaunchKernelGGL(objective_grad_sum_kernel, dim3((J + 255) / 256), dim3(256), 0, st,
                     narm, J, K, badchi, make_double4(bc[0], bc[1], bc[2], bc[3]),
                     arms[0].pt.pen_scale, job_spec, armchi, armgrad, armst, armout, out,
                     grad, status);
  RVS_LAUNCH_CHECK();
  return 0;
}
