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
  const int64_t o = obj_out_index(J, j);
  double *B0 = lds, *B1 = lds + N, *B2 = lds + 2 * (int64_t)N;
  PolyLoc &PL = sh.PL;

  // ---- the grid cell: cell search, dw/dp, the job's Doppler scalars -------------------------
  // hands over: PL, mode, sh.dw, sh.jobsc
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

  // ---- gather (A3/A5): the template into B0 -------------------------------------------------
  // hands over: B0; for the template guard every thread's {mx, anynan} of a nearest row
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
      obj_guard_scan(val, mx, anynan);
    }
    // ---- template guard ---------------------------------------------------------------------
    // hands over: `outside`, the arm's penalty term
    outside = obj_template_guard<OG_NW>(mx, anynan, &PL.dist, sh.red8);
  }
  __syncthreads();
  if (obj_template_unusable(outside)) {
    obj_store_skipped(o, armchi, armst, armout);
    if (tid < K) armgrad[o * K + tid] = 0.0;
    return;
  }

  // ---- rotational kernel ----------------------------------------------------------------------
  // hands over: kmax (0: `copy`, no FIR), R, st_extra; the taps are built where they are used
  bool refused = false;
  int kmax = 0;
  double R = 0;
  if (vsini) kmax = obj_rot_kmax(T, vsini[j], R, refused);
  const bool copy = kmax == 0;
  const int st_extra = refused ? RVS_ST_NONFINITE : 0;
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

  // ---- FIR (A6): y = w (*) t ----------------------------------------------------------------
  // Y, Z: the buffers of y and z; F: the third one (taps, then the pixel pair)
  double *Y = B0, *Z = B1, *F = B2;
  if (!copy) {
    obj_build_taps<OG_NT, false>(kmax, R, eps_ld, T.lnstep, B1, B2, nullptr, sh.red8);
    for (int i = tid; i < N; i += OG_NT) B1[i] = fir_at(B0, B2, i);
    Y = B1;
    Z = B0;
    __syncthreads();
  }

  // ---- spline construct (A7): the natural spline's tridiagonal solve ------------------------
  // hands over: Z (second derivatives of Y)
  // Thread t owns the rows [a0, a1) (CH of them) of the m unknowns; the chunks are joined
  // by obj_chain3 (barriers between the two solves).  The factors are the chunk-ordered
  // copy of rvs_spline_factors: record {1/h_u, 1/h_{u+1}, g_u, e_u} of row t CH + q at
  // [q][t], then the backward multipliers in pairs.
  const int CH = rvs_obj_chunk_len(m);
  const int a0 = min(m, tid * CH), a1 = min(m, a0 + CH);
  const double *FT = T.factors + 5 * (int64_t)N;
  const double *FC = FT + 4 * (int64_t)OG_NT * OG_CHMAX;
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
    const double d_in = obj_chain3<OG_NW>(sh.edge, d, pb, -1);
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
    const double z_in = obj_chain3<OG_NW>(sh.edge, z, pb, +1);
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

  // ---- model pass (A7 eval): the pixels' spline values -------------------------------------
  // hands over: F ([npix] m/e, [npix] D/e)
  const rvs_point_arm &S = T.pt;
  const int npix = S.npix;
  const int s = job_spec ? job_spec[j] : j;
  const ObjArmGrid AG = obj_arm_grid(S, s);
  const double2 *sig = AG.sig;   // {1/e, D/e} of the spectrum's pixels
  const double xlast = S.knots[N - 1];
  const double *hh = T.factors + 3 * (int64_t)N, *ih = T.factors + 4 * (int64_t)N;
  const ObjKnotMap KM = {S.log_step, N, sh.jobsc[0], sh.jobsc[1], sh.jobsc[2], S.knots[0]};
  const double f = KM.f;
  // The knot interval and the spline piece in this kernel's own spelling: through
  // obj_knot_interval / obj_piece the same arithmetic measured 0.6 % slower per call
  // (DESIGN 4.22); the value and the derivative of the piece are the shared ones.
  const double shift = KM.shift, lin_inv_step = KM.lin_inv_step, x0 = KM.x0;
  auto pix_pos = [&](int k) {   // (obj_knot_interval)
    int pos = S.log_step ? (int)(AG.pix[k] + shift)
                         : (int)((AG.lam[k] * f - x0) * lin_inv_step);
    return min(max(pos, 0), N - 2);
  };
  auto piece = [&](int pos) {   // (obj_piece)
    ObjPiece p;
    const double h = hh[pos], hinv = ih[pos];
    const double zi = (pos == 0) ? 0.0 : Z[pos - 1];
    const double zi1 = (pos + 1 == N - 1) ? 0.0 : Z[pos];
    const double yi1 = Y[pos + 1];
    p.yi = Y[pos];
    const double t1 = hinv * (1.0 / 6), t2 = h * (1.0 / 6);
    p.cb = (yi1 - p.yi) * hinv - t2 * (2 * zi + zi1);
    p.c2 = 0.5 * zi;
    p.c3 = (zi1 - zi) * t1;
    return p;
  };
  // (a loop of its own, which holds no accumulators, as in objective_kernel)
  for (int k = tid; k < npix; k += OG_NT) {
    const int pos = pix_pos(k);
    const double dl = AG.lam[k] * f - S.knots[pos];
    const double tv = obj_piece_value(piece(pos), dl);
    const double2 sg = sig[k];
    F[k] = tv * sg.x;
    F[npix + k] = sg.y;
  }
  // ---- normal equations (A10): the sums per lane, waves' totals into sh.red ---------------
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
  // ---- solve (A10): Cholesky factor, coefficients, log det ---------------------------------
  // hands over: acc[] (L with 1 / L_ii on the diagonal) and av[] (the coefficients) in
  // every lane's registers; sh.fact
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
  // ---- residual (A11) and the pixel adjoint ---------------------------------------------------
  // hands over: rr, gvel (this thread's shares); mbar in F[0, npix)
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
    const double dtv = obj_piece_deriv(piece(pos), dl);
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
    obj_build_taps<OG_NT, false>(kmax, R, eps_ld, T.lnstep, Zb, F, vs_grad ? F + kmax + 1 : nullptr,
                          sh.red8);
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

  // ---- tail: the block's sums (lanes by butterfly, waves in order), value and status --------
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
  double chi;
  int st;
  obj_value_status(S, AG, s, KM, xlast, sh.fact[0], sh.fact[1] != 0.0, sh.red[0][0], st_extra,
                   chi, st);
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
