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
// arithmetic of the stand-alone kernels they replace.  Cell, gather and guard, rotational
// kernel, FIR and spline construct are objective_point_dev.h's, shared with
// objective_fisher.hip, as are the host side and the sum over the arms; the passes over
// the pixels are this kernel's own text.
#include "objective_point_dev.h"

namespace {

template <int P>
using OgShared = OpShared<P, (op_nv(P) > OP_MAXK + 1 ? op_nv(P) : OP_MAXK + 1)>;

// FROMT (rvs_objective_grad_from_template): the unbroadened template of a
// (job, arm) is a row an evaluator that is no grid gather left in HBM (the MLP of
// rvs_template_nn), with its outside flag, as objective_kernel<P, true> takes it.  There is
// no cell and no contraction at the knots: the adjoint row tbar = d chi^2 / d t goes to HBM
// as it stands in LDS behind the transposed FIR -- the row the evaluator's own reverse
// pass contracts with its Jacobian -- and the gradient has the velocity and, with vsini
// fitted, the vsini column.  Everything between is the text below, unchanged.
struct OgNoTempl {};
struct OgTempl {
  const double *templ[RVS_MAX_ARMS];    // [J, ntp] per arm
  const double *outside[RVS_MAX_ARMS];  // [J] per arm
  double *tbar[RVS_MAX_ARMS];           // [J, ntp] per arm
};

// RESOL (rvs_objective_grad_resol, rvs_objective_grad_from_template_resol): arms
// with a banded resolution matrix of nd <= 33 diagonals (rvs_point_arm.taps), applied in
// LDS as objective_kernel<.., RESOL> applies it, and its transpose applied to the one
// adjoint row.  The third buffer then holds
//   F[0, npix)                     m/e of the model pass; behind the transposed band rawbar
//   PAD = F + npix: [hb zeros] [npix: raw, from pass 2 on mbar] [hb zeros],  hb = (nd - 1) / 2
// (the data column D/e is read from sig[k].y, the same double), and the first-pixel table
// lies over PAD once the transposed band has read it: 2 npix + nd - 1 <= ntp
// (rvs_objective_grad_resol_ok).
//   model pass   raw[k] -> PAD[hb + k]; barrier; m_k = sum_d taps[s, k, d] PAD[k + d], d
//                ascending: the products of resolution_band (objective.hip) in its order
//   pass 2       mbar_k -> PAD[hb + k] (the pads stay zero); barrier
//   band^T       rawbar_j = sum_d taps[s, j + hb - d, d] PAD[j + 2 hb - d], d ascending,
//                threads = pixels: stride nd - 1 in taps; a row outside [0, npix) meets a
//                loaded zero (its tap is read from the nearest row inside), no atomic
//   velocity     gvel = sum_j rawbar_j S'(x_j) lam_j df/dvel: behind the band, so y and z
//                stay live until here
// and from there on rawbar is what mbar is without a matrix.  An arm without a matrix
// beside arms that have one is a band of one diagonal.
template <int P, bool FROMT = false, bool RESOL = false>
__global__ void __launch_bounds__(OP_NT)
    objective_grad_kernel(ObjArms A, const double *__restrict__ params,
                          const double *__restrict__ vsini, int vsini_grad,
                          const int32_t *__restrict__ job_spec, int J,
                          const double *__restrict__ vel, double eps_ld,
                          double *__restrict__ armchi, double *__restrict__ armgrad,
                          int32_t *__restrict__ armst, double *__restrict__ armout,
                          std::conditional_t<FROMT, OgTempl, OgNoTempl> TT) {
  static_assert(sizeof(OgShared<P>) <= OP_STATIC_MAX, "op_point_ok's bound");
  extern __shared__ double lds[];
  __shared__ OgShared<P> sh;
  const int j = blockIdx.x;
  const int64_t o = obj_out_index(J, j);
  ObjPoint<P, OgShared<P>::REDW> pt(sh, A.a[blockIdx.y], lds, j, eps_ld);
  const rvs_objective_arm &T = pt.T;
  const PolyLoc &PL = pt.PL;
  const int tid = pt.tid, lane = pt.lane, w = pt.w;
  const int N = pt.N, m = pt.m, nd = FROMT ? 0 : pt.nd, nv = pt.nv;
  const int K = 1 + nd + (vsini_grad ? 1 : 0);
  constexpr int NTR = P * (P + 1) / 2;
  constexpr int NV = NTR + P;
  // FROMT: this (job, arm)'s template row and the row its adjoint goes to
  const double *trow = nullptr;
  double *tbrow = nullptr;

  // ---- cell, gather and guard, rotational kernel, FIR, spline construct ---------------------
  // (objective_point_dev.h, shared with objective_fisher_kernel) hands over: PL, sh.dw,
  // sh.jobsc, mode, nrow, outside; kmax, R, copy, st_extra; Y, Z, F; the chunk tables
  if constexpr (FROMT) {
    trow = TT.templ[blockIdx.y] + (int64_t)j * N;
    tbrow = TT.tbar[blockIdx.y] + (int64_t)j * N;
    pt.template_row(trow, TT.outside[blockIdx.y][j], vel);
  } else {
    pt.cell(params, vel);
    pt.gather_and_guard();
  }
  if (obj_template_unusable(pt.outside)) {
    obj_store_skipped(o, armchi, armst, armout);
    if (tid < K) armgrad[o * K + tid] = 0.0;
    if constexpr (FROMT)   // (a skipped arm adds nothing to the parameters' gradient)
      for (int n = tid; n < N; n += OP_NT) tbrow[n] = 0.0;
    return;
  }
  pt.rotational_kernel(vsini);
  pt.fir();
  const int mode = pt.mode, kmax = pt.kmax, st_extra = pt.st_extra;
  const float *nrow = pt.nrow;
  const double outside = pt.outside, R = pt.R;
  const bool copy = pt.copy;
  double *Y = pt.Y, *Z = pt.Z, *F = pt.F;
  pt.spline_chunks();
  pt.spline_construct();
  __syncthreads();

  // From here to the end of pass 2 this kernel keeps its own text: through ObjPoint's
  // model_pass, normal_equations, solve and pixel_adjoint -- the statements
  // objective_fisher_kernel runs, and faster there -- grad_ab.py --fused --vsini-grad
  // measured 17.80 ms against 17.48 (spread 0.05); with these passes its own 17.50
  // (DESIGN 4.24).  A change to one of them is a change to the other.
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
  // RESOL: the band of this spectrum, the padded row (see above)
  const int rnd = (RESOL && S.taps) ? S.nd : 1, hb = (rnd - 1) >> 1;
  const double *tps = (RESOL && S.taps) ? S.taps + (int64_t)s * S.taps_stride : nullptr;
  double *PAD = F + npix;
  if (RESOL && tid < hb) {
    PAD[tid] = 0.0;
    PAD[hb + npix + tid] = 0.0;
  }
  // (a loop of its own, which holds no accumulators, as in objective_kernel)
  for (int k = tid; k < npix; k += OP_NT) {
    const int pos = pix_pos(k);
    const double dl = AG.lam[k] * f - S.knots[pos];
    const double tv = obj_piece_value(piece(pos), dl);
    if constexpr (RESOL) {
      PAD[hb + k] = tv;
    } else {
      const double2 sg = sig[k];
      F[k] = tv * sg.x;
      F[npix + k] = sg.y;
    }
  }
  if constexpr (RESOL) {
    // ---- resolution band (A9): m_k = sum_d taps[s, k, d] raw[k - hb + d], then m/e ----------
    __syncthreads();
    for (int k = tid; k < npix; k += OP_NT) {
      const double *rk = PAD + k;   // raw[k - hb]
      double a = rk[0];
      if (tps) {
        const double *tk = tps + (int64_t)k * rnd;
        a = 0;
        for (int d = 0; d < rnd; d++) a = fma(tk[d], rk[d], a);
      }
      F[k] = a * sig[k].x;
    }
  }
  // ---- normal equations (A10): the sums per lane, waves' totals into sh.red ---------------
  {
    double vals[NV];   // [NTR] packed lower triangle, then [P] right-hand sides
#pragma unroll
    for (int i = 0; i < NV; i++) vals[i] = 0;
    for (int k = tid; k < npix; k += OP_NT) {
      // (written by this same thread; RESOL: the data column from the pixel's record)
      const double te = F[k], dk = RESOL ? sig[k].y : F[npix + k];
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
    for (int q = 1; q < OP_NW; q++) v += sh.red[q][tid];
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
  for (int k = tid; k < npix; k += OP_NT) {
    const double te = F[k], dk = RESOL ? sig[k].y : F[npix + k];
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
    if constexpr (RESOL) {
      PAD[hb + k] = mbar;
    } else {
      const int pos = pix_pos(k);
      const double lamk = AG.lam[k];
      const double dl = lamk * f - S.knots[pos];
      const double dtv = obj_piece_deriv(piece(pos), dl);
      gvel = fma(mbar, dtv * (lamk * dfdv), gvel);
      F[k] = mbar;
    }
  }
  if constexpr (RESOL) {
    // ---- resolution band, transposed: rawbar = R^T mbar; the velocity component ---------------
    // hands over: gvel; rawbar in F[0, npix)
    __syncthreads();
    for (int k = tid; k < npix; k += OP_NT) {
      const double *mk = PAD + k + 2 * hb;   // mbar[k + hb]
      double rawbar = mk[0];
      if (tps) {
        rawbar = 0;
        for (int d = 0; d < rnd; d++) {
          const int row = min(max(k + hb - d, 0), npix - 1);
          rawbar = fma(tps[(int64_t)row * rnd + d], mk[-d], rawbar);
        }
      }
      const int pos = pix_pos(k);
      const double lamk = AG.lam[k];
      const double dl = lamk * f - S.knots[pos];
      const double dtv = obj_piece_deriv(piece(pos), dl);
      gvel = fma(rawbar, dtv * (lamk * dfdv), gvel);
      F[k] = rawbar;
    }
  }
  __syncthreads();   // y, z and the data column of F (RESOL: the padded row) are dead

  // ---- resampling, transposed -------------------------------------------------------
  // first[n] = the number of pixels in intervals below n (pixels ascend in wavelength,
  // so the pixels of interval n are [first[n], first[n + 1])); every entry is written
  // once, by the first pixel at or behind it
  int32_t *first = reinterpret_cast<int32_t *>(F + npix);
  for (int k = tid; k <= npix; k += OP_NT) {
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
  for (int n = tid; n < N; n += OP_NT) {
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
  pt.tri_solve([&](int u, double, double) { return Zb[u]; }, Zb);
  __syncthreads();
  // sl_j = 6 (u_{j-1} - u_j), u_j at knot j + 1, 0 beyond both ends;
  // ybar_{j+1} += sl_j / h_j, ybar_j -= sl_j / h_j
  {
    auto U = [&](int i) { return (i >= 0 && i < m) ? Zb[i] : 0.0; };
    for (int n = tid; n < N; n += OP_NT) {
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
    obj_build_taps<OP_NT, false>(kmax, R, eps_ld, T.lnstep, Zb, F, vs_grad ? F + kmax + 1 : nullptr,
                          sh.red8);
    for (int i = tid; i < N; i += OP_NT) Zb[i] = pt.fir_at(Yb, F, i);
    tbar = Zb;
    dwt = F + kmax + 1;
    __syncthreads();
  }

  // ---- contraction at the knots -----------------------------------------------------
  double gp[OP_MAXDIM], gvs = 0;
#pragma unroll
  for (int d = 0; d < OP_MAXDIM; d++) gp[d] = 0;
  if constexpr (FROMT) {
    // tbar to HBM, coalesced (every thread the knots it wrote); with vsini fitted
    // vbar_n t_n with t_n read again from the template row: t is dead in LDS
    for (int n = tid; n < N; n += OP_NT) {
      tbrow[n] = tbar[n];
      if (vs_grad) gvs = fma(pt.fir_at(Yb, dwt, n), trow[n], gvs);
    }
  }
  for (int n = tid; !FROMT && n < N; n += OP_NT) {
    double tn;
    if (mode == 0) {
      double a = 0, g[OP_MAXDIM];
#pragma unroll
      for (int d = 0; d < OP_MAXDIM; d++) g[d] = 0;
      for (int v = 0; v < nv; v++) {
        const double Lv = (double)T.dats[PL.id[v] * N + n];
        a = fma(PL.w[v], Lv, a);
#pragma unroll
        for (int d = 0; d < OP_MAXDIM; d++)
          if (d < nd) g[d] = fma(sh.dw[d * nv + v], Lv, g[d]);
      }
      tn = T.exp_flag ? exp(a) : a;
      const double tb = tbar[n];
#pragma unroll
      for (int d = 0; d < OP_MAXDIM; d++)
        if (d < nd) gp[d] = fma(tb, T.exp_flag ? tn * g[d] : g[d], gp[d]);
    } else {
      tn = T.exp_flag ? (double)np_expf(nrow[n]) : (double)nrow[n];
    }
    if (vs_grad) gvs = fma(pt.fir_at(Yb, dwt, n), tn, gvs);
  }

  // ---- tail: the block's sums (lanes by butterfly, waves in order), value and status --------
  {
    double fin[OP_MAXK + 1];
    fin[0] = rr;
    fin[1] = gvel;
#pragma unroll
    for (int d = 0; d < OP_MAXDIM; d++) fin[2 + d] = gp[d];
    fin[2 + OP_MAXDIM] = gvs;
#pragma unroll
    for (int i = 0; i <= OP_MAXK; i++) {
      const double v = wave_sum(fin[i]);
      if (lane == 0) sh.red[w][i] = v;
    }
  }
  __syncthreads();
  if (tid <= OP_MAXK) {
    double v = sh.red[0][tid];
#pragma unroll
    for (int q = 1; q < OP_NW; q++) v += sh.red[q][tid];
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
    const int src = (tid == 0) ? 1 : (tid <= nd ? 1 + tid : 2 + OP_MAXDIM);
    armgrad[o * K + tid] = (chi == chi) ? sh.red[0][src] : __builtin_nan("");
  }
}

}  // namespace

// (what the kernel covers: op_point_ok)
extern "C" int rvs_objective_grad_ok(int npoly, int npix, int ntp, int ndim,
                                     int vsini_grad) {
  return op_point_ok(npoly, npix, ntp, ndim, vsini_grad);
}

// per (arm, job): chi^2, outside, 1 + ntan gradient entries, status (padded to 8 bytes)
extern "C" int64_t rvs_objective_grad_work_size(int J, int narm, int ntan) {
  if (J < 1 || narm < 1 || narm > RVS_MAX_ARMS || ntan < 1 || ntan > OP_MAXDIM + 1)
    return 0;
  return (int64_t)narm * J * (int64_t)((4 + ntan) * sizeof(double));
}

// What the kernel covers under a resolution matrix of nd diagonals, the one statement of
// the condition (host arithmetic only): nd odd, 1 .. 33; everything op_point_ok asks (ndim
// = 0: the from-template form, which reads no cell -- op_geometry_ok); and the LDS layout
// of objective_grad_kernel<.., RESOL>: the third buffer of ntp doubles holds m/e in
// [0, npix) and behind it the padded row [hb zeros][npix][hb zeros], hb = (nd - 1) / 2, so
//   npix + (npix + nd - 1) <= ntp.
// The first-pixel table ((ntp + 1) / 2 doubles behind rawbar in [0, npix)) lies over the
// padded row once the transposed band has read it: npix + (ntp + 1) / 2 <= ntp already
// follows from 2 npix <= ntp.
extern "C" int rvs_objective_grad_resol_ok(int npoly, int npix, int ntp, int ndim, int nd,
                                           int vsini_grad) {
  if (ndim < 0 || ndim > OP_MAXDIM) return 0;
  return op_resol_geometry_ok(npoly, npix, ntp, nd, vsini_grad);
}

namespace {
int objective_grad_call(bool resol, const rvs_objective_arm *arms, int narm, int npoly,
                        int ntan, const double *params, const double *vsini,
                        const int32_t *job_spec, int J, const double *vel, double badchi,
                        const double *basis_const, void *scratch, double *out,
                        double *grad, int32_t *status, void *stream) {
  OpCall c;
  if (J < 1 || !params || !vel || !scratch || !out || !grad || !status ||
      !op_check_arms(arms, narm, npoly, ntan, vsini, basis_const, c, resol))
    return RVS_E_ARG;
  hipStream_t st = rvs_stream(stream);
  const int K = 1 + ntan;
  double *armchi = (double *)scratch;
  double *armout = armchi + (int64_t)narm * J;
  double *armgrad = armout + (int64_t)narm * J;
  int32_t *armst = (int32_t *)(armgrad + (int64_t)narm * J * K);
  op_for_npoly(npoly, [&](auto p) {
    constexpr int PP = decltype(p)::value;
    if (resol)
      op_launch<objective_grad_kernel<PP, false, true>, (int)sizeof(OgShared<PP>)>(
          dim3(J, narm), c.shm, st, c.A, params, vsini, c.vsini_grad, job_spec, J, vel,
          0.6, armchi, armgrad, armst, armout, OgNoTempl());
    else
      op_launch<objective_grad_kernel<PP>, (int)sizeof(OgShared<PP>)>(
          dim3(J, narm), c.shm, st, c.A, params, vsini, c.vsini_grad, job_spec, J, vel,
          0.6, armchi, armgrad, armst, armout, OgNoTempl());
  });
  hipLaunchKernelGGL(objective_point_sum_kernel, dim3((J + 255) / 256), dim3(256), 0, st,
                     narm, J, 0, K, badchi, c.bc, arms[0].pt.pen_scale, job_spec, armchi,
                     armgrad, nullptr, armst, armout, out, grad, nullptr, status);
  RVS_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int rvs_objective_grad(const rvs_objective_arm *arms, int narm, int npoly,
                                  int ntan, const double *params, const double *vsini,
                                  const int32_t *job_spec, int J, const double *vel,
                                  double badchi, const double *basis_const,
                                  void *scratch, double *out, double *grad,
                                  int32_t *status, void *stream) {
  return objective_grad_call(false, arms, narm, npoly, ntan, params, vsini, job_spec, J,
                             vel, badchi, basis_const, scratch, out, grad, status, stream);
}

// ... with the arms' resolution matrices (pt.taps / pt.nd) applied: the RESOL form of the
// kernel; scratch as for rvs_objective_grad
extern "C" int rvs_objective_grad_resol(const rvs_objective_arm *arms, int narm, int npoly,
                                        int ntan, const double *params,
                                        const double *vsini, const int32_t *job_spec,
                                        int J, const double *vel, double badchi,
                                        const double *basis_const, void *scratch,
                                        double *out, double *grad, int32_t *status,
                                        void *stream) {
  return objective_grad_call(true, arms, narm, npoly, ntan, params, vsini, job_spec, J,
                             vel, badchi, basis_const, scratch, out, grad, status, stream);
}

// ---- the from-template form ---------------------------------------------------
// (op_point_ok without the ndim bound of the cell record: the kernel reads no cell)
extern "C" int rvs_objective_grad_from_template_ok(int npoly, int npix, int ntp,
                                                   int vsini_grad) {
  return op_geometry_ok(npoly, npix, ntp, vsini_grad);
}

// per (arm, job): chi^2, outside, 1 + vsini_grad gradient entries, status (padded to 8
// bytes)
extern "C" int64_t rvs_objective_grad_from_template_work_size(int J, int narm,
                                                              int vsini_grad) {
  if (J < 1 || narm < 1 || narm > RVS_MAX_ARMS || vsini_grad < 0 || vsini_grad > 1)
    return 0;
  return (int64_t)narm * J * (int64_t)((4 + vsini_grad) * sizeof(double));
}

namespace {
int objective_grad_from_template_call(
    bool resol, const rvs_objective_arm *arms, int narm, int npoly, int vsini_grad,
    const double *const *templ, const double *const *outside, const double *vsini,
    const int32_t *job_spec, int J, const double *vel, double badchi,
    const double *basis_const, void *scratch, double *const *tbar, double *out,
    double *grad, int32_t *status, void *stream) {
  OpCall c;
  if (J < 1 || !templ || !outside || !tbar || !vel || !scratch || !out || !grad ||
      !status ||
      !op_check_arms_templ(arms, narm, npoly, vsini_grad, vsini, basis_const, c, resol))
    return RVS_E_ARG;
  OgTempl tt = {};
  for (int i = 0; i < RVS_MAX_ARMS; i++) {
    const int a = i < narm ? i : 0;
    if (!templ[a] || !outside[a] || !tbar[a]) return RVS_E_ARG;
    tt.templ[i] = templ[a];
    tt.outside[i] = outside[a];
    tt.tbar[i] = tbar[a];
  }
  hipStream_t st = rvs_stream(stream);
  const int K = 1 + vsini_grad;
  double *armchi = (double *)scratch;
  double *armout = armchi + (int64_t)narm * J;
  double *armgrad = armout + (int64_t)narm * J;
  int32_t *armst = (int32_t *)(armgrad + (int64_t)narm * J * K);
  op_for_npoly(npoly, [&](auto p) {
    constexpr int PP = decltype(p)::value;
    if (resol)
      op_launch<objective_grad_kernel<PP, true, true>, (int)sizeof(OgShared<PP>)>(
          dim3(J, narm), c.shm, st, c.A, (const double *)nullptr, vsini, c.vsini_grad,
          job_spec, J, vel, 0.6, armchi, armgrad, armst, armout, tt);
    else
      op_launch<objective_grad_kernel<PP, true>, (int)sizeof(OgShared<PP>)>(
          dim3(J, narm), c.shm, st, c.A, (const double *)nullptr, vsini, c.vsini_grad,
          job_spec, J, vel, 0.6, armchi, armgrad, armst, armout, tt);
  });
  hipLaunchKernelGGL(objective_point_sum_kernel, dim3((J + 255) / 256), dim3(256), 0, st,
                     narm, J, 0, K, badchi, c.bc, arms[0].pt.pen_scale, job_spec, armchi,
                     armgrad, nullptr, armst, armout, out, grad, nullptr, status);
  RVS_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int rvs_objective_grad_from_template(
    const rvs_objective_arm *arms, int narm, int npoly, int vsini_grad,
    const double *const *templ, const double *const *outside, const double *vsini,
    const int32_t *job_spec, int J, const double *vel, double badchi,
    const double *basis_const, void *scratch, double *const *tbar, double *out,
    double *grad, int32_t *status, void *stream) {
  return objective_grad_from_template_call(false, arms, narm, npoly, vsini_grad, templ,
                                           outside, vsini, job_spec, J, vel, badchi,
                                           basis_const, scratch, tbar, out, grad, status,
                                           stream);
}

// ... with the arms' resolution matrices applied: the adjoint row behind the
// transposed band; scratch as for rvs_objective_grad_from_template
extern "C" int rvs_objective_grad_from_template_resol(
    const rvs_objective_arm *arms, int narm, int npoly, int vsini_grad,
    const double *const *templ, const double *const *outside, const double *vsini,
    const int32_t *job_spec, int J, const double *vel, double badchi,
    const double *basis_const, void *scratch, double *const *tbar, double *out,
    double *grad, int32_t *status, void *stream) {
  return objective_grad_from_template_call(true, arms, narm, npoly, vsini_grad, templ,
                                           outside, vsini, job_spec, J, vel, badchi,
                                           basis_const, scratch, tbar, out, grad, status,
                                           stream);
}

// ---- the sum over the arms of the evaluator's reverse pass --------------------------------
// grad [J, 1 + ndim + vsini_grad] = (vel, parameters, vsini) from the from-template call's
// own gradient [J, 1 + vsini_grad] and the arms' gparams [J, ndim] (rvs_template_nn_vjp of
// the arm's tbar rows), arms in order.  An arm whose outside flag -- read from the
// from-template call's scratch -- is not finite adds exactly nothing; where the value is
// NaN so are the parameters' components; the penalties are on the value only.
namespace {
struct OgJoin {
  const double *gparams[RVS_MAX_ARMS];
};
__global__ void objective_grad_join_kernel(int narm, int J, int ndim, int vg,
                                           const double *__restrict__ armout, OgJoin G,
                                           const double *__restrict__ out,
                                           const double *__restrict__ gvv,
                                           double *__restrict__ grad) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= J) return;
  const int K2 = 1 + vg, K = 1 + ndim + vg;
  const double chi = out[j];
  bool counts[RVS_MAX_ARMS];
#pragma unroll
  for (int ia = 0; ia < RVS_MAX_ARMS; ia++)
    counts[ia] = ia < narm && fabs(armout[(int64_t)min(ia, narm - 1) * J + j]) <= 1.79e308;
  grad[(int64_t)j * K] = gvv[(int64_t)j * K2];
  for (int d = 0; d < ndim; d++) {
    double v = 0;
#pragma unroll
    for (int ia = 0; ia < RVS_MAX_ARMS; ia++)
      if (counts[ia]) v += G.gparams[ia][(int64_t)j * ndim + d];
    grad[(int64_t)j * K + 1 + d] = (chi == chi) ? v : __builtin_nan("");
  }
  if (vg) grad[(int64_t)j * K + 1 + ndim] = gvv[(int64_t)j * K2 + 1];
}
}  // namespace

extern "C" int rvs_objective_grad_join(int narm, int J, int ndim, int vsini_grad,
                                       const void *scratch, const double *const *gparams,
                                       const double *out, const double *grad_vv,
                                       double *grad, void *stream) {
  if (narm < 1 || narm > RVS_MAX_ARMS || J < 1 || ndim < 1 || ndim > 8 || vsini_grad < 0 ||
      vsini_grad > 1 || !scratch || !gparams || !out || !grad_vv || !grad)
    return RVS_E_ARG;
  OgJoin G = {};
  for (int i = 0; i < RVS_MAX_ARMS; i++) {
    G.gparams[i] = gparams[i < narm ? i : 0];
    if (!G.gparams[i]) return RVS_E_ARG;
  }
  // (the layout of rvs_objective_grad_from_template's scratch: [narm, J] values, then flags)
  const double *armout = (const double *)scratch + (int64_t)narm * J;
  hipLaunchKernelGGL(objective_grad_join_kernel, dim3((J + 255) / 256), dim3(256), 0,
                     rvs_stream(stream), narm, J, ndim, vsini_grad, armout, G, out, grad_vv,
                     grad);
  RVS_LAUNCH_CHECK();
  return 0;
}
