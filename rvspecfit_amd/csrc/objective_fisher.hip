// objective_fisher.hip -- the optimiser's objective, its gradient AND the Fisher matrix
// of the marginalised fit at one (template parameters, vsini, velocity) point per job,
// as a single kernel: objective_grad.hip's value phases, then the tangents in FORWARD
// mode.
//
// The adjoint of objective_grad.hip carries one row back from the pixels, which gives
// the gradient and nothing else: the Gauss-Newton matrix F = J^T (1 - U U^T) J needs the
// K = 1 + ntan tangent rows AT the pixels.  The template path (gather, FIR, spline,
// resampling) is linear in the template row, so each tangent row goes through the
// value's own statements, one at a time, in the buffers the value has left.  One
// 512-thread block owns a (job, arm):
//   value        cell, gather, FIR, spline construct, model pass, normal equations,
//                Cholesky factor and solve: objective_grad_kernel's statements (the
//                same value and status)
//   factor       L (1 / L_ii on the diagonal) and the coefficients c to static LDS:
//                no later phase needs them per lane
//   pass 2       residual, the pixel adjoint mbar_k, te_k = m_k / e_k and the velocity
//                tangent m'_k0 = S'(x_k) lam_k df/dvel -> the (job, arm)'s work row
//   (t, y, z and the pixel pair are dead from here on; the taps w, dw/dvsini are built
//    once more, into the third buffer, where they stay)
//   tangent i    parameter d: t'_n = t_n sum_v (dw_v/dp_d) L_vn gathered at the knots as
//                polylinear_kernel<true> forms it, y' = w (*) t', z' by tri_solve, m'_ki
//                by obj_piece_value; vsini (last): y' = dw/dvsini (*) t, t regathered
//   moments i    threads = pixels: J_ki = (c.phi_k) m'_ki / e_k -> work row; the P raw
//                moments B'_pi = sum_k phi_pk te_k J_ki and g_i = sum_k mbar_k m'_ki
//   B = L^-1 B'  K threads, one forward substitution each: by linearity the
//                sum_k y_p(k) te_k J_ki of point_fisher_block, y(k) never formed
//   Gram         threads = pixels: the K (K + 1) / 2 sums G_il = sum_k J_ki J_kl
//   F            K (K + 1) / 2 threads: F_il = G_il - sum_p B_pi B_pl, both halves
// The pixel-side state -- mbar, te and the K columns -- lives in a work row of (K + 2)
// npix doubles in HBM per (job, arm): LDS is full (three template buffers), and the
// thread that owns a pixel (k = tid mod 512) is the only one to write and read it, so
// the accesses are coalesced and need no fence.  No template row, tangent row or spline
// record goes to HBM.  There is no floating point atomic: every sum has a fixed order
// (lanes by wave_halve / wave_sum, waves in order through LDS), so repeated runs,
// permuted job lists and another work size agree to the bit.
#include "objective_dev.h"

#define OF_NT RVS_OBJ_NT
#define OF_NW (OF_NT / 64)
#define OF_CHMAX RVS_OBJ_CHMAX
#define OF_MAXP 10     // as objective_grad.hip: the wave totals' place
#define OF_MAXDIM 4    // the bound of the cell record (OBJ_LOC_NV vertices)
#define OF_MAXK (2 + OF_MAXDIM)   // vel, parameters, vsini
#define OF_NG (OF_MAXK * (OF_MAXK + 1) / 2)   // packed lower triangle of G
// upper bound of the kernel's static LDS (OfShared): what rvs_objective_fisher_ok, host
// arithmetic only, counts beside the three template buffers
#define OF_STATIC_MAX 8192
#define OF_LDS_MAX (160 * 1024)

namespace {

template <int P>
struct OfShared {
  static constexpr int NV = P * (P + 1) / 2 + P;
  PolyLoc PL;
  double dw[OF_MAXDIM << OF_MAXDIM];   // dw_v/dp_d [d][v] (polylinear_kernel<true>)
  double red[OF_NW][(NV > OF_NG ? NV : OF_NG) + 1];
  double edge[2][OF_NW][6];   // chunk coefficients across wave boundaries
  double red8[2 * OF_NW];
  double rrw[OF_NW];          // the waves' shares of the residual norm
  double fact[2];             // log det L, 1: every pivot positive
  double jobsc[3];            // obj_job_scalars
  double Lc[NV];              // L packed (1 / L_ii on the diagonal), then c
  double bp[OF_MAXK][P];      // B'_.i, then B_.i = L^-1 B'_.i
  double g[OF_MAXK];          // g_i
};

// entry t of the packed lower triangle: row i, column l <= i
__device__ __forceinline__ void of_tri_pair(int t, int &i, int &l) {
  i = 0;
  while ((i + 1) * (i + 2) / 2 <= t) i++;
  l = t - i * (i + 1) / 2;
}

// Jl: the jobs of this launch (the stride of the per-arm outputs and work rows); j0:
// the first of them in the caller's arrays
template <int P>
__global__ void __launch_bounds__(OF_NT)
    objective_fisher_kernel(ObjArms A, const double *__restrict__ params,
                            const double *__restrict__ vsini, int vsini_grad,
                            const int32_t *__restrict__ job_spec, int Jl, int j0,
                            const double *__restrict__ vel, double eps_ld,
                            double *__restrict__ wrows, int64_t wstride,
                            double *__restrict__ armchi, double *__restrict__ armgrad,
                            double *__restrict__ armfisher, int32_t *__restrict__ armst,
                            double *__restrict__ armout) {
  constexpr int NTR = P * (P + 1) / 2;
  constexpr int NV = NTR + P;
  static_assert(sizeof(OfShared<P>) <= OF_STATIC_MAX, "rvs_objective_fisher_ok's bound");
  extern __shared__ double lds[];
  __shared__ OfShared<P> sh;
  const rvs_objective_arm &T = A.a[blockIdx.y];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int j = j0 + blockIdx.x;
  const int N = T.ntp, m = N - 2;
  const int nd = T.ndim, nv = 1 << nd;
  const int K = 1 + nd + (vsini_grad ? 1 : 0);
  const int64_t o = obj_out_index(Jl, blockIdx.x);
  double *B0 = lds, *B1 = lds + N, *B2 = lds + 2 * (int64_t)N;
  PolyLoc &PL = sh.PL;

  // ---- the grid cell: cell search, dw/dp, the job's Doppler scalars -------------------------
  // hands over: PL, mode, sh.dw, sh.jobsc
  const GridDesc G = obj_grid_desc(T);
  const double *prow = params + (int64_t)j * nd;
  poly_locate<OF_NT>(PL, G, prow, T.idgrid, T.uvecs, T.vecs_s, T.ngrid);
  const int mode = PL.mode;
  if (mode == 0) {
    // the weight's factor of dimension d replaced by -+1 / (cell width), per PHYSICAL
    // unit of p_d (the chain through log10 of a log_mask parameter included)
    for (int i = tid; i < nd * nv; i += OF_NT) {
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
    for (int k = tid; k < N; k += OF_NT) {
      double acc = 0;
      for (int v = 0; v < nv; v++)
        acc = fma(PL.w[v], (double)T.dats[PL.id[v] * N + k], acc);
      B0[k] = T.exp_flag ? exp(acc) : acc;
    }
  } else {
    double mx = 0;
    bool anynan = false;
    for (int k = tid; k < N; k += OF_NT) {
      const double val = T.exp_flag ? (double)np_expf(nrow[k]) : (double)nrow[k];
      B0[k] = val;
      obj_guard_scan(val, mx, anynan);
    }
    // ---- template guard ---------------------------------------------------------------------
    // hands over: `outside`, the arm's penalty term
    outside = obj_template_guard<OF_NW>(mx, anynan, &PL.dist, sh.red8);
  }
  __syncthreads();
  if (obj_template_unusable(outside)) {
    obj_store_skipped(o, armchi, armst, armout);
    if (tid < K) armgrad[o * K + tid] = 0.0;
    if (tid < K * K) armfisher[o * K * K + tid] = 0.0;
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
    obj_build_taps<OF_NT, false>(kmax, R, eps_ld, T.lnstep, B1, B2, nullptr, sh.red8);
    for (int i = tid; i < N; i += OF_NT) B1[i] = fir_at(B0, B2, i);
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
  const double *FC = FT + 4 * (int64_t)OF_NT * OF_CHMAX;
  // M x = rhs: rhs(u, 1/h_u, 1/h_{u+1}) is read by the row's owner ahead of every
  // barrier and x written behind them, so `out` may be the buffer rhs reads
  auto tri_solve = [&](auto rhs, double *out) __attribute__((always_inline)) {
    double loc[OF_CHMAX], pr[OF_CHMAX];
    double d = 0, pb = 1;
#pragma unroll
    for (int q = 0; q < OF_CHMAX; q++)
      if (q < CH && a0 + q < a1) {
        const double *rec = FT + ((int64_t)q * OF_NT + tid) * 4;
        const double ei = rec[3];
        d = rhs(a0 + q, rec[0], rec[1]) * rec[2] - ei * d;
        pb = -ei * pb;
        loc[q] = d;
        pr[q] = pb;
      }
    const double d_in = obj_chain3<OF_NW>(sh.edge, d, pb, -1);
    double z = 0;
    pb = 1;
#pragma unroll
    for (int q = OF_CHMAX - 1; q >= 0; q--)
      if (q < CH && a0 + q < a1) {
        const double ci = FC[((int64_t)(q >> 1) * OF_NT + tid) * 2 + (q & 1)];
        z = (loc[q] + pr[q] * d_in) - ci * z;   // d of the forward sweep, then z
        pb = -ci * pb;
        loc[q] = z;
        pr[q] = pb;
      }
    const double z_in = obj_chain3<OF_NW>(sh.edge, z, pb, +1);
#pragma unroll
    for (int q = 0; q < OF_CHMAX; q++)
      if (q < CH && a0 + q < a1) out[a0 + q] = loc[q] + pr[q] * z_in;
  };
  // the spline of the row in Y: right-hand sides 6 ((y_{u+2} - y_{u+1}) / h_{u+1} -
  // (y_{u+1} - y_u) / h_u); Z[u] = z at knot u + 1
  auto spline_construct = [&]() __attribute__((always_inline)) {
    tri_solve([&](int u, double ih0, double ih1) {
      const double s0 = (Y[u + 1] - Y[u]) * ih0, s1 = (Y[u + 2] - Y[u + 1]) * ih1;
      return 6 * (s1 - s0);
    }, Z);
  };
  spline_construct();
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
  // (the knot interval and the spline piece in objective_grad_kernel's spelling, so that
  // the value's bits are that kernel's)
  const double shift = KM.shift, lin_inv_step = KM.lin_inv_step, x0 = KM.x0;
  auto pix_pos = [&](int k) {   // (obj_knot_interval)
    int pos = S.log_step ? (int)(AG.pix[k] + shift)
                         : (int)((AG.lam[k] * f - x0) * lin_inv_step);
    return min(max(pos, 0), N - 2);
  };
  auto piece = [&](int pos) {   // (obj_piece) of the row in Y with its spline in Z
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
  for (int k = tid; k < npix; k += OF_NT) {
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
    for (int k = tid; k < npix; k += OF_NT) {
      const double te = F[k], dk = F[npix + k];   // (written by this same thread)
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
    for (int q = 1; q < OF_NW; q++) v += sh.red[q][tid];
    sh.Lc[tid] = v;
  }
  __syncthreads();
  // ---- solve (A10): Cholesky factor, coefficients, log det ---------------------------------
  // hands over: acc[] (L with 1 / L_ii on the diagonal) and av[] (the coefficients) in
  // every lane's registers for pass 2, and (behind pass 2's barrier) in sh.Lc; sh.fact
  // every lane factors the same matrix: A = L L^T in place with 1 / L_ii on the diagonal
  // (the only form the substitutions need), c = A^-1 v by the two substitutions
  // (point_grad_block)
  double acc[NTR], av[P];
  bool okl = true;
  double ldet = 0;
#pragma unroll
  for (int i = 0; i < NTR; i++) acc[i] = sh.Lc[i];
#pragma unroll
  for (int i = 0; i < P; i++) av[i] = sh.Lc[NTR + i];
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
  if (tid == 0) {
    sh.fact[0] = ldet;
    sh.fact[1] = okl ? 1.0 : 0.0;
  }
  // ---- residual (A11), the pixel adjoint and the velocity tangent ----------------------------
  // hands over: the work row W: [0] mbar, [1] te, [2] the velocity tangent m'_k0 (each
  // pixel by the thread that owns it); sh.rrw
  const double bb = vel[j] / RVS_C_KMS;
  const double dfdv = -f / (RVS_C_KMS * (1.0 - bb * bb));
  double *W = wrows + o * wstride;
  {
    double rr = 0;
    for (int k = tid; k < npix; k += OF_NT) {
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
      W[k] = mbar;
      W[npix + k] = te;
      W[2 * (int64_t)npix + k] = dtv * (lamk * dfdv);
    }
    rr = wave_sum(rr);
    if (lane == 0) sh.rrw[w] = rr;
  }
  __syncthreads();   // t, y, z and the pixel pair in F are dead; every lane has read sh.Lc
  // L and c leave the registers: the substitutions B = L^-1 B' and the fitted
  // continuum c.phi of the moment passes read them from LDS
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < NTR; i++) sh.Lc[i] = acc[i];
#pragma unroll
    for (int i = 0; i < P; i++) sh.Lc[NTR + i] = av[i];
  }

  // ---- the taps once more, to stay: w in B2[0, kmax], dw/dvsini behind them -------------------
  // (stage: two runs of kmax + 3 doubles in B0; 2 (kmax + 3) <= ntp by obj_rot_kmax)
  const bool vs_grad = vsini_grad && !copy;
  const double *wt = B2, *dwt = B2 + kmax + 1;
  if (!copy)
    obj_build_taps<OF_NT, false>(kmax, R, eps_ld, T.lnstep, B0, B2,
                                 vs_grad ? B2 + kmax + 1 : nullptr, sh.red8);
  else
    __syncthreads();   // (sh.Lc)

  // ---- the tangents, one at a time ------------------------------------------------------------
  // tangent 0 is the velocity (its values wait in the work row); 1 .. nd the library's
  // parameters; 1 + nd vsini.  Each row goes through the value's FIR, spline and
  // resampling; a row that is exactly 0 (nearest-neighbour templates: the parameters; the
  // FIR's copy branches: vsini) is written as such.
  for (int i = 0; i < K; i++) {
    double *Wi = W + (2 + (int64_t)i) * npix;
    const bool zero = (i >= 1 && i <= nd) ? (mode != 0) : (i > nd && !vs_grad);
    if (zero) {
      for (int k = tid; k < npix; k += OF_NT) Wi[k] = 0.0;
      if (tid < P) sh.bp[i][tid] = 0.0;
      if (tid == P) sh.g[i] = 0.0;
      continue;
    }
    if (i >= 1) {
      // ---- the row at the knots into B0 -----------------------------------------------------
      // parameter d: t'_n = t_n sum_v (dw_v/dp_d) L_vn with exp_flag, sum_v (dw_v/dp_d)
      // L_vn without (polylinear_kernel<true>); vsini: t itself, regathered
      const bool par = i <= nd;
      const int d = par ? i - 1 : 0;
      for (int n = tid; n < N; n += OF_NT) {
        double val;
        if (mode == 0) {
          double a = 0, g = 0;
          for (int v = 0; v < nv; v++) {
            const double Lv = (double)T.dats[PL.id[v] * N + n];
            a = fma(PL.w[v], Lv, a);
            g = fma(sh.dw[d * nv + v], Lv, g);
          }
          const double tn = T.exp_flag ? exp(a) : a;
          val = par ? (T.exp_flag ? tn * g : g) : tn;
        } else {
          val = T.exp_flag ? (double)np_expf(nrow[n]) : (double)nrow[n];
        }
        B0[n] = val;
      }
      __syncthreads();
      // ---- FIR: y' = w (*) t' (parameters), dw/dvsini (*) t (vsini) ------------------------
      Y = B0;
      Z = B1;
      if (!copy) {
        const double *tp = par ? wt : dwt;
        for (int n = tid; n < N; n += OF_NT) B1[n] = fir_at(B0, tp, n);
        Y = B1;
        Z = B0;
        __syncthreads();
      }
      // ---- spline: z' by the value's sweeps --------------------------------------------------
      spline_construct();
      __syncthreads();
    }
    // ---- moments: J_ki to the work row, B'_.i to sh.bp[i], g_i to sh.g[i] --------------------
    double vals[P + 1];   // [P] B'_pi, then g_i
#pragma unroll
    for (int p = 0; p <= P; p++) vals[p] = 0;
    for (int k = tid; k < npix; k += OF_NT) {
      double md;   // the tangent's value at pixel k
      if (i == 0) {
        md = Wi[k];
      } else {
        const int pos = pix_pos(k);
        const double dl = AG.lam[k] * f - S.knots[pos];
        md = obj_piece_value(piece(pos), dl);
      }
      const double mbar = W[k], te = W[npix + k];
      const double ie = sig[k].x;
      const double *pr = AG.polysT + (int64_t)k * P;
      double ph[P], sk = 0;
#pragma unroll
      for (int p = 0; p < P; p++) {
        ph[p] = pr[p];
        sk = fma(sh.Lc[NTR + p], ph[p], sk);
      }
      const double jk = (sk * ie) * md;   // J_ki = (c.phi_k / e_k) m'_ki
      const double zk = te * jk;
#pragma unroll
      for (int p = 0; p < P; p++) vals[p] = fma(ph[p], zk, vals[p]);
      vals[P] = fma(mbar, md, vals[P]);
      Wi[k] = jk;
    }
    int cnt, base, lim;
    wave_halve<P + 1>(vals, lane, cnt, base, lim);
#pragma unroll
    for (int q = 0; q < (P + 1 + 63) / 64 + 1; q++)
      if (q < cnt && base + q < lim) sh.red[w][base + q] = vals[q];
    __syncthreads();
    if (tid <= P) {   // the waves' totals in wave order
      double v = sh.red[0][tid];
#pragma unroll
      for (int q = 1; q < OF_NW; q++) v += sh.red[q][tid];
      if (tid < P)
        sh.bp[i][tid] = v;
      else
        sh.g[i] = v;
    }
    __syncthreads();   // the template buffers and sh.red are free again
  }
  __syncthreads();   // (the entries of sh.bp of a row that is exactly 0)

  // ---- B = L^-1 B': one forward substitution per tangent ---------------------------------
  if (tid < K) {
    double *b = sh.bp[tid];
#pragma unroll
    for (int p = 0; p < P; p++) {
      double sum = b[p];
#pragma unroll
      for (int q = 0; q < p; q++) sum = fma(-sh.Lc[TRI(p, q)], b[q], sum);
      b[p] = sum * sh.Lc[TRI(p, p)];
    }
  }
  // ---- Gram sums G_il = sum_k J_ki J_kl, l <= i ---------------------------------------------
  {
    double gv[OF_NG];
#pragma unroll
    for (int i = 0; i < OF_NG; i++) gv[i] = 0;
    for (int k = tid; k < npix; k += OF_NT) {
      double jr[OF_MAXK];
#pragma unroll
      for (int i = 0; i < OF_MAXK; i++)
        jr[i] = (i < K) ? W[(2 + (int64_t)i) * npix + k] : 0.0;
#pragma unroll
      for (int i = 0; i < OF_MAXK; i++)
        if (i < K) {
#pragma unroll
          for (int l = 0; l <= i; l++) gv[TRI(i, l)] = fma(jr[i], jr[l], gv[TRI(i, l)]);
        }
    }
    int cnt, base, lim;
    wave_halve<OF_NG>(gv, lane, cnt, base, lim);
#pragma unroll
    for (int q = 0; q < (OF_NG + 63) / 64 + 1; q++)
      if (q < cnt && base + q < lim) sh.red[w][base + q] = gv[q];
  }
  __syncthreads();

  // ---- tail: value and status, gradient, F = G - B^T B on both halves ------------------------
  double rr = sh.rrw[0];
#pragma unroll
  for (int q = 1; q < OF_NW; q++) rr += sh.rrw[q];
  double chi;
  int st;
  obj_value_status(S, AG, s, KM, xlast, sh.fact[0], sh.fact[1] != 0.0, rr, st_extra, chi, st);
  if (tid == 0) {
    armchi[o] = chi;
    armst[o] = st;
    armout[o] = outside;
  }
  if (tid < K) {
    // columns: vel, the parameters in library order (exactly 0 in the nearest-neighbour
    // modes), vsini (exactly 0 in the FIR's copy branches)
    armgrad[o * K + tid] = (chi == chi) ? sh.g[tid] : __builtin_nan("");
  }
  if (tid < K * (K + 1) / 2) {
    int i, l;
    of_tri_pair(tid, i, l);
    double gil = sh.red[0][tid];   // the waves' totals in wave order
#pragma unroll
    for (int q = 1; q < OF_NW; q++) gil += sh.red[q][tid];
    double bb2 = 0;
#pragma unroll
    for (int p = 0; p < P; p++) bb2 = fma(sh.bp[i][p], sh.bp[l][p], bb2);
    const double v = (chi == chi) ? gil - bb2 : __builtin_nan("");
    double *fo = armfisher + o * K * K;
    fo[i * K + l] = v;
    fo[l * K + i] = v;
  }
}

// arms summed in order (objective_grad_sum_kernel, point_fisher_sum_kernel); the
// penalties of A11 (spec_fit.py:888-896) on the value only: an arm whose outside flag
// is not finite adds 1000 badchi and nothing to the gradient and the Fisher matrix
__global__ void objective_fisher_sum_kernel(int narm, int Jl, int j0, int K, double badchi,
                                            double4 bconst,
                                            const double *__restrict__ pen_scale,
                                            const int32_t *__restrict__ job_spec,
                                            const double *__restrict__ armchi,
                                            const double *__restrict__ armgrad,
                                            const double *__restrict__ armfisher,
                                            const int32_t *__restrict__ armst,
                                            const double *__restrict__ armout,
                                            double *__restrict__ out,
                                            double *__restrict__ grad,
                                            double *__restrict__ fisher,
                                            int32_t *__restrict__ status) {
  const int jl = blockIdx.x * blockDim.x + threadIdx.x;
  if (jl >= Jl) return;
  const int j = j0 + jl;
  if (pen_scale) badchi *= pen_scale[job_spec ? job_spec[j] : j];
  const double bc[RVS_MAX_ARMS] = {bconst.x, bconst.y, bconst.z, bconst.w};
  const int KK = K * K;
  double tot = 0;
  bool counts[RVS_MAX_ARMS];
  int st = 0;
#pragma unroll
  for (int ia = 0; ia < RVS_MAX_ARMS; ia++) {
    counts[ia] = false;
    if (ia >= narm) continue;
    const int64_t o = (int64_t)ia * Jl + jl;
    const double ov = armout[o];
    if (!(fabs(ov) <= 1.79e308)) {
      tot += 1000.0 * badchi;
      continue;
    }
    counts[ia] = true;
    tot += armchi[o] + bc[ia] + ov * badchi;
    st |= armst[o];
  }
  out[j] = tot;
  for (int e = 0; e < K + KK; e++) {
    double v = 0;
#pragma unroll
    for (int ia = 0; ia < RVS_MAX_ARMS; ia++)
      if (counts[ia]) {
        const int64_t o = (int64_t)ia * Jl + jl;
        v += (e < K) ? armgrad[o * K + e] : armfisher[o * KK + (e - K)];
      }
    if (e < K)
      grad[(int64_t)j * K + e] = v;
    else
      fisher[(int64_t)j * KK + (e - K)] = v;
  }
  if (st) atomicOr(&status[j], st);
}

// doubles of a (job, arm) in the work buffer: value, outside, status (padded), K
// gradient entries, K^2 Fisher entries, the work row of (K + 2) npix_max
int64_t of_job_arm_doubles(int ntan, int npix_max) {
  const int64_t K = 1 + ntan;
  return 3 + K + K * K + (K + 2) * (int64_t)npix_max;
}

}  // namespace

// What the kernel covers, in host arithmetic only -- rvs_objective_grad_ok's rule, for
// the same reasons: npoly 1..10, grids of up to 4 dimensions, a template grid whose
// three buffers fit LDS beside the kernel's static part, and the pixels twice in one
// buffer (the sigma-scaled pair of the model pass).  The tangent passes add no
// condition: the taps and their derivatives (2 kmax + 2 doubles) and the primitives'
// stage (2 (kmax + 3)) fit a buffer of ntp doubles wherever obj_rot_kmax admits kmax.
extern "C" int rvs_objective_fisher_ok(int npoly, int npix, int ntp, int ndim,
                                       int vsini_grad) {
  if (npoly < 1 || npoly > OF_MAXP || npix < 1 || ntp < 32 ||
      ntp > RVS_OBJ_FT_MAX_NTP)
    return 0;
  if (ndim < 1 || ndim > OF_MAXDIM || vsini_grad < 0 || vsini_grad > 1) return 0;
  if (2 * (int64_t)npix > ntp) return 0;
  if (3 * (int64_t)ntp * (int64_t)sizeof(double) + OF_STATIC_MAX > OF_LDS_MAX) return 0;
  return 1;
}

extern "C" int64_t rvs_objective_fisher_work_size(int J, int narm, int ntan,
                                                  int npix_max) {
  if (J < 1 || narm < 1 || narm > RVS_MAX_ARMS || ntan < 1 || ntan > OF_MAXDIM + 1 ||
      npix_max < 1)
    return 0;
  return (int64_t)narm * J * of_job_arm_doubles(ntan, npix_max) * (int64_t)sizeof(double);
}

extern "C" int rvs_objective_fisher(const rvs_objective_arm *arms, int narm, int npoly,
                                    int ntan, const double *params, const double *vsini,
                                    const int32_t *job_spec, int J, const double *vel,
                                    double badchi, const double *basis_const, void *work,
                                    int64_t work_bytes, double *out, double *grad,
                                    double *fisher, int32_t *status, void *stream) {
  if (J < 1 || narm < 1 || narm > RVS_MAX_ARMS || !arms || !params || !vel || !work ||
      !out || !grad || !fisher || !status || npoly < 1 || npoly > OF_MAXP || ntan < 1 ||
      ntan > OF_MAXDIM + 1)
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
  int npix_max = 0;
  for (int i = 0; i < narm; i++) {
    const rvs_objective_arm &a = arms[i];
    if (a.ndim != ndim || a.pt.fast_interp || a.pt.taps || a.pt.G > 1 || !a.factors ||
        !a.dats || !a.idgrid || !a.uvecs || !a.vecs_s || a.pt.ntp != a.ntp ||
        !rvs_objective_fisher_ok(npoly, a.pt.npix, a.ntp, ndim, vsini_grad))
      return RVS_E_ARG;
    A.a[i] = a;
    if (basis_const) bc[i] = basis_const[i];
    shm = max(shm, (size_t)3 * a.ntp * sizeof(double));
    npix_max = max(npix_max, a.pt.npix);
  }
  for (int i = narm; i < RVS_MAX_ARMS; i++) A.a[i] = arms[0];
  // the jobs go in launches of as many as the work buffer holds, at least one
  const int64_t per_job = rvs_objective_fisher_work_size(1, narm, ntan, npix_max);
  if (work_bytes < per_job) return RVS_E_ARG;
  const int Jc = (int)min((int64_t)J, work_bytes / per_job);
  hipStream_t st = rvs_stream(stream);
  const int K = 1 + ntan;
  const int64_t wstride = (int64_t)(K + 2) * npix_max;
  const int64_t n = (int64_t)narm * Jc;
  double *armchi = (double *)work;
  double *armout = armchi + n;
  double *armgrad = armout + n;
  double *armfisher = armgrad + n * K;
  double *wrows = armfisher + n * K * K;
  int32_t *armst = (int32_t *)(wrows + n * wstride);
  for (int j0 = 0; j0 < J; j0 += Jc) {
    const int Jl = min(Jc, J - j0);
    dim3 grid(Jl, narm);
#define RVS_CASE(PP)                                                                \
  case PP: {                                                                        \
    static bool attr_set = false;                                                   \
    if (!attr_set) {                                                                \
      (void)hipFuncSetAttribute((const void *)objective_fisher_kernel<PP>,          \
                                hipFuncAttributeMaxDynamicSharedMemorySize,         \
                                OF_LDS_MAX - (int)sizeof(OfShared<PP>));            \
      (void)hipGetLastError();                                                      \
      attr_set = true;                                                              \
    }                                                                               \
    hipLaunchKernelGGL(objective_fisher_kernel<PP>, grid, dim3(OF_NT), shm, st, A,  \
                       params, vsini, vsini_grad, job_spec, Jl, j0, vel, 0.6, wrows, \
                       wstride, armchi, armgrad, armfisher, armst, armout);         \
  } break;
    switch (npoly) {
      RVS_CASE(1) RVS_CASE(2) RVS_CASE(3) RVS_CASE(4) RVS_CASE(5)
      RVS_CASE(6) RVS_CASE(7) RVS_CASE(8) RVS_CASE(9) RVS_CASE(10)
      default:
        return RVS_E_ARG;
    }
#undef RVS_CASE
    hipLaunchKernelGGL(objective_fisher_sum_kernel, dim3((Jl + 255) / 256), dim3(256), 0,
                       st, narm, Jl, j0, K, badchi,
                       make_double4(bc[0], bc[1], bc[2], bc[3]), arms[0].pt.pen_scale,
                       job_spec, armchi, armgrad, armfisher, armst, armout, out, grad,
                       fisher, status);
  }
  RVS_LAUNCH_CHECK();
  return 0;
}
