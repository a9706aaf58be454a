// What objective_grad.hip (value and gradient by the adjoint method) and
// objective_fisher.hip (value, gradient and Fisher matrix in forward mode)
// have in common, stated once: the constants, the shared part of the
// static LDS, the value phases of a (job, arm) with the state they hand over, the
// per-pixel body of pass 2, the coverage rule, the argument check, the launch and the
// sum over the arms.  Included by those two files only.  objective_fisher_kernel runs all
// of it; objective_grad_kernel takes the phases up to the spline construct and keeps
// model pass, normal equations, solve and pass 2 in its own text, on a measurement
// (DESIGN 4.24): a change to model_pass, normal_equations, solve or pixel_adjoint here is
// a change there.
#pragma once
#include <type_traits>
#include "objective_dev.h"

#define OP_NT RVS_OBJ_NT
#define OP_NW (OP_NT / 64)
#define OP_CHMAX RVS_OBJ_CHMAX
#define OP_MAXP 10     // beyond: the value kernel's wave totals live in the template buffer
#define OP_MAXDIM 4    // the bound of the cell record (OBJ_LOC_NV vertices)
#define OP_MAXK (2 + OP_MAXDIM)   // vel, parameters, vsini
// upper bound of a kernel's static LDS (OgShared, OfShared): what op_point_ok, host
// arithmetic only, counts beside the three template buffers
#define OP_STATIC_MAX 8192
#define OP_LDS_MAX (160 * 1024)

namespace {

// the normal equations' sums: [P (P + 1) / 2] packed lower triangle, then [P] right-hand
// sides
constexpr int op_nv(int P) { return P * (P + 1) / 2 + P; }

// the static LDS of the value phases; REDW: the most sums a kernel reduces at once
template <int P, int REDW_>
struct OpShared {
  static constexpr int REDW = REDW_;
  PolyLoc PL;
  double dw[OP_MAXDIM << OP_MAXDIM];   // dw_v/dp_d [d][v] (polylinear_kernel<true>)
  double red[OP_NW][REDW + 1];
  double edge[2][OP_NW][6];   // chunk coefficients across wave boundaries
  double red8[2 * OP_NW];
  double fact[2];             // log det L, 1: every pivot positive
  double jobsc[3];            // obj_job_scalars
};

// what pass 2 knows of a pixel: te = m/e, the residual r, the pixel adjoint
// mbar = 2 (m/e^2) q - 2 r s/e and the velocity tangent S'(x_k) lam_k df/dvel
struct OpPixelAdjoint {
  double te, r, mbar, dmdv;
};

// The value phases of one (job, arm) and what they hand over.  The members are the
// hand-over state: each phase's heading names the ones it sets.  Everything is inlined
// into the kernel, where the members are registers.
template <int P, int REDW>
struct ObjPoint {
  static constexpr int NTR = P * (P + 1) / 2;
  static constexpr int NV = op_nv(P);
  OpShared<P, REDW> &sh;
  PolyLoc &PL;
  const rvs_objective_arm &T;
  const rvs_point_arm &S;
  const int tid, lane, w;
  const int j;              // the job in the caller's arrays
  const int N, m, nd, nv, npix;
  double *const B0, *const B1, *const B2;   // the three template buffers
  const double eps_ld;
  // the grid cell
  int mode;
  const float *nrow;        // the nearest row (mode != 0)
  double outside;
  // rotational kernel
  int kmax, st_extra;
  double R;
  bool copy;
  // FIR: the buffers of y and z; F: the third one (taps, then the pixel pair)
  double *Y, *Z, *F;
  // spline chunks
  int CH, a0, a1;
  const double *FT, *FC;
  // model pass
  int s;
  ObjArmGrid AG;
  const double2 *sig;       // {1/e, D/e} of the spectrum's pixels
  double xlast;
  ObjKnotMap KM;
  double f, shift, lin_inv_step, x0;
  // solve: L with 1 / L_ii on the diagonal, the coefficients
  double acc[NTR], av[P];

  __device__ __forceinline__ ObjPoint(OpShared<P, REDW> &sh_, const rvs_objective_arm &T_,
                                      double *lds, int j_, double eps_ld_)
      : sh(sh_), PL(sh_.PL), T(T_), S(T_.pt), tid(threadIdx.x), lane(threadIdx.x & 63),
        w(threadIdx.x >> 6), j(j_), N(T_.ntp), m(T_.ntp - 2), nd(T_.ndim),
        nv(1 << T_.ndim), npix(T_.pt.npix), B0(lds), B1(lds + T_.ntp),
        B2(lds + 2 * (int64_t)T_.ntp), eps_ld(eps_ld_) {}

  // ---- the grid cell: cell search, dw/dp, the job's Doppler scalars -------------------------
  // hands over: PL, mode, sh.dw, sh.jobsc
  __device__ __forceinline__ void cell(const double *__restrict__ params,
                                       const double *__restrict__ vel) {
    const GridDesc G = obj_grid_desc(T);
    const double *prow = params + (int64_t)j * nd;
    poly_locate<OP_NT>(PL, G, prow, T.idgrid, T.uvecs, T.vecs_s, T.ngrid);
    mode = PL.mode;
    if (mode == 0) {
      // the weight's factor of dimension d replaced by -+1 / (cell width), per PHYSICAL
      // unit of p_d (the chain through log10 of a log_mask parameter included)
      for (int i = tid; i < nd * nv; i += OP_NT) {
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
  }

  // ---- gather (A3/A5): the template into B0; the template guard ---------------------------
  // hands over: B0, nrow; `outside`, the arm's penalty term (from every thread's {mx,
  // anynan} of a nearest row)
  __device__ __forceinline__ void gather_and_guard() {
    nrow = T.dats + (int64_t)(mode == 0 ? 0 : PL.nearest) * N;
    outside = 0.0;
    if (mode == 0) {
      for (int k = tid; k < N; k += OP_NT) {
        double a = 0;
        for (int v = 0; v < nv; v++)
          a = fma(PL.w[v], (double)T.dats[PL.id[v] * N + k], a);
        B0[k] = T.exp_flag ? exp(a) : a;
      }
    } else {
      double mx = 0;
      bool anynan = false;
      for (int k = tid; k < N; k += OP_NT) {
        const double val = T.exp_flag ? (double)np_expf(nrow[k]) : (double)nrow[k];
        B0[k] = val;
        obj_guard_scan(val, mx, anynan);
      }
      outside = obj_template_guard<OP_NW>(mx, anynan, &PL.dist, sh.red8);
    }
    __syncthreads();
  }

  // ---- template row: an evaluator's row from HBM into B0; the template guard ----------------
  // (in place of cell and gather_and_guard where the template is no grid gather: the MLP of
  // rvs_template_nn, as objective_kernel<P, true> takes it)
  // hands over: B0, mode (0: inside the evaluator's domain), sh.jobsc; `outside`, the arm's
  // penalty term (outside_in, or NaN where the MAX_VAL guard refuses the row)
  __device__ __forceinline__ void template_row(const double *__restrict__ row,
                                               double outside_in,
                                               const double *__restrict__ vel) {
    mode = (outside_in == 0.0) ? 0 : 1;
    nrow = nullptr;
    outside = 0.0;
    if (tid == 64) obj_job_scalars(T.pt, vel[j], sh.jobsc);
    double mx = 0;
    bool anynan = false;
    for (int k = tid; k < N; k += OP_NT) {
      const double val = row[k];
      B0[k] = val;
      if (mode != 0) obj_guard_scan(val, mx, anynan);
    }
    if (mode != 0) outside = obj_template_guard<OP_NW>(mx, anynan, &outside_in, sh.red8);
    __syncthreads();
  }

  // ---- rotational kernel ----------------------------------------------------------------------
  // hands over: kmax (0: `copy`, no FIR), R, st_extra; the taps are built where they are used
  __device__ __forceinline__ void rotational_kernel(const double *__restrict__ vsini) {
    bool refused = false;
    kmax = 0;
    R = 0;
    if (vsini) kmax = obj_rot_kmax(T, vsini[j], R, refused);
    copy = kmax == 0;
    st_extra = refused ? RVS_ST_NONFINITE : 0;
  }
  // 'same' convolution with zero padding and the symmetric taps tp[|m|], ascending
  // input index (vsini_fir)
  __device__ __forceinline__ double fir_at(const double *in, const double *tp, int i) const {
    double a = 0;
    const int q0 = max(i - kmax, 0), q1 = min(i + kmax, N - 1);
    for (int q = q0; q <= q1; q++) {
      const int mm = q - i;
      a = fma(in[q], tp[mm < 0 ? -mm : mm], a);
    }
    return a;
  }

  // ---- FIR (A6): y = w (*) t ----------------------------------------------------------------
  // hands over: Y, Z, F
  __device__ __forceinline__ void fir() {
    Y = B0, Z = B1, F = B2;
    if (!copy) {
      obj_build_taps<OP_NT, false>(kmax, R, eps_ld, T.lnstep, B1, B2, nullptr, sh.red8);
      for (int i = tid; i < N; i += OP_NT) B1[i] = fir_at(B0, B2, i);
      Y = B1;
      Z = B0;
      __syncthreads();
    }
  }

  // ---- spline construct (A7): the natural spline's tridiagonal solve ------------------------
  // hands over: Z (second derivatives of Y)
  // Thread t owns the rows [a0, a1) (CH of them) of the m unknowns; the chunks are joined
  // by obj_chain3 (barriers between the two solves).  The factors are the chunk-ordered
  // copy of rvs_spline_factors: record {1/h_u, 1/h_{u+1}, g_u, e_u} of row t CH + q at
  // [q][t], then the backward multipliers in pairs.
  __device__ __forceinline__ void spline_chunks() {
    CH = rvs_obj_chunk_len(m);
    a0 = min(m, tid * CH), a1 = min(m, a0 + CH);
    FT = T.factors + 5 * (int64_t)N;
    FC = FT + 4 * (int64_t)OP_NT * OP_CHMAX;
  }
  // M x = rhs: rhs(u, 1/h_u, 1/h_{u+1}) is read by the row's owner ahead of every
  // barrier and x written behind them, so `out` may be the buffer rhs reads
  template <class RHS>
  __device__ __forceinline__ void tri_solve(RHS rhs, double *out) const {
    double loc[OP_CHMAX], pr[OP_CHMAX];
    double d = 0, pb = 1;
#pragma unroll
    for (int q = 0; q < OP_CHMAX; q++)
      if (q < CH && a0 + q < a1) {
        const double *rec = FT + ((int64_t)q * OP_NT + tid) * 4;
        const double ei = rec[3];
        d = rhs(a0 + q, rec[0], rec[1]) * rec[2] - ei * d;
        pb = -ei * pb;
        loc[q] = d;
        pr[q] = pb;
      }
    const double d_in = obj_chain3<OP_NW>(sh.edge, d, pb, -1);
    double z = 0;
    pb = 1;
#pragma unroll
    for (int q = OP_CHMAX - 1; q >= 0; q--)
      if (q < CH && a0 + q < a1) {
        const double ci = FC[((int64_t)(q >> 1) * OP_NT + tid) * 2 + (q & 1)];
        z = (loc[q] + pr[q] * d_in) - ci * z;   // d of the forward sweep, then z
        pb = -ci * pb;
        loc[q] = z;
        pr[q] = pb;
      }
    const double z_in = obj_chain3<OP_NW>(sh.edge, z, pb, +1);
#pragma unroll
    for (int q = 0; q < OP_CHMAX; q++)
      if (q < CH && a0 + q < a1) out[a0 + q] = loc[q] + pr[q] * z_in;
  }
  // the spline of the row in Y: right-hand sides 6 ((y_{u+2} - y_{u+1}) / h_{u+1} -
  // (y_{u+1} - y_u) / h_u); Z[u] = z at knot u + 1
  __device__ __forceinline__ void spline_construct() const {
    tri_solve([&](int u, double ih0, double ih1) {
      const double s0 = (Y[u + 1] - Y[u]) * ih0, s1 = (Y[u + 2] - Y[u + 1]) * ih1;
      return 6 * (s1 - s0);
    }, Z);
  }

  // ---- model pass (A7 eval): the pixels' spline values -------------------------------------
  // hands over: s, AG, sig, xlast, KM; F ([npix] m/e, [npix] D/e)
  // The knot interval and the spline piece in these kernels' own spelling: through
  // obj_knot_interval / obj_piece the same arithmetic measured 0.6 % slower per call
  // (DESIGN 4.22); the value and the derivative of the piece are the shared ones.
  __device__ __forceinline__ int pix_pos(int k) const {   // (obj_knot_interval)
    int pos = S.log_step ? (int)(AG.pix[k] + shift)
                         : (int)((AG.lam[k] * f - x0) * lin_inv_step);
    return min(max(pos, 0), N - 2);
  }
  // the knot intervals' widths and their reciprocals (formed where they are read: as
  // members they left objective_fisher_kernel<1> a dead 36 B of scratch per lane)
  __device__ __forceinline__ const double *hh() const { return T.factors + 3 * (int64_t)N; }
  __device__ __forceinline__ const double *ih() const { return T.factors + 4 * (int64_t)N; }
  // (obj_piece) of the row in Y with its spline in Z
  __device__ __forceinline__ ObjPiece piece(int pos) const {
    ObjPiece p;
    const double h = hh()[pos], hinv = ih()[pos];
    const double zi = (pos == 0) ? 0.0 : Z[pos - 1];
    const double zi1 = (pos + 1 == N - 1) ? 0.0 : Z[pos];
    const double yi1 = Y[pos + 1];
    p.yi = Y[pos];
    const double t1 = hinv * (1.0 / 6), t2 = h * (1.0 / 6);
    p.cb = (yi1 - p.yi) * hinv - t2 * (2 * zi + zi1);
    p.c2 = 0.5 * zi;
    p.c3 = (zi1 - zi) * t1;
    return p;
  }
  __device__ __forceinline__ void model_pass(const int32_t *__restrict__ job_spec) {
    s = job_spec ? job_spec[j] : j;
    AG = obj_arm_grid(S, s);
    sig = AG.sig;
    xlast = S.knots[N - 1];
    KM = {S.log_step, N, sh.jobsc[0], sh.jobsc[1], sh.jobsc[2], S.knots[0]};
    f = KM.f;
    shift = KM.shift, lin_inv_step = KM.lin_inv_step, x0 = KM.x0;
    // (a loop of its own, which holds no accumulators, as in objective_kernel)
    for (int k = tid; k < npix; k += OP_NT) {
      const int pos = pix_pos(k);
      const double dl = AG.lam[k] * f - S.knots[pos];
      const double tv = obj_piece_value(piece(pos), dl);
      const double2 sg = sig[k];
      F[k] = tv * sg.x;
      F[npix + k] = sg.y;
    }
  }

  // ---- normal equations (A10): the sums per lane, waves' totals into `totals` --------------
  // hands over: totals[NV] (the caller's place in static LDS)
  __device__ __forceinline__ void normal_equations(double *totals) {
    {
      double vals[NV];   // [NTR] packed lower triangle, then [P] right-hand sides
#pragma unroll
      for (int i = 0; i < NV; i++) vals[i] = 0;
      for (int k = tid; k < npix; k += OP_NT) {
        const double te = F[k], dk = F[npix + k];   // (written by this same thread)
        // (the rows ST = phi m/e themselves: one register row where the value kernel
        // keeps phi and phi (m/e)^2 -- these kernels have the adjoint's state beside it)
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
      totals[tid] = v;
    }
    __syncthreads();
  }

  // ---- solve (A10): Cholesky factor, coefficients, log det ---------------------------------
  // hands over: acc[] (L with 1 / L_ii on the diagonal) and av[] (the coefficients) in
  // every lane's registers; sh.fact
  // every lane factors the same matrix: A = L L^T in place with 1 / L_ii on the diagonal
  // (the only form the substitutions need), c = A^-1 v by the two substitutions
  // (point_grad_block)
  __device__ __forceinline__ void solve(const double *totals) {
    bool okl = true;
    double ldet = 0;
#pragma unroll
    for (int i = 0; i < NTR; i++) acc[i] = totals[i];
#pragma unroll
    for (int i = 0; i < P; i++) av[i] = totals[NTR + i];
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
  }

  // The value phases in order.  totals: NV doubles of the caller's static LDS for the
  // normal equations' sums.  false: the template is unusable (the arm is skipped; the
  // caller stores its own zeros) -- every thread of the block returns the same.
  __device__ __forceinline__ bool value_phases(const double *__restrict__ params,
                                               const double *__restrict__ vsini,
                                               const int32_t *__restrict__ job_spec,
                                               const double *__restrict__ vel,
                                               double *totals) {
    cell(params, vel);
    gather_and_guard();
    if (obj_template_unusable(outside)) return false;
    rotational_kernel(vsini);
    fir();
    spline_chunks();
    spline_construct();
    __syncthreads();
    model_pass(job_spec);
    normal_equations(totals);
    solve(totals);
    return true;
  }

  // ---- residual (A11) and the pixel adjoint: the body of pass 2 -------------------------------
  // d chi^2 / d vel = sum_k mbar_k S'(x_k) lam_k df/dvel; dfdv: the job's df/dvel
  __device__ __forceinline__ double dfdvel(double velj) const {
    const double bb = velj / RVS_C_KMS;
    return -f / (RVS_C_KMS * (1.0 - bb * bb));
  }
  __device__ __forceinline__ OpPixelAdjoint pixel_adjoint(int k, double dfdv) const {
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
    const double mbar = 2.0 * ie * (te * qk - r * mk);
    const int pos = pix_pos(k);
    const double lamk = AG.lam[k];
    // (lam f rounded on its own: where the pass was the kernels' own text the product sat
    // in pix_pos's basic block and was never contracted into the difference)
    const double dl = obj_mul_rounded(lamk, f) - S.knots[pos];
    const double dtv = obj_piece_deriv(piece(pos), dl);
    return {te, r, mbar, dtv * (lamk * dfdv)};
  }

  // ---- tail: value and status as rvs_chisq_point forms them, to the per-arm outputs ----------
  // rr: the residual norm; returns chi (NaN: the gradient is NaN under the same status)
  __device__ __forceinline__ double store_value(double rr, int64_t o,
                                                double *__restrict__ armchi,
                                                int32_t *__restrict__ armst,
                                                double *__restrict__ armout) const {
    double chi;
    int st;
    obj_value_status(S, AG, s, KM, xlast, sh.fact[0], sh.fact[1] != 0.0, rr, st_extra, chi,
                     st);
    if (tid == 0) {
      armchi[o] = chi;
      armst[o] = st;
      armout[o] = outside;
    }
    return chi;
  }
  // where chi^2 is NaN, so are the gradient and the Fisher matrix
  static __device__ __forceinline__ double nan_with(double chi, double v) {
    return (chi == chi) ? v : __builtin_nan("");
  }
};

// arms summed in order; the penalties of A11 (spec_fit.py:888-896) on the value only: an
// arm whose outside flag is not finite adds 1000 badchi and nothing to the gradient and
// the Fisher matrix.  Jl: the jobs of this launch (the stride of the per-arm outputs),
// j0: the first of them in the caller's arrays; fisher == nullptr: value and gradient
// (every entry is 0 + the arms' terms in arm order, whichever caller)
__global__ void objective_point_sum_kernel(int narm, int Jl, int j0, int K, double badchi,
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
  for (int e = 0; e < K + (fisher ? KK : 0); e++) {
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

// What the two kernels cover, in host arithmetic only: npoly 1..10 (beyond, the value
// kernel's wave totals live in the template buffer), grids of up to 4 dimensions, a
// template grid whose three buffers fit LDS beside the kernel's static part, and the
// pixels twice in one buffer (the sigma-scaled pair of the model pass; in the gradient
// kernel then the pixel adjoint with the first-pixel table of ntp int32 behind it:
// npix + ntp / 2 <= ntp).  The Fisher kernel's tangent passes add no condition: the taps
// and their derivatives (2 kmax + 2 doubles) and the primitives' stage (2 (kmax + 3)) fit
// a buffer of ntp doubles wherever obj_rot_kmax admits kmax.
// (the geometry alone: what the from-template form of the gradient kernel, which reads no
// cell record, asks of an arm)
inline int op_geometry_ok(int npoly, int npix, int ntp, int vsini_grad) {
  if (npoly < 1 || npoly > OP_MAXP || npix < 1 || ntp < 32 || ntp > RVS_OBJ_FT_MAX_NTP)
    return 0;
  if (vsini_grad < 0 || vsini_grad > 1) return 0;
  if (2 * (int64_t)npix > ntp) return 0;
  if (3 * (int64_t)ntp * (int64_t)sizeof(double) + OP_STATIC_MAX > OP_LDS_MAX) return 0;
  return 1;
}
inline int op_point_ok(int npoly, int npix, int ntp, int ndim, int vsini_grad) {
  if (ndim < 1 || ndim > OP_MAXDIM) return 0;
  return op_geometry_ok(npoly, npix, ntp, vsini_grad);
}
// ... of the gradient kernel under a resolution matrix of nd diagonals (objective_grad_kernel
// <.., RESOL>): the arithmetic of rvs_objective_grad_resol_ok, where the
// inequality is derived from the layout (objective_grad.hip)
#define OP_MAXND 33
inline int op_resol_geometry_ok(int npoly, int npix, int ntp, int nd, int vsini_grad) {
  if (nd < 1 || nd > OP_MAXND || !(nd & 1)) return 0;
  if (!op_geometry_ok(npoly, npix, ntp, vsini_grad)) return 0;
  if (2 * (int64_t)npix + nd - 1 > ntp) return 0;
  return 1;
}
// an arm's matrix as the RESOL form takes it (an arm without one: a band of one diagonal)
inline bool op_arm_resol_ok(const rvs_objective_arm &a, int npoly, int vsini_grad) {
  if (!a.pt.taps) return true;   // (2 npix <= ntp: op_geometry_ok)
  return op_resol_geometry_ok(npoly, a.pt.npix, a.ntp, a.pt.nd, vsini_grad) &&
         (a.pt.taps_stride == 0 || a.pt.taps_stride >= (int64_t)a.pt.npix * a.pt.nd);
}

// the arms of a call, checked and copied for the launch
struct OpCall {
  ObjArms A;
  double4 bc;                // the basis constants
  size_t shm;                // dynamic LDS: the widest arm's three buffers
  int vsini_grad, npix_max;
};
// ntan = ndim: vel and the parameters; ndim + 1: vsini fitted, its column last.  resol:
// the RESOL form of the gradient kernel, which reads pt.taps / pt.nd.  false: RVS_E_ARG
inline bool op_check_arms(const rvs_objective_arm *arms, int narm, int npoly, int ntan,
                          const double *vsini, const double *basis_const, OpCall &c,
                          bool resol = false) {
  static_assert(RVS_MAX_ARMS == 4, "basis constants travel as a double4");
  if (narm < 1 || narm > RVS_MAX_ARMS || !arms || npoly < 1 || npoly > OP_MAXP ||
      ntan < 1 || ntan > OP_MAXDIM + 1)
    return false;
  const int ndim = arms[0].ndim;
  c.vsini_grad = (ntan == ndim + 1) ? 1 : 0;
  if (ntan != ndim + c.vsini_grad || (c.vsini_grad && !vsini)) return false;
  c.A.n = narm;
  c.shm = 0;
  c.npix_max = 0;
  double bc[RVS_MAX_ARMS] = {0, 0, 0, 0};
  for (int i = 0; i < narm; i++) {
    const rvs_objective_arm &a = arms[i];
    if (a.ndim != ndim || a.pt.fast_interp || (a.pt.taps && !resol) || a.pt.G > 1 ||
        !a.factors || !a.dats || !a.idgrid || !a.uvecs || !a.vecs_s || a.pt.ntp != a.ntp ||
        !op_point_ok(npoly, a.pt.npix, a.ntp, ndim, c.vsini_grad) ||
        !op_arm_resol_ok(a, npoly, c.vsini_grad))
      return false;
    c.A.a[i] = a;
    if (basis_const) bc[i] = basis_const[i];
    c.shm = max(c.shm, (size_t)3 * a.ntp * sizeof(double));
    c.npix_max = max(c.npix_max, a.pt.npix);
  }
  for (int i = narm; i < RVS_MAX_ARMS; i++) c.A.a[i] = arms[0];
  c.bc = make_double4(bc[0], bc[1], bc[2], bc[3]);
  return true;
}

// ... of the from-template form: the arms carry no grid (dats, idgrid, uvecs and ndim are
// not read), the geometry rule is op_geometry_ok.  false: RVS_E_ARG
inline bool op_check_arms_templ(const rvs_objective_arm *arms, int narm, int npoly,
                                int vsini_grad, const double *vsini,
                                const double *basis_const, OpCall &c, bool resol = false) {
  if (narm < 1 || narm > RVS_MAX_ARMS || !arms || npoly < 1 || npoly > OP_MAXP ||
      vsini_grad < 0 || vsini_grad > 1 || (vsini_grad && !vsini))
    return false;
  c.vsini_grad = vsini_grad;
  c.A.n = narm;
  c.shm = 0;
  c.npix_max = 0;
  double bc[RVS_MAX_ARMS] = {0, 0, 0, 0};
  for (int i = 0; i < narm; i++) {
    const rvs_objective_arm &a = arms[i];
    if (a.pt.fast_interp || (a.pt.taps && !resol) || a.pt.G > 1 || !a.factors ||
        a.pt.ntp != a.ntp || !op_geometry_ok(npoly, a.pt.npix, a.ntp, vsini_grad) ||
        !op_arm_resol_ok(a, npoly, vsini_grad))
      return false;
    c.A.a[i] = a;
    c.A.a[i].ndim = 0;   // (documented as not read: no shift by a caller's leftover)
    if (basis_const) bc[i] = basis_const[i];
    c.shm = max(c.shm, (size_t)3 * a.ntp * sizeof(double));
    c.npix_max = max(c.npix_max, a.pt.npix);
  }
  for (int i = narm; i < RVS_MAX_ARMS; i++) c.A.a[i] = c.A.a[0];
  c.bc = make_double4(bc[0], bc[1], bc[2], bc[3]);
  return true;
}

// the dynamic-LDS attribute of KERN once, then the launch; STATIC_BYTES: the kernel's
// static LDS
template <auto KERN, int STATIC_BYTES, class... Args>
void op_launch(dim3 grid, size_t shm, hipStream_t st, Args... args) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void *)KERN, hipFuncAttributeMaxDynamicSharedMemorySize,
                              OP_LDS_MAX - STATIC_BYTES);
    (void)hipGetLastError();
    attr_set = true;
  }
  hipLaunchKernelGGL(KERN, grid, dim3(OP_NT), shm, st, args...);
}
// f(std::integral_constant<int, npoly>) for npoly 1 .. OP_MAXP; false beyond
template <int P = 1, class F>
bool op_for_npoly(int npoly, F f) {
  if constexpr (P <= OP_MAXP) {
    if (npoly != P) return op_for_npoly<P + 1>(npoly, f);
    f(std::integral_constant<int, P>());
    return true;
  }
  return false;
}

}  // namespace
