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
//                Cholesky factor and solve: the value phases objective_grad_kernel runs
//                (objective_point_dev.h; the same value and status)
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
#include "objective_point_dev.h"

#define OF_NG (OP_MAXK * (OP_MAXK + 1) / 2)   // packed lower triangle of G

namespace {

template <int P>
struct OfShared : OpShared<P, (op_nv(P) > OF_NG ? op_nv(P) : OF_NG)> {
  double rrw[OP_NW];          // the waves' shares of the residual norm
  double Lc[op_nv(P)];        // L packed (1 / L_ii on the diagonal), then c
  double bp[OP_MAXK][P];      // B'_.i, then B_.i = L^-1 B'_.i
  double g[OP_MAXK];          // g_i
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
__global__ void __launch_bounds__(OP_NT)
    objective_fisher_kernel(ObjArms A, const double *__restrict__ params,
                            const double *__restrict__ vsini, int vsini_grad,
                            const int32_t *__restrict__ job_spec, int Jl, int j0,
                            const double *__restrict__ vel, double eps_ld,
                            double *__restrict__ wrows, int64_t wstride,
                            double *__restrict__ armchi, double *__restrict__ armgrad,
                            double *__restrict__ armfisher, int32_t *__restrict__ armst,
                            double *__restrict__ armout) {
  constexpr int NTR = P * (P + 1) / 2;
  static_assert(sizeof(OfShared<P>) <= OP_STATIC_MAX, "op_point_ok's bound");
  extern __shared__ double lds[];
  __shared__ OfShared<P> sh;
  const int j = j0 + blockIdx.x;
  const int64_t o = obj_out_index(Jl, blockIdx.x);
  ObjPoint<P, OfShared<P>::REDW> pt(sh, A.a[blockIdx.y], lds, j, eps_ld);
  const rvs_objective_arm &T = pt.T;
  const rvs_point_arm &S = pt.S;
  const PolyLoc &PL = pt.PL;
  const int tid = pt.tid, lane = pt.lane, w = pt.w;
  const int N = pt.N, nd = pt.nd, nv = pt.nv, npix = pt.npix;
  const int K = 1 + nd + (vsini_grad ? 1 : 0);
  double *B0 = pt.B0, *B1 = pt.B1, *B2 = pt.B2;

  // ---- the value phases (objective_point_dev.h): the waves' totals into sh.Lc --------------
  // hands over, beyond the phases' own: L and c in pt.acc, pt.av for pass 2, and (behind
  // pass 2's barrier) in sh.Lc
  if (!pt.value_phases(params, vsini, job_spec, vel, sh.Lc)) {
    obj_store_skipped(o, armchi, armst, armout);
    if (tid < K) armgrad[o * K + tid] = 0.0;
    if (tid < K * K) armfisher[o * K * K + tid] = 0.0;
    return;
  }
  const ObjArmGrid &AG = pt.AG;
  const double2 *sig = pt.sig;
  const int mode = pt.mode, kmax = pt.kmax;
  const bool copy = pt.copy;
  const double f = pt.f;

  // ---- residual (A11), the pixel adjoint and the velocity tangent ----------------------------
  // hands over: the work row W: [0] mbar, [1] te, [2] the velocity tangent m'_k0 (each
  // pixel by the thread that owns it); sh.rrw
  const double dfdv = pt.dfdvel(vel[j]);
  double *W = wrows + o * wstride;
  {
    double rr = 0;
    for (int k = tid; k < npix; k += OP_NT) {
      const OpPixelAdjoint a = pt.pixel_adjoint(k, dfdv);
      rr = fma(a.r, a.r, rr);
      W[k] = a.mbar;
      W[npix + k] = a.te;
      W[2 * (int64_t)npix + k] = a.dmdv;
    }
    rr = wave_sum(rr);
    if (lane == 0) sh.rrw[w] = rr;
  }
  __syncthreads();   // t, y, z and the pixel pair in F are dead; every lane has read sh.Lc
  // L and c leave the registers: the substitutions B = L^-1 B' and the fitted
  // continuum c.phi of the moment passes read them from LDS
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < NTR; i++) sh.Lc[i] = pt.acc[i];
#pragma unroll
    for (int i = 0; i < P; i++) sh.Lc[NTR + i] = pt.av[i];
  }

  // ---- the taps once more, to stay: w in B2[0, kmax], dw/dvsini behind them -------------------
  // (stage: two runs of kmax + 3 doubles in B0; 2 (kmax + 3) <= ntp by obj_rot_kmax)
  const bool vs_grad = vsini_grad && !copy;
  const double *wt = B2, *dwt = B2 + kmax + 1;
  if (!copy)
    obj_build_taps<OP_NT, false>(kmax, pt.R, eps_ld, T.lnstep, B0, B2,
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
      for (int k = tid; k < npix; k += OP_NT) Wi[k] = 0.0;
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
      for (int n = tid; n < N; n += OP_NT) {
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
          val = T.exp_flag ? (double)np_expf(pt.nrow[n]) : (double)pt.nrow[n];
        }
        B0[n] = val;
      }
      __syncthreads();
      // ---- FIR: y' = w (*) t' (parameters), dw/dvsini (*) t (vsini) ------------------------
      pt.Y = B0;
      pt.Z = B1;
      if (!copy) {
        const double *tp = par ? wt : dwt;
        for (int n = tid; n < N; n += OP_NT) B1[n] = pt.fir_at(B0, tp, n);
        pt.Y = B1;
        pt.Z = B0;
        __syncthreads();
      }
      // ---- spline: z' by the value's sweeps --------------------------------------------------
      pt.spline_construct();
      __syncthreads();
    }
    // ---- moments: J_ki to the work row, B'_.i to sh.bp[i], g_i to sh.g[i] --------------------
    double vals[P + 1];   // [P] B'_pi, then g_i
#pragma unroll
    for (int p = 0; p <= P; p++) vals[p] = 0;
    for (int k = tid; k < npix; k += OP_NT) {
      double md;   // the tangent's value at pixel k
      if (i == 0) {
        md = Wi[k];
      } else {
        const int pos = pt.pix_pos(k);
        const double dl = AG.lam[k] * f - S.knots[pos];
        md = obj_piece_value(pt.piece(pos), dl);
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
      for (int q = 1; q < OP_NW; q++) v += sh.red[q][tid];
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
    for (int k = tid; k < npix; k += OP_NT) {
      double jr[OP_MAXK];
#pragma unroll
      for (int i = 0; i < OP_MAXK; i++)
        jr[i] = (i < K) ? W[(2 + (int64_t)i) * npix + k] : 0.0;
#pragma unroll
      for (int i = 0; i < OP_MAXK; i++)
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
  for (int q = 1; q < OP_NW; q++) rr += sh.rrw[q];
  const double chi = pt.store_value(rr, o, armchi, armst, armout);
  if (tid < K) {
    // columns: vel, the parameters in library order (exactly 0 in the nearest-neighbour
    // modes), vsini (exactly 0 in the FIR's copy branches)
    armgrad[o * K + tid] = pt.nan_with(chi, sh.g[tid]);
  }
  if (tid < K * (K + 1) / 2) {
    int i, l;
    of_tri_pair(tid, i, l);
    double gil = sh.red[0][tid];   // the waves' totals in wave order
#pragma unroll
    for (int q = 1; q < OP_NW; q++) gil += sh.red[q][tid];
    double bb2 = 0;
#pragma unroll
    for (int p = 0; p < P; p++) bb2 = fma(sh.bp[i][p], sh.bp[l][p], bb2);
    const double v = pt.nan_with(chi, gil - bb2);
    double *fo = armfisher + o * K * K;
    fo[i * K + l] = v;
    fo[l * K + i] = v;
  }
}

// doubles of a (job, arm) in the work buffer: value, outside, status (padded), K
// gradient entries, K^2 Fisher entries, the work row of (K + 2) npix_max
int64_t of_job_arm_doubles(int ntan, int npix_max) {
  const int64_t K = 1 + ntan;
  return 3 + K + K * K + (K + 2) * (int64_t)npix_max;
}

}  // namespace

// (what the kernel covers, rvs_objective_grad_ok's rule: op_point_ok)
extern "C" int rvs_objective_fisher_ok(int npoly, int npix, int ntp, int ndim,
                                       int vsini_grad) {
  return op_point_ok(npoly, npix, ntp, ndim, vsini_grad);
}

extern "C" int64_t rvs_objective_fisher_work_size(int J, int narm, int ntan,
                                                  int npix_max) {
  if (J < 1 || narm < 1 || narm > RVS_MAX_ARMS || ntan < 1 || ntan > OP_MAXDIM + 1 ||
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
  OpCall c;
  if (J < 1 || !params || !vel || !work || !out || !grad || !fisher || !status ||
      !op_check_arms(arms, narm, npoly, ntan, vsini, basis_const, c))
    return RVS_E_ARG;
  // the jobs go in launches of as many as the work buffer holds, at least one
  const int64_t per_job = rvs_objective_fisher_work_size(1, narm, ntan, c.npix_max);
  if (work_bytes < per_job) return RVS_E_ARG;
  const int Jc = (int)min((int64_t)J, work_bytes / per_job);
  hipStream_t st = rvs_stream(stream);
  const int K = 1 + ntan;
  const int64_t wstride = (int64_t)(K + 2) * c.npix_max;
  const int64_t n = (int64_t)narm * Jc;
  double *armchi = (double *)work;
  double *armout = armchi + n;
  double *armgrad = armout + n;
  double *armfisher = armgrad + n * K;
  double *wrows = armfisher + n * K * K;
  int32_t *armst = (int32_t *)(wrows + n * wstride);
  for (int j0 = 0; j0 < J; j0 += Jc) {
    const int Jl = min(Jc, J - j0);
    op_for_npoly(npoly, [&](auto p) {
      constexpr int PP = decltype(p)::value;
      op_launch<objective_fisher_kernel<PP>, (int)sizeof(OfShared<PP>)>(
          dim3(Jl, narm), c.shm, st, c.A, params, vsini, c.vsini_grad, job_spec, Jl, j0, vel,
          0.6, wrows, wstride, armchi, armgrad, armfisher, armst, armout);
    });
    hipLaunchKernelGGL(objective_point_sum_kernel, dim3((Jl + 255) / 256), dim3(256), 0, st,
                       narm, Jl, j0, K, badchi, c.bc, arms[0].pt.pen_scale, job_spec, armchi,
                       armgrad, armfisher, armst, armout, out, grad, fisher, status);
  }
  RVS_LAUNCH_CHECK();
  return 0;
}
