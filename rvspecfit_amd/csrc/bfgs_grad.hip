// bfgs_grad.hip -- the optimiser's (f, grad f) from the analytic-gradient chain: what
// vel_fit.chisq_func_grad is to one vector, for the rows of a round of rvs_bfgs_run_grad
// (bfgs_dev.hip).
//
//   rvs_proc_map            X [J, n] -> vel, vsini, params, prior / vsini penalty, bad
//   per arm                 rvs_template_polylinear_grad | rvs_template_tri(_buckets)_grad
//                           | rvs_template_nn_grad + rvs_nn_outside
//                           rvs_vsini_convolve_grad (vsini fitted) | rvs_vsini_convolve
//                           over the 1 + ndim rows (vsini fixed) | nothing
//                           rvs_spline_construct of the (1 + ntan) J rows
//                           the outside penalty of the rows
//   rvs_chisq_point_grad    all arms: chi [J], grad [J, 1 + ntan] = d/d(vel, parameters
//                           in library order[, vsini])
//   rvs_proc_finish_grad    F [J, 1 + n] = (chisq_func, its gradient in X's columns)
// and the Fisher form of the last two calls, for the rows of a round of rvs_lm_run
// (lm_dev.hip):
//   rvs_chisq_point_fisher  chi, grad and fisher [J, 1 + ntan, 1 + ntan]
//   rvs_proc_finish_fisher  F [J, 1 + n + n (n + 1) / 2] = (chisq_func, its gradient, the
//                           lower triangle of its Gauss-Newton Hessian in X's columns)
//
// The chain is engine.build_templates(tangents=True, vsini_tangent=...) +
// engine.chisq_point_grad: the same entry points with the same arguments, called from
// C on one stream, so a row has the bits spec_fit.chisq_grad_jobs gives it.
//
// The steps the chain shares with the fused forms of bfgs_dev.hip and lm_dev.hip are
// the internal entries of nm_internal.h: the map (nm.hip), the finish of either form
// (rvs_internal_proc_finish) and the check that g and o fit each other
// (rvs_internal_grad_rows_ok); the rounds around a chunk are rounds_run's (rounds_dev.h).
#include "common.h"
#include "nm_internal.h"

namespace {

struct FinP {
  int n, ndim, ntan, vsini_col;
  int src[8];
  int tan[8];   // column of X -> its row of grad / fisher (the inverse of src)
  const double *prior_mean, *prior_isig;
  double max_vsini;
};

// one row of rvs_proc_finish_grad (FISHER = false) or rvs_proc_finish_fisher: the value
// and the gradient are the same statements for both, the Fisher form appends the packed
// Hessian behind them
template <bool FISHER>
__global__ void __launch_bounds__(256)
    proc_finish_kernel(int J, const int32_t *__restrict__ counts, int cidx, FinP P,
                       const double *__restrict__ chi, const double *__restrict__ grad,
                       const double *__restrict__ fisher, const double *__restrict__ X,
                       const double *__restrict__ params,
                       const double *__restrict__ extra,
                       const int32_t *__restrict__ bad,
                       const int32_t *__restrict__ job_spec,
                       const int32_t *__restrict__ job_status,
                       double *__restrict__ F, int32_t *__restrict__ spec_status) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= J) return;
  const int n = P.n, K = 1 + P.ntan;
  const int width = FISHER ? 1 + n + n * (n + 1) / 2 : n + 1;
  double *f = F + (int64_t)j * width;
  const int isbad = bad[j];
  f[0] = isbad ? 1e30 : chi[j] + extra[j];
  if (isbad) {
    for (int c = 1; c < width; c++) f[c] = 0.0;
    return;
  }
  const double *g = grad + (int64_t)j * K;
  const int r = job_spec[j];
  f[1] = g[0];   // column 0 of X is the velocity
  for (int i = 0; i < P.ndim; i++) {
    const int c = P.src[i];
    if (c < 0) continue;   // fixed: no column
    double v = g[1 + i];
    if (P.prior_mean) {
      const double is = P.prior_isig[(int64_t)r * P.ndim + i];
      if (is != 0)
        v += 2.0 * (params[(int64_t)j * P.ndim + i] -
                    P.prior_mean[(int64_t)r * P.ndim + i]) * is * is;
    }
    f[1 + c] = v;
  }
  bool inside = true, beyond = false;
  if (P.vsini_col >= 0) {
    // VSiniMapper clamps: inside (0, max_vsini) the physical derivative, outside 0;
    // the penalty (x - clamp(x))^2 adds 2 (x - clamp(x))
    const double x = X[(int64_t)j * n + P.vsini_col];
    const double cl = fmin(fmax(x, 0.0), P.max_vsini);
    inside = (0 < x) && (x < P.max_vsini);
    beyond = (x < 0) || (x > P.max_vsini);
    f[1 + P.vsini_col] = (inside ? g[P.ntan] : 0.0) + 2.0 * (x - cl);
  }
  if (FISHER) {
    // H_ab = 2 fisher[tan a, tan b] (the matrix is in the 0.5 chi^2 convention); the
    // vsini row and column where the mapper does not clamp, else 0; on the diagonal the
    // second derivatives of a prior, 2 isig^2, and of the clamp penalty, 2
    const double *fm = fisher + (int64_t)j * K * K;
    double *h = f + 1 + n;
    for (int a = 0; a < n; a++)
      for (int b = 0; b <= a; b++) {
        double v = 2.0 * fm[P.tan[a] * K + P.tan[b]];
        if ((a == P.vsini_col || b == P.vsini_col) && !inside) v = 0.0;
        if (a == b) {
          const int i = P.tan[a] - 1;
          if (a == P.vsini_col) {
            if (beyond) v += 2.0;
          } else if (i >= 0 && P.prior_mean) {
            const double is = P.prior_isig[(int64_t)r * P.ndim + i];
            if (is != 0) v += 2.0 * (is * is);
          }
        }
        h[a * (a + 1) / 2 + b] = v;
      }
  }
  const int live = counts ? counts[cidx] : J;
  if (j < live && job_status[j]) atomicOr(&spec_status[r], job_status[j]);
}

// penalty[j] = outside[j] * (badchi of the job's spectrum): engine.chisq_point_grad's
// `o * batch.badchi_jobs(job_spec)`
__global__ void __launch_bounds__(256)
    grad_penalty_kernel(int J, const double *__restrict__ outside,
                        const double *__restrict__ pen_scale,
                        const int32_t *__restrict__ job_spec, double badchi,
                        double *__restrict__ pen) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= J) return;
  const double b = pen_scale ? pen_scale[job_spec[j]] * badchi : badchi;
  pen[j] = outside[j] * b;
}

// one vsini / outside flag per ROW of rvs_vsini_convolve over the R rows of a job
__global__ void __launch_bounds__(256)
    grad_repeat_kernel(int J, int R, const double *__restrict__ vsini,
                       const double *__restrict__ outside, double *__restrict__ vs_rows,
                       double *__restrict__ out_rows) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= J * R) return;
  vs_rows[t] = vsini[t / R];
  out_rows[t] = outside[t / R];
}

}  // namespace

int rvs_internal_grad_rows_ok(const rvs_grad_chain *g, const rvs_nm_objective *o,
                              int max_ndim) {
  return g && o && g->chi && g->grad && g->cap >= 1 && g->narm >= 1 &&
         g->narm <= RVS_MAX_ARMS && g->narm == o->narm && g->vsini_mode >= 0 &&
         g->vsini_mode <= 2 && o->ndim >= 1 && o->ndim <= max_ndim &&
         g->ntan == o->ndim + (g->vsini_mode == 2 ? 1 : 0) &&
         (g->vsini_mode == 2) == (o->vsini_col >= 0) &&
         (g->vsini_mode != 0) == (o->vsini != nullptr) && o->vel && o->params &&
         o->extra && o->bad && o->job_spec && o->jstatus && o->status && o->fixed &&
         o->safe;
}

int rvs_internal_grad_chain_ok(const rvs_grad_chain *g, const rvs_nm_objective *o) {
  if (!rvs_internal_grad_rows_ok(g, o, 6) || !g->arms || !g->point || !g->point_work ||
      g->ntan > 6 || o->n < 1 || o->n > 8)
    return 0;
  for (int a = 0; a < g->narm; a++) {
    const rvs_grad_arm &A = g->arms[a];
    if (!A.dats || !A.knots || !A.templ || !A.coef || !A.outside || !A.penalty ||
        A.ntp < 3 || A.ntp != g->point[a].ntp || !(A.lnstep > 0))
      return 0;
    if (g->point[a].coef != A.coef || g->point[a].penalty != A.penalty) return 0;
    if (A.tri == 2) {   // an MLP library: dats is a HOST rvs_nm_nn_arm
      const rvs_nm_nn_arm *N = static_cast<const rvs_nm_nn_arm *>(A.dats);
      if (!N->M || !N->S || !N->W || !N->b || !N->dims || !N->act0 || !N->act1 ||
          N->nlayer < 3 || N->dims[0] != o->ndim || N->dims[N->nlayer] != A.ntp ||
          (N->xeqs ? (!N->yeqs || N->nfx < 1 || N->nfy < 1) : (N->nfx || N->nfy)))
        return 0;
    } else if (A.tri ? (!A.transform || !A.extraflags || !A.simplices || !A.simplex ||
                        A.nsimplex < 1)
                     : (!A.idgrid || !A.uvecs || !A.vecs_s || !A.lens || !A.ptp ||
                        A.ngrid < 1))
      return 0;
    if (g->vsini_mode != 0 && !A.templ2) return 0;
    if (g->vsini_mode == 1 && (!A.vs_rows || !A.out_rows)) return 0;
  }
  return 1;
}

namespace {

// the argument checks and the launch of both forms (fisher == NULL: the gradient's)
int proc_finish(bool want_fisher, int J, int n, int ndim, int ntan,
                const int32_t *counts, int cidx, const double *chi, const double *grad,
                const double *fisher, const double *X, const double *params,
                const double *extra, const int32_t *bad, const int32_t *job_spec,
                const int32_t *job_status, const int32_t *src, int vsini_col,
                const double *prior_mean, const double *prior_isig, double max_vsini,
                double *F, int32_t *spec_status, void *stream) {
  if (J < 1 || n < 1 || n > 8 || ndim < 1 || ndim > 6 || !src || !chi || !grad || !X ||
      !params || !extra || !bad || !job_spec || !job_status || !F || !spec_status ||
      vsini_col >= n || (prior_mean && !prior_isig) || (want_fisher && !fisher))
    return RVS_E_ARG;
  if (ntan != ndim + (vsini_col >= 0 ? 1 : 0)) return RVS_E_ARG;
  FinP P;
  P.n = n, P.ndim = ndim, P.ntan = ntan, P.vsini_col = vsini_col;
  int ncol = 1 + (vsini_col >= 0 ? 1 : 0);
  for (int i = 0; i < 8; i++) P.tan[i] = 0;
  for (int i = 0; i < 8; i++) {
    P.src[i] = (i < ndim) ? src[i] : -1;
    if (P.src[i] >= n || P.src[i] == 0 || (P.src[i] >= 0 && P.src[i] == vsini_col))
      return RVS_E_ARG;
    if (P.src[i] > 0) {
      ncol++;
      P.tan[P.src[i]] = 1 + i;
    }
  }
  if (ncol != n) return RVS_E_ARG;   // every column of X has exactly one source
  if (vsini_col >= 0) P.tan[vsini_col] = ntan;
  P.prior_mean = prior_mean, P.prior_isig = prior_isig;
  P.max_vsini = max_vsini;
  if (want_fisher)
    hipLaunchKernelGGL(proc_finish_kernel<true>, dim3((J + 255) / 256), dim3(256), 0,
                       rvs_stream(stream), J, counts, cidx, P, chi, grad, fisher, X,
                       params, extra, bad, job_spec, job_status, F, spec_status);
  else
    hipLaunchKernelGGL(proc_finish_kernel<false>, dim3((J + 255) / 256), dim3(256), 0,
                       rvs_stream(stream), J, counts, cidx, P, chi, grad, fisher, X,
                       params, extra, bad, job_spec, job_status, F, spec_status);
  RVS_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int rvs_proc_finish_grad(int J, int n, int ndim, int ntan,
                                    const int32_t *counts, int cidx, const double *chi,
                                    const double *grad, const double *X,
                                    const double *params, const double *extra,
                                    const int32_t *bad, const int32_t *job_spec,
                                    const int32_t *job_status, const int32_t *src,
                                    int vsini_col, const double *prior_mean,
                                    const double *prior_isig, double max_vsini,
                                    double *F, int32_t *spec_status, void *stream) {
  return proc_finish(false, J, n, ndim, ntan, counts, cidx, chi, grad, nullptr, X,
                     params, extra, bad, job_spec, job_status, src, vsini_col,
                     prior_mean, prior_isig, max_vsini, F, spec_status, stream);
}

extern "C" int rvs_proc_finish_fisher(int J, int n, int ndim, int ntan,
                                      const int32_t *counts, int cidx,
                                      const double *chi, const double *grad,
                                      const double *fisher, const double *X,
                                      const double *params, const double *extra,
                                      const int32_t *bad, const int32_t *job_spec,
                                      const int32_t *job_status, const int32_t *src,
                                      int vsini_col, const double *prior_mean,
                                      const double *prior_isig, double max_vsini,
                                      double *F, int32_t *spec_status, void *stream) {
  return proc_finish(true, J, n, ndim, ntan, counts, cidx, chi, grad, fisher, X, params,
                     extra, bad, job_spec, job_status, src, vsini_col, prior_mean,
                     prior_isig, max_vsini, F, spec_status, stream);
}

extern "C" int64_t rvs_grad_chain_work_size(int cap, int narm, int ntan,
                                            const int32_t *ntp, int vsini_mode) {
  if (cap < 1 || narm < 1 || narm > RVS_MAX_ARMS || ntan < 1 || ntan > 6 || !ntp ||
      vsini_mode < 0 || vsini_mode > 2)
    return 0;
  const int64_t K = 1 + ntan;
  int64_t b = rvs_chisq_point_grad_work_size(cap, narm, ntan);
  b += (int64_t)cap * (1 + K) * sizeof(double);   // chi, grad
  for (int a = 0; a < narm; a++) {
    if (ntp[a] < 3) return 0;
    const int64_t rows = (int64_t)cap * K * ntp[a] * sizeof(double);
    b += rows * (vsini_mode ? 2 : 1);   // templ (+ templ2)
    b += rows * 4;                      // coef
    b += (int64_t)cap * (2 * sizeof(double) + sizeof(int32_t));   // outside, penalty, simplex
    if (vsini_mode == 1) b += (int64_t)cap * K * 2 * sizeof(double);   // vs_rows, out_rows
  }
  return b;
}

extern "C" int64_t rvs_fisher_chain_work_size(int cap, int narm, int ntan,
                                              const int32_t *ntp, int vsini_mode) {
  const int64_t b = rvs_grad_chain_work_size(cap, narm, ntan, ntp, vsini_mode);
  if (b <= 0) return 0;
  const int64_t K = 1 + ntan;
  return b + rvs_chisq_point_fisher_work_size(cap, narm, ntan) +
         (int64_t)cap * K * K * sizeof(double);
}

int rvs_internal_proc_finish(const rvs_nm_objective *o, const rvs_grad_chain *g,
                             const double *fisher, const double *X, int J,
                             const int32_t *counts, int cidx, double *F, hipStream_t st) {
  if (fisher)
    return rvs_proc_finish_fisher(J, o->n, o->ndim, g->ntan, counts, cidx, g->chi,
                                  g->grad, fisher, X, o->params, o->extra, o->bad,
                                  o->job_spec, o->jstatus, o->src, o->vsini_col,
                                  o->prior_mean, o->prior_isig, o->max_vsini, F,
                                  o->status, st);
  return rvs_proc_finish_grad(J, o->n, o->ndim, g->ntan, counts, cidx, g->chi, g->grad, X,
                              o->params, o->extra, o->bad, o->job_spec, o->jstatus,
                              o->src, o->vsini_col, o->prior_mean, o->prior_isig,
                              o->max_vsini, F, o->status, st);
}

int rvs_internal_grad_chain_eval(const rvs_nm_objective *o, const rvs_grad_chain *g,
                                 const int32_t *list, const double *X, int J,
                                 const int32_t *counts, int cidx, double *F,
                                 hipStream_t st, const rvs_fisher_chain *fc) {
  if (J < 1 || J > g->cap || (fc && (!fc->fisher_work || !fc->fisher)))
    return RVS_E_ARG;
  const int ndim = o->ndim, ntan = g->ntan;
  int rc = rvs_internal_proc_map(J, X, list, o, st);
  if (rc) return rc;
  const int R = 1 + ndim;
  for (int a = 0; a < g->narm; a++) {
    const rvs_grad_arm &A = g->arms[a];
    if (A.tri == 2) {
      const rvs_nm_nn_arm *N = static_cast<const rvs_nm_nn_arm *>(A.dats);
      rc = rvs_template_nn_grad(o->params, J, ndim, N->log_mask, N->M, N->S, N->nlayer,
                                N->W, N->b, N->dims, N->act0, N->act1, A.templ, st);
      if (rc) return rc;
      // (xeqs == NULL: nfx = nfy = 0, the flags are zeroed on the stream -- also
      // those of a job whose rows are NaN: include/rvsgpu.h, rvs_grad_arm)
      rc = rvs_nn_outside(N->xeqs ? o->params : nullptr, J, ndim, N->log_mask, N->M,
                          N->S, N->xeqs ? 0 : 1, N->xeqs, N->nfx, N->yeqs, N->nfy,
                          A.outside, st);
    } else if (!A.tri)
      rc = rvs_template_polylinear_grad(
          static_cast<const float *>(A.dats), A.ngrid, A.ntp, A.idgrid, A.uvecs, A.lens,
          ndim, A.vecs_s, A.ptp, A.log_mask, A.exp_flag, o->params, J, A.templ,
          A.outside, nullptr, nullptr, st);
    else if (A.buckets.cell_start)
      rc = rvs_template_tri_buckets_grad(
          static_cast<const double *>(A.dats), A.ntp, A.simplices, A.transform,
          A.extraflags, A.nsimplex, ndim, A.log_mask, A.exp_flag, &A.buckets, o->params,
          J, A.templ, A.outside, A.simplex, nullptr, st);
    else
      rc = rvs_template_tri_grad(static_cast<const double *>(A.dats), A.ntp,
                                 A.simplices, A.transform, A.extraflags, A.nsimplex,
                                 ndim, A.log_mask, A.exp_flag, o->params, J, A.templ,
                                 A.outside, A.simplex, nullptr, st);
    if (rc) return rc;
    const double *rows = A.templ;
    if (g->vsini_mode == 2) {   // R rows in, R + 1 out: the vsini tangent last
      rc = rvs_vsini_convolve_grad(A.templ, o->vsini, A.outside, A.lnstep, 0.6, A.ntp, R,
                                   J, A.templ2, st);
      if (rc) return rc;
      rows = A.templ2;
    } else if (g->vsini_mode == 1) {
      hipLaunchKernelGGL(grad_repeat_kernel, dim3((J * R + 255) / 256), dim3(256), 0, st,
                         J, R, o->vsini, A.outside, A.vs_rows, A.out_rows);
      RVS_LAUNCH_CHECK();
      rc = rvs_vsini_convolve(A.templ, A.vs_rows, A.out_rows, A.lnstep, 0.6, A.ntp,
                              J * R, A.templ2, st);
      if (rc) return rc;
      rows = A.templ2;
    }
    rc = rvs_spline_construct(A.knots, rows, A.ntp, J * (1 + ntan), A.spline_form,
                              A.factors, A.coef, st);
    if (rc) return rc;
    hipLaunchKernelGGL(grad_penalty_kernel, dim3((J + 255) / 256), dim3(256), 0, st, J,
                       A.outside, g->pen_scale, o->job_spec, o->badchi, A.penalty);
    RVS_LAUNCH_CHECK();
  }
  rc = rvs_internal_zero_jstatus(o, J, st);
  if (rc) return rc;
  // arms under a resolution matrix: the _resol entry points (R acts after the
  // resampling, so the template, FIR and spline stages above are as without)
  bool resol = false;
  for (int a = 0; a < g->narm; a++) resol = resol || g->point[a].taps;
  if (fc)   // the Fisher form of the last two calls
    rc = (resol ? rvs_chisq_point_fisher_resol : rvs_chisq_point_fisher)(
        g->point, g->narm, o->npoly, ntan, o->job_spec, nullptr, J, o->vel, o->badchi,
        g->basis_const, fc->fisher_work, g->chi, g->grad, fc->fisher, o->jstatus, st);
  else
    rc = (resol ? rvs_chisq_point_grad_resol : rvs_chisq_point_grad)(
        g->point, g->narm, o->npoly, ntan, o->job_spec, nullptr, J, o->vel, o->badchi,
        g->basis_const, g->point_work, g->chi, g->grad, o->jstatus, st);
  if (rc) return rc;
  return rvs_internal_proc_finish(o, g, fc ? fc->fisher : nullptr, X, J, counts, cidx, F,
                                  st);
}
