// lm_dev.hip -- the Levenberg-Marquardt polish of vel_fit.process
// (config['second_minimizer_lm']) with its rounds on the device.
//
// S runs of lm_machine.h -- the state machine the CPU suite holds against
// tests/refmachines/lm_restated.py through lm_host.cpp -- live in HBM, one thread per
// spectrum advances its run to its next request, and a round is
//   lm_advance_kernel    (f, g, H) of the last request -> run -> the row it needs next:
//                        the scaled n <= 8 Cholesky factor and the two triangular solves
//   rounds_scan_kernel   \ what rvs_bfgs_run_grad launches (rounds_dev.h): every run's
//   rounds_emit_kernel   / row, the rows of each chunk, the live runs; the rows' list
//   <objective>          per chunk of g->cap rows the Fisher form of the gradient chain
//                        (bfgs_grad.hip: ... rvs_chisq_point_fisher ->
//                        rvs_proc_finish_fisher), or -- rvs_lm_run_fused -- one
//                        rvs_objective_fisher call (objective_fisher.hip) between
//                        rvs_proc_map and rvs_proc_finish_fisher
// with the counts on the device and the host looking at them under rvs_bfgs_run's policy.
#include "common.h"
#include "lm_machine.h"
#include "nm_internal.h"

using rvs_lm::Run;

#ifndef LM_NT
// runs per block of the advance and result kernels.  A run's state is 0.6 KB of its own
// in HBM and its path is its own, so few lanes per wave and many waves over the CUs, as
// for bfgs_advance_kernel; 16 is not a measured optimum
#define LM_NT 16
#endif

namespace {

__device__ inline const double *rounds_request_rows(const Run &r) { return r.xt; }

}  // namespace

#include "rounds_dev.h"

namespace {

struct LmDev {
  Run *runs;
  int S, n, cap;
  const double *x0;
  double gtol, xtol, tau, mu_max;
  int maxiter;
  int32_t *nreq, *off, *list, *counts;
  double *X, *F;
};

__global__ void __launch_bounds__(LM_NT) lm_advance_kernel(LmDev D, int first) {
  const int s = blockIdx.x * LM_NT + threadIdx.x;
  if (s >= D.S) return;
  Run &r = D.runs[s];
  if (first) {
    rvs_lm::init(r, D.n, D.x0 + (int64_t)s * D.n, D.gtol, D.xtol, D.tau, D.mu_max,
                 D.maxiter);
    rvs_lm::advance(r, nullptr);
  } else {
    if (r.done) return;   // (nreq[s] is 0 since the round it finished in)
    rvs_lm::advance(r, D.F + (int64_t)D.off[s] * rvs_lm::npack(D.n));
  }
  D.nreq[s] = (!r.done && r.pending) ? 1 : 0;
}

__global__ void __launch_bounds__(LM_NT)
    lm_result_kernel(LmDev D, double *x, double *fun, double *grad, double *hess,
                     double *mu, int32_t *nit, int32_t *nfev, int32_t *status) {
  const int s = blockIdx.x * LM_NT + threadIdx.x;
  if (s >= D.S) return;
  const Run &r = D.runs[s];
  const int n = D.n;
  for (int i = 0; i < n; i++) {
    x[(int64_t)s * n + i] = r.x[i];
    grad[(int64_t)s * n + i] = r.g[i];
  }
  fun[s] = r.f;
  mu[s] = r.mu;
  nit[s] = r.nit;
  nfev[s] = r.nfev;
  status[s] = r.done ? r.status : -1;
  if (hess) rvs_lm::unpack_hess(r, hess + (int64_t)s * n * n);
}

}  // namespace

extern "C" int64_t rvs_lm_run_bytes(void) { return (int64_t)sizeof(Run); }

namespace {

// what both forms of the polish ask of b and o beside their own checks
bool lm_args_ok(const rvs_lm_state *b, const rvs_nm_objective *o, const rvs_grad_chain *g,
                int sync_every) {
  return b && o && g && b->S >= 1 && b->n >= 1 && b->n <= rvs_lm::MAXN && b->n == o->n &&
         sync_every >= 1 && b->runs && b->x0 && b->x && b->fun && b->grad && b->mu &&
         b->nit && b->nfev && b->status && b->nreq && b->off && b->list && b->X && b->F &&
         b->counts;
}

// the rounds of rvs_lm_run over eval(list, X, J, chunk, F, stream): (f, grad f, H packed)
// of a chunk of rows into F [J, npack(n)]
template <class Eval>
int lm_run_rows(const rvs_lm_state *b, int cap, int sync_every, int64_t *stats,
                void *stream, Eval eval) {
  const int S = b->S, n = b->n;
  const int m = rvs_lm::npack(n);
  const int64_t maxrows = S;   // one row per live run
  if (cap < 1 || (maxrows + cap - 1) / cap > BF_NCHUNK) return RVS_E_ARG;
  hipStream_t st = rvs_stream(stream);
  LmDev D;
  D.runs = static_cast<Run *>(b->runs);
  D.S = S, D.n = n, D.cap = cap;
  D.x0 = b->x0;
  D.gtol = b->gtol, D.xtol = b->xtol, D.tau = b->tau, D.mu_max = b->mu_max;
  D.maxiter = b->maxiter;
  D.nreq = b->nreq, D.off = b->off, D.list = b->list, D.counts = b->counts;
  D.X = b->X, D.F = b->F;
  const dim3 agrid((S + LM_NT - 1) / LM_NT);
  const dim3 egrid((int)(((int64_t)S * (n + 1) + 255) / 256));
  auto step = [&](int first) {
    hipLaunchKernelGGL(lm_advance_kernel, agrid, dim3(LM_NT), 0, st, D, first);
    hipLaunchKernelGGL(rounds_scan_kernel<LmDev>, dim3(1), dim3(BF_SCAN_NT), 0, st, D);
    hipLaunchKernelGGL(rounds_emit_kernel<LmDev>, egrid, dim3(256), 0, st, D);
  };
  step(1);
  RVS_LAUNCH_CHECK();
  int64_t rounds = 0, calls = 0, jobs = 0;
  int32_t c[BF_NCHUNK + 8];
  while (true) {
    if (hipMemcpyAsync(c, b->counts, sizeof(int32_t) * (BF_NCHUNK + 2),
                       hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return RVS_E_LAUNCH;
    const int64_t total = c[BF_NCHUNK], live = c[BF_NCHUNK + 1];
    if (total == 0) break;
    // (the policy of rvs_bfgs_run; behind the look every live run asks for at most
    // its one row)
    const int window = (total > 4096) ? 1 : sync_every;
    for (int r = 0; r < window; r++) {
      int64_t bound = (r == 0) ? total : live;
      if (bound > maxrows) bound = maxrows;
      for (int64_t a = 0, ch = 0; a < bound; a += cap, ch++) {
        const int J = (int)((bound - a < cap) ? bound - a : cap);
        int rc = eval(b->list + a, b->X + a * n, J, (int)ch, b->F + a * m, st);
        if (rc) return rc;
        calls++;
        jobs += J;
      }
      step(0);
      RVS_LAUNCH_CHECK();
      rounds++;
    }
  }
  hipLaunchKernelGGL(lm_result_kernel, agrid, dim3(LM_NT), 0, st, D, b->x, b->fun,
                     b->grad, b->hess, b->mu, b->nit, b->nfev, b->status);
  RVS_LAUNCH_CHECK();
  if (hipStreamSynchronize(st) != hipSuccess) return RVS_E_LAUNCH;
  if (stats) {
    stats[0] = rounds;
    stats[1] = calls;
    stats[2] = jobs;
  }
  return 0;
}

}  // namespace

extern "C" int rvs_lm_run(const rvs_lm_state *b, const rvs_nm_objective *o,
                          const rvs_grad_chain *g, const rvs_fisher_chain *fc,
                          int sync_every, int64_t *stats, void *stream) {
  if (!lm_args_ok(b, o, g, sync_every) || !fc || !fc->fisher_work || !fc->fisher ||
      !rvs_internal_grad_chain_ok(g, o))
    return RVS_E_ARG;
  return lm_run_rows(b, g->cap, sync_every, stats, stream,
                     [&](const int32_t *list, const double *X, int J, int ch, double *F,
                         hipStream_t st) {
                       return rvs_internal_grad_chain_eval(o, g, list, X, J, b->counts, ch,
                                                           F, st, fc);
                     });
}

// ... with the chain's stages between rvs_proc_map and rvs_proc_finish_fisher replaced by
// one rvs_objective_fisher call (objective_fisher.hip).  fwork: the chunk's matrices
// [cap, K, K] first, the kernel's work buffer behind them
extern "C" int rvs_lm_run_fused(const rvs_lm_state *b, const rvs_nm_objective *o,
                                const rvs_grad_chain *g, const rvs_objective_arm *garms,
                                const double *basis_const, void *fwork,
                                int64_t fwork_bytes, int sync_every, int64_t *stats,
                                void *stream) {
  if (!lm_args_ok(b, o, g, sync_every) || !garms || !fwork || !g->chi || !g->grad ||
      g->cap < 1 || g->narm < 1 || g->narm > RVS_MAX_ARMS || g->narm != o->narm ||
      g->vsini_mode < 0 || g->vsini_mode > 2 || o->ndim < 1 || o->ndim > 4 ||
      g->ntan != o->ndim + (g->vsini_mode == 2 ? 1 : 0) ||
      (g->vsini_mode == 2) != (o->vsini_col >= 0) ||
      (g->vsini_mode != 0) != (o->vsini != nullptr) || !o->vel || !o->params ||
      !o->extra || !o->bad || !o->job_spec || !o->jstatus || !o->status || !o->fixed ||
      !o->safe)
    return RVS_E_ARG;
  int npix_max = 0;
  for (int a = 0; a < g->narm; a++) {
    if (garms[a].ndim != o->ndim || garms[a].pt.taps || garms[a].pt.G > 1 ||
        garms[a].pt.fast_interp ||
        !rvs_objective_fisher_ok(o->npoly, garms[a].pt.npix, garms[a].ntp, o->ndim,
                                 g->vsini_mode == 2))
      return RVS_E_ARG;
    npix_max = garms[a].pt.npix > npix_max ? garms[a].pt.npix : npix_max;
  }
  const int64_t K = 1 + g->ntan;
  const int64_t fisher_bytes = (int64_t)g->cap * K * K * (int64_t)sizeof(double);
  if (fwork_bytes < fisher_bytes +
                        rvs_objective_fisher_work_size(1, g->narm, g->ntan, npix_max))
    return RVS_E_ARG;
  double *fisher = static_cast<double *>(fwork);
  void *kwork = fisher + (int64_t)g->cap * K * K;
  const int64_t kwork_bytes = fwork_bytes - fisher_bytes;
  return lm_run_rows(
      b, g->cap, sync_every, stats, stream,
      [&](const int32_t *list, const double *X, int J, int ch, double *F,
          hipStream_t st) {
        int rc = rvs_proc_map(J, o->n, o->ndim, X, list, o->src, o->vsini_col, o->fixed,
                              o->vsini_fixed, o->safe, o->prior_mean, o->prior_isig,
                              o->min_vel, o->max_vel, o->max_vsini, o->job_spec, o->vel,
                              o->vsini, o->params, o->extra, o->bad, st);
        if (rc) return rc;
        if (hipMemsetAsync(o->jstatus, 0, sizeof(int32_t) * J, st) != hipSuccess)
          return RVS_E_LAUNCH;
        rc = rvs_objective_fisher(garms, g->narm, o->npoly, g->ntan, o->params, o->vsini,
                                  o->job_spec, J, o->vel, o->badchi, basis_const, kwork,
                                  kwork_bytes, g->chi, g->grad, fisher, o->jstatus, st);
        if (rc) return rc;
        return rvs_proc_finish_fisher(J, o->n, o->ndim, g->ntan, b->counts, ch, g->chi,
                                      g->grad, fisher, X, o->params, o->extra, o->bad,
                                      o->job_spec, o->jstatus, o->src, o->vsini_col,
                                      o->prior_mean, o->prior_isig, o->max_vsini, F,
                                      o->status, st);
      });
}
