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
// driven by rounds_run (rounds_dev.h), the round driver this file shares with
// bfgs_dev.hip: the counts on the device, the host's looks at them its policy.
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

// the rounds of the machine (rounds_run) over eval(list, X, J, chunk, F, stream): a live
// run asks for its one row, answered with (f, grad f, H packed), F [J, npack(n)]
template <class Eval>
int lm_rounds(const rvs_lm_state *b, int cap, int sync_every, int64_t *stats,
              void *stream, Eval eval) {
  LmDev D;
  rounds_fill(D, b, static_cast<Run *>(b->runs), cap);
  D.x0 = b->x0;
  D.gtol = b->gtol, D.xtol = b->xtol, D.tau = b->tau, D.mu_max = b->mu_max;
  D.maxiter = b->maxiter;
  const dim3 agrid((b->S + LM_NT - 1) / LM_NT);
  return rounds_run(
      D, 1, rvs_lm::npack(b->n), sync_every, stats, stream,
      [&](int first, hipStream_t st) {
        hipLaunchKernelGGL(lm_advance_kernel, agrid, dim3(LM_NT), 0, st, D, first);
      },
      eval,
      [&](hipStream_t st) {
        hipLaunchKernelGGL(lm_result_kernel, agrid, dim3(LM_NT), 0, st, D, b->x, b->fun,
                           b->grad, b->hess, b->mu, b->nit, b->nfev, b->status);
      });
}

}  // namespace

extern "C" int rvs_lm_run(const rvs_lm_state *b, const rvs_nm_objective *o,
                          const rvs_grad_chain *g, const rvs_fisher_chain *fc,
                          int sync_every, int64_t *stats, void *stream) {
  if (!lm_args_ok(b, o, g, sync_every) || !fc || !fc->fisher_work || !fc->fisher ||
      !rvs_internal_grad_chain_ok(g, o))
    return RVS_E_ARG;
  return lm_rounds(b, g->cap, sync_every, stats, stream,
                   [&](const int32_t *list, const double *X, int J, int ch, double *F,
                       hipStream_t st) {
                     return rvs_internal_grad_chain_eval(o, g, list, X, J, b->counts, ch,
                                                         F, st, fc);
                   });
}

// ... with the chain's stages between the map and the finish replaced by one
// rvs_objective_fisher call (objective_fisher.hip).  fwork: the chunk's matrices
// [cap, K, K] first, the kernel's work buffer behind them
extern "C" int rvs_lm_run_fused(const rvs_lm_state *b, const rvs_nm_objective *o,
                                const rvs_grad_chain *g, const rvs_objective_arm *garms,
                                const double *basis_const, void *fwork,
                                int64_t fwork_bytes, int sync_every, int64_t *stats,
                                void *stream) {
  if (!lm_args_ok(b, o, g, sync_every) || !garms || !fwork ||
      !rvs_internal_grad_rows_ok(g, o, 4))
    return RVS_E_ARG;
  int npix_max = 0;
  for (int a = 0; a < g->narm; a++) {
    if (garms[a].ndim != o->ndim || !rvs_internal_arm_plain(garms[a]) ||
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
  return lm_rounds(
      b, g->cap, sync_every, stats, stream,
      [&](const int32_t *list, const double *X, int J, int ch, double *F,
          hipStream_t st) {
        return rvs_internal_fused_eval(
            o, g, fisher, list, X, J, b->counts, ch, F, st, [&] {
              return rvs_objective_fisher(garms, g->narm, o->npoly, g->ntan, o->params,
                                          o->vsini, o->job_spec, J, o->vel, o->badchi,
                                          basis_const, kwork, kwork_bytes, g->chi, g->grad,
                                          fisher, o->jstatus, st);
            });
      });
}
