// bfgs_dev.hip -- the second minimiser of vel_fit.process on the device
// (vel_fit.py:653-658: scipy.optimize.minimize(method='BFGS', hess_inv0=...) from
// the simplex optimum; utils.py:26 makes it the reference's default).
//
// S runs of bfgs_machine.h -- the state machine the CPU suite pins to scipy through
// bfgs_host.cpp -- live in HBM, one thread per spectrum advances its run to the next
// request, and a round is
//   bfgs_advance_kernel  values of the last request -> run -> rows it needs next
//   rounds_scan_kernel   exclusive scan of the row counts: every run's first row,
//                        the rows of each launch chunk, the number of live runs
//   rounds_emit_kernel   the requested points into one list (spectrum order)
//   <objective>          rvs_proc_map -> objective kernel -> rvs_proc_finish per chunk
//                        of `cap` rows (nm.hip: the objective of rvs_nm_run)
// driven by rounds_run (rounds_dev.h), the one round driver of this file and of
// lm_dev.hip: the counts stay on the device, and when the host looks at them is its
// policy.  Every entry point here checks its arguments and hands rounds_run, through
// bfgs_rounds, how a chunk of rows is answered.
// The host-driven form of the same rounds (bfgs_host.cpp behind a Python objective)
// cost 1.6 ms per round in torch calls and copies: 0.35 s per 2000 spectra on 0.19 s
// of objective kernels.
#include "bfgs_machine.h"
#include "common.h"
#include "nm_internal.h"

using rvs_bfgs::Run;

#ifndef BF_NT
// advance: FOUR runs per block -- a run's state is 7.7 KB of its own, so every load of
// a wave touches as many cache lines as it has live lanes; few lanes per wave and many
// waves over the CUs: BFGS of 500 / 2000 spectra 0.088 / 0.227 -> 0.083 / 0.221 s
// against 64 runs per block (16: 0.085 / 0.224; tools/perf/ab_libs3.sh)
#define BF_NT 4
#endif

namespace {

__device__ inline const double *rounds_request_rows(const Run &r) { return r.rows; }

}  // namespace

#include "rounds_dev.h"   // scan, emit and the round driver (shared with lm_dev.hip)

namespace {

struct BfgsDev {
  Run *runs;
  int S, n, cap;
  const double *x0, *H0;
  double gtol, c1, c2, xrtol;
  int maxiter;
  int32_t *nreq, *off, *list, *counts;
  double *X, *F;
};

__global__ void __launch_bounds__(BF_NT) bfgs_advance_kernel(BfgsDev D, int first) {
  const int s = blockIdx.x * BF_NT + threadIdx.x;
  if (s >= D.S) return;
  Run &r = D.runs[s];
  if (first) {
    rvs_bfgs::init(r, D.n, D.x0 + (int64_t)s * D.n, D.H0, D.gtol, D.c1, D.c2, D.xrtol,
                   D.maxiter);
  } else {
    if (r.done) return;   // (nreq[s] is 0 since the round it finished in)
    const int m = r.nrows, o = D.off[s];
    for (int q = 0; q < m; q++) r.vals[q] = D.F[o + q];
  }
  rvs_bfgs::advance(r);
  D.nreq[s] = r.done ? 0 : r.nrows;
}

// jac mode (rvs_bfgs_run_grad): the second instantiation of the machine.  A run's one
// row was answered with (f, grad f) = F[row, 0 .. n]
__global__ void __launch_bounds__(BF_NT) bfgs_advance_jac_kernel(BfgsDev D, int first) {
  const int s = blockIdx.x * BF_NT + threadIdx.x;
  if (s >= D.S) return;
  Run &r = D.runs[s];
  if (first) {
    rvs_bfgs::init_jac(r, D.n, D.x0 + (int64_t)s * D.n, D.H0, D.gtol, D.c1, D.c2,
                       D.xrtol, D.maxiter);
  } else {
    if (r.done) return;
    const double *f = D.F + (int64_t)D.off[s] * (D.n + 1);
    for (int q = 0; q <= D.n; q++) r.vals[q] = f[q];
  }
  rvs_bfgs::advance_jac(r);
  D.nreq[s] = r.done ? 0 : r.nrows;
}

__global__ void __launch_bounds__(BF_NT)
    bfgs_result_kernel(BfgsDev D, double *x, double *fun, double *hess_inv,
                       int32_t *nit, int32_t *nfev, int32_t *status) {
  const int s = blockIdx.x * BF_NT + threadIdx.x;
  if (s >= D.S) return;
  const Run &r = D.runs[s];
  const int n = D.n;
  for (int i = 0; i < n; i++) x[(int64_t)s * n + i] = r.xk[i];
  fun[s] = r.fval;
  nit[s] = r.nit;
  nfev[s] = r.nfev;
  status[s] = r.done ? r.status : -1;
  if (hess_inv)
    for (int i = 0; i < n * n; i++) hess_inv[(int64_t)s * n * n + i] = r.Hk[i];
}

__global__ void __launch_bounds__(256) bfgs_njev_kernel(BfgsDev D, int32_t *njev) {
  const int s = blockIdx.x * 256 + threadIdx.x;
  if (s < D.S) njev[s] = D.runs[s].ngev;
}

}  // namespace

extern "C" int64_t rvs_bfgs_run_bytes(void) { return (int64_t)sizeof(Run); }

namespace {

// what every form asks of b and o beside its own checks
bool bfgs_args_ok(const rvs_bfgs_state *b, const rvs_nm_objective *o, int sync_every) {
  return b && o && b->S >= 1 && b->n >= 1 && b->n <= 8 && b->n == o->n &&
         sync_every >= 1 && b->runs && b->x0 && b->x && b->fun && b->nit && b->nfev &&
         b->status && b->nreq && b->off && b->list && b->X && b->F && b->counts;
}

// the rounds of the machine (rounds_run) over eval(list, X, J, chunk, F, stream).
// njev == NULL: rvs_bfgs_run -- a live run asks for up to n + 1 values, F [J]; else the
// jac form -- a live run asks for its one row, answered with (f, grad f), F [J, 1 + n]
template <class Eval>
int bfgs_rounds(const rvs_bfgs_state *b, int cap, int32_t *njev, int sync_every,
                int64_t *stats, void *stream, Eval eval) {
  const int S = b->S, n = b->n;
  BfgsDev D;
  rounds_fill(D, b, static_cast<Run *>(b->runs), cap);
  D.x0 = b->x0, D.H0 = b->hess_inv0;
  D.gtol = b->gtol, D.c1 = b->c1, D.c2 = b->c2, D.xrtol = b->xrtol;
  D.maxiter = b->maxiter;
  const dim3 agrid((S + BF_NT - 1) / BF_NT);
  return rounds_run(
      D, njev ? 1 : n + 1, njev ? n + 1 : 1, sync_every, stats, stream,
      [&](int first, hipStream_t st) {
        hipLaunchKernelGGL(njev ? bfgs_advance_jac_kernel : bfgs_advance_kernel, agrid,
                           dim3(BF_NT), 0, st, D, first);
      },
      eval,
      [&](hipStream_t st) {
        hipLaunchKernelGGL(bfgs_result_kernel, agrid, dim3(BF_NT), 0, st, D, b->x, b->fun,
                           b->hess_inv, b->nit, b->nfev, b->status);
        if (njev)
          hipLaunchKernelGGL(bfgs_njev_kernel, dim3((S + 255) / 256), dim3(256), 0, st, D,
                             njev);
      });
}

}  // namespace

extern "C" int rvs_bfgs_run(const rvs_bfgs_state *b, const rvs_nm_objective *o,
                            int sync_every, int64_t *stats, void *stream) {
  if (!bfgs_args_ok(b, o, sync_every)) return RVS_E_ARG;
  return bfgs_rounds(b, b->cap, nullptr, sync_every, stats, stream,
                     [&](const int32_t *list, const double *X, int J, int ch, double *F,
                         hipStream_t st) {
                       return rvs_internal_nm_eval(o, list, X, J, b->counts, ch, F, st);
                     });
}

// The polish on the exact gradient: every form runs bfgs_rounds with g->cap rows per
// chunk and differs in how a chunk's (f, grad f) come about -- here through the chain
extern "C" int rvs_bfgs_run_grad(const rvs_bfgs_state *b, const rvs_nm_objective *o,
                                 const rvs_grad_chain *g, int sync_every,
                                 int64_t *stats, void *stream) {
  if (!bfgs_args_ok(b, o, sync_every) || !g || !g->njev ||
      !rvs_internal_grad_chain_ok(g, o))
    return RVS_E_ARG;
  return bfgs_rounds(b, g->cap, g->njev, sync_every, stats, stream,
                     [&](const int32_t *list, const double *X, int J, int ch, double *F,
                         hipStream_t st) {
                       return rvs_internal_grad_chain_eval(o, g, list, X, J, b->counts,
                                                           ch, F, st);
                     });
}

namespace {

// an arm of a fused polish: plain (nm_internal.h), or -- resol: the _resol forms, DESIGN
// 4.27 -- with a resolution matrix the RESOL form of the gradient kernel takes (ndim 0:
// the from-template form)
bool bfgs_fused_arm_ok(bool resol, const rvs_objective_arm &A, int npoly, int ndim, int vg) {
  if (!resol) return rvs_internal_arm_plain(A);
  // (the band as rvs_objective_grad_resol takes it, refused here, before any launch: the
  // geometry, and taps of one matrix for all or of whole matrices per spectrum)
  return A.pt.G <= 1 && !A.pt.fast_interp &&
         (!A.pt.taps ||
          (rvs_objective_grad_resol_ok(npoly, A.pt.npix, A.ntp, ndim, A.pt.nd, vg) &&
           (A.pt.taps_stride == 0 ||
            A.pt.taps_stride >= (int64_t)A.pt.npix * A.pt.nd)));
}

// ... with the chain's stages between the map and the finish replaced by one
// rvs_objective_grad call (objective_grad.hip); resol: rvs_objective_grad_resol
int bfgs_run_grad_fused(bool resol, const rvs_bfgs_state *b, const rvs_nm_objective *o,
                        const rvs_grad_chain *g, const rvs_objective_arm *garms,
                        const double *basis_const, void *gwork, int sync_every,
                        int64_t *stats, void *stream) {
  if (!bfgs_args_ok(b, o, sync_every) || !g || !g->njev || !garms || !gwork ||
      !rvs_internal_grad_rows_ok(g, o, 4))
    return RVS_E_ARG;
  for (int a = 0; a < g->narm; a++)
    if (garms[a].ndim != o->ndim ||
        !bfgs_fused_arm_ok(resol, garms[a], o->npoly, o->ndim, g->vsini_mode == 2) ||
        !rvs_objective_grad_ok(o->npoly, garms[a].pt.npix, garms[a].ntp, o->ndim,
                               g->vsini_mode == 2))
      return RVS_E_ARG;
  return bfgs_rounds(
      b, g->cap, g->njev, sync_every, stats, stream,
      [&](const int32_t *list, const double *X, int J, int ch, double *F,
          hipStream_t st) {
        return rvs_internal_fused_eval(
            o, g, nullptr, list, X, J, b->counts, ch, F, st, [&] {
              return (resol ? rvs_objective_grad_resol : rvs_objective_grad)(
                  garms, g->narm, o->npoly, g->ntan, o->params, o->vsini, o->job_spec, J,
                  o->vel, o->badchi, basis_const, gwork, g->chi, g->grad, o->jstatus, st);
            });
      });
}

}  // namespace

extern "C" int rvs_bfgs_run_grad_fused(const rvs_bfgs_state *b,
                                       const rvs_nm_objective *o,
                                       const rvs_grad_chain *g,
                                       const rvs_objective_arm *garms,
                                       const double *basis_const, void *gwork,
                                       int sync_every, int64_t *stats, void *stream) {
  return bfgs_run_grad_fused(false, b, o, g, garms, basis_const, gwork, sync_every, stats,
                             stream);
}
extern "C" int rvs_bfgs_run_grad_fused_resol(const rvs_bfgs_state *b,
                                             const rvs_nm_objective *o,
                                             const rvs_grad_chain *g,
                                             const rvs_objective_arm *garms,
                                             const double *basis_const, void *gwork,
                                             int sync_every, int64_t *stats,
                                             void *stream) {
  return bfgs_run_grad_fused(true, b, o, g, garms, basis_const, gwork, sync_every, stats,
                             stream);
}

// ... on MLP libraries: the rows' template rows from the networks of o->nn,
// value, velocity and vsini components and the adjoint rows from one
// rvs_objective_grad_from_template call per chunk, the parameter components from the
// networks' reverse pass (rvs_template_nn_vjp per arm), the arms summed by
// rvs_objective_grad_join.  The adjoint rows and the reverse pass's work belong to the
// caller: tbar, vjp_work, gparams are HOST arrays of narm device pointers ([cap, ntp],
// rvs_template_nn_vjp_work_size(cap, ...) bytes, [cap, ndim]), grad_vv [cap, 1 + (vsini
// fitted)].
namespace {
int bfgs_run_grad_fused_nn(
    bool resol, const rvs_bfgs_state *b, const rvs_nm_objective *o,
    const rvs_grad_chain *g, const rvs_objective_arm *garms, const double *basis_const,
    void *gwork, double *const *tbar, void *const *vjp_work, double *const *gparams,
    double *grad_vv, int sync_every, int64_t *stats, void *stream) {
  if (!bfgs_args_ok(b, o, sync_every) || !g || !g->njev || !garms || !gwork || !tbar ||
      !vjp_work || !gparams || !grad_vv || !rvs_internal_grad_rows_ok(g, o, 6) || !o->nn)
    return RVS_E_ARG;
  const int vg = g->vsini_mode == 2 ? 1 : 0;
  const double *tp[RVS_MAX_ARMS], *op[RVS_MAX_ARMS];
  for (int a = 0; a < g->narm; a++) {
    const rvs_nm_nn_arm &N = o->nn[a];
    if (!tbar[a] || !vjp_work[a] || !gparams[a] || !N.templ || !N.outside || !N.dims ||
        N.dims[0] != o->ndim || N.nlayer < 1 || N.dims[N.nlayer] != garms[a].ntp ||
        !bfgs_fused_arm_ok(resol, garms[a], o->npoly, 0, vg) ||
        !rvs_objective_grad_from_template_ok(o->npoly, garms[a].pt.npix, garms[a].ntp, vg) ||
        rvs_template_nn_vjp_work_size(g->cap, N.nlayer, N.dims) <= 0)
      return RVS_E_ARG;
    tp[a] = N.templ;
    op[a] = N.outside;
  }
  return bfgs_rounds(
      b, g->cap, g->njev, sync_every, stats, stream,
      [&](const int32_t *list, const double *X, int J, int ch, double *F,
          hipStream_t st) {
        return rvs_internal_fused_eval(
            o, g, nullptr, list, X, J, b->counts, ch, F, st, [&] {
              int rc = rvs_template_nn_arms_n(o->params, J, nullptr, o->ndim, o->narm,
                                              o->nn, st);
              if (rc) return rc;
              rc = (resol ? rvs_objective_grad_from_template_resol
                          : rvs_objective_grad_from_template)(
                  garms, g->narm, o->npoly, vg, tp, op, o->vsini, o->job_spec, J, o->vel,
                  o->badchi, basis_const, gwork, tbar, g->chi, grad_vv, o->jstatus, st);
              if (rc) return rc;
              for (int a = 0; a < g->narm; a++) {
                const rvs_nm_nn_arm &N = o->nn[a];
                rc = rvs_template_nn_vjp(o->params, J, o->ndim, N.log_mask, N.M, N.S,
                                         N.nlayer, N.W, N.b, N.dims, N.templ, tbar[a],
                                         vjp_work[a], gparams[a], st);
                if (rc) return rc;
              }
              return rvs_objective_grad_join(g->narm, J, o->ndim, vg, gwork, gparams,
                                             g->chi, grad_vv, g->grad, st);
            });
      });
}

}  // namespace

extern "C" int rvs_bfgs_run_grad_fused_nn(
    const rvs_bfgs_state *b, const rvs_nm_objective *o, const rvs_grad_chain *g,
    const rvs_objective_arm *garms, const double *basis_const, void *gwork,
    double *const *tbar, void *const *vjp_work, double *const *gparams, double *grad_vv,
    int sync_every, int64_t *stats, void *stream) {
  return bfgs_run_grad_fused_nn(false, b, o, g, garms, basis_const, gwork, tbar, vjp_work,
                                gparams, grad_vv, sync_every, stats, stream);
}
extern "C" int rvs_bfgs_run_grad_fused_nn_resol(
    const rvs_bfgs_state *b, const rvs_nm_objective *o, const rvs_grad_chain *g,
    const rvs_objective_arm *garms, const double *basis_const, void *gwork,
    double *const *tbar, void *const *vjp_work, double *const *gparams, double *grad_vv,
    int sync_every, int64_t *stats, void *stream) {
  return bfgs_run_grad_fused_nn(true, b, o, g, garms, basis_const, gwork, tbar, vjp_work,
                                gparams, grad_vv, sync_every, stats, stream);
}

// ... on Delaunay libraries: the form above with the triangulations of
// o->tri as the evaluator -- the rows' template rows, outside flags and simplex ids from
// rvs_internal_template_tri_arms_n into the buffers of o->tri[a], and the parameter
// components from rvs_template_tri_vjp per arm on the simplex the evaluator found (the
// search is not repeated).  float64 throughout; the reverse step needs no work buffer.
// tbar, gparams: HOST arrays of narm device pointers ([cap, ntp], [cap, ndim]), grad_vv
// [cap, 1 + (vsini fitted)].
namespace {
int bfgs_run_grad_fused_tri(
    bool resol, const rvs_bfgs_state *b, const rvs_nm_objective *o,
    const rvs_grad_chain *g, const rvs_objective_arm *garms, const double *basis_const,
    void *gwork, double *const *tbar, double *const *gparams, double *grad_vv,
    int sync_every, int64_t *stats, void *stream) {
  if (!bfgs_args_ok(b, o, sync_every) || !g || !g->njev || !garms || !gwork || !tbar ||
      !gparams || !grad_vv || !rvs_internal_grad_rows_ok(g, o, 6) || !o->tri)
    return RVS_E_ARG;
  const int vg = g->vsini_mode == 2 ? 1 : 0;
  const double *tp[RVS_MAX_ARMS], *op[RVS_MAX_ARMS];
  for (int a = 0; a < g->narm; a++) {
    const rvs_nm_tri_arm &T = o->tri[a];
    if (!tbar[a] || !gparams[a] || !T.templ || !T.outside || !T.simplex || !T.dats ||
        !T.simplices || !T.transform || !T.buckets.cell_start || !T.buckets.cell_list ||
        T.nsimplex < 1 || T.ntp != garms[a].ntp ||
        !bfgs_fused_arm_ok(resol, garms[a], o->npoly, 0, vg) ||
        !rvs_objective_grad_from_template_ok(o->npoly, garms[a].pt.npix, garms[a].ntp, vg))
      return RVS_E_ARG;
    tp[a] = T.templ;
    op[a] = T.outside;
  }
  return bfgs_rounds(
      b, g->cap, g->njev, sync_every, stats, stream,
      [&](const int32_t *list, const double *X, int J, int ch, double *F,
          hipStream_t st) {
        return rvs_internal_fused_eval(
            o, g, nullptr, list, X, J, b->counts, ch, F, st, [&] {
              int rc = rvs_internal_template_tri_arms_n(o->params, J, nullptr, o->ndim,
                                                        o->narm, o->tri, st);
              if (rc) return rc;
              rc = (resol ? rvs_objective_grad_from_template_resol
                          : rvs_objective_grad_from_template)(
                  garms, g->narm, o->npoly, vg, tp, op, o->vsini, o->job_spec, J, o->vel,
                  o->badchi, basis_const, gwork, tbar, g->chi, grad_vv, o->jstatus, st);
              if (rc) return rc;
              for (int a = 0; a < g->narm; a++) {
                const rvs_nm_tri_arm &T = o->tri[a];
                rc = rvs_template_tri_vjp(T.dats, T.ntp, T.simplices, T.transform,
                                          T.nsimplex, o->ndim, T.log_mask, T.exp_flag,
                                          o->params, J, T.simplex, T.templ, tbar[a],
                                          gparams[a], st);
                if (rc) return rc;
              }
              return rvs_objective_grad_join(g->narm, J, o->ndim, vg, gwork, gparams,
                                             g->chi, grad_vv, g->grad, st);
            });
      });
}

}  // namespace

extern "C" int rvs_bfgs_run_grad_fused_tri(
    const rvs_bfgs_state *b, const rvs_nm_objective *o, const rvs_grad_chain *g,
    const rvs_objective_arm *garms, const double *basis_const, void *gwork,
    double *const *tbar, double *const *gparams, double *grad_vv, int sync_every,
    int64_t *stats, void *stream) {
  return bfgs_run_grad_fused_tri(false, b, o, g, garms, basis_const, gwork, tbar, gparams,
                                 grad_vv, sync_every, stats, stream);
}
extern "C" int rvs_bfgs_run_grad_fused_tri_resol(
    const rvs_bfgs_state *b, const rvs_nm_objective *o, const rvs_grad_chain *g,
    const rvs_objective_arm *garms, const double *basis_const, void *gwork,
    double *const *tbar, double *const *gparams, double *grad_vv, int sync_every,
    int64_t *stats, void *stream) {
  return bfgs_run_grad_fused_tri(true, b, o, g, garms, basis_const, gwork, tbar, gparams,
                                 grad_vv, sync_every, stats, stream);
}
