// Internal (not exported) entries shared by nm.hip, bfgs_grad.hip, bfgs_dev.hip and
// lm_dev.hip: the objective of a chunk of rows on the row buffers of `o`, whole and in
// the steps the fused forms put their own kernels between.
#pragma once
#include "common.h"

#define RVS_HIDDEN __attribute__((visibility("hidden")))

// template.hip: the rows of a round through the Delaunay evaluators of all arms
RVS_HIDDEN int rvs_internal_template_tri_arms_n(const double *params, int B,
                                                const int32_t *live, int ndim, int narm,
                                                const rvs_nm_tri_arm *arms,
                                                hipStream_t st);

// nm.hip: rvs_proc_map on `o`: X [J, n] of spectra list[j] -> o->vel, vsini, params,
// extra (prior / vsini penalty), bad, job_spec
RVS_HIDDEN int rvs_internal_proc_map(int J, const double *X, const int32_t *list,
                                     const rvs_nm_objective *o, hipStream_t st);

// the status words of the J rows start at zero
static inline int rvs_internal_zero_jstatus(const rvs_nm_objective *o, int J,
                                            hipStream_t st) {
  return hipMemsetAsync(o->jstatus, 0, sizeof(int32_t) * J, st) == hipSuccess
             ? 0 : RVS_E_LAUNCH;
}

// nm.hip: F[j] = chisq_func(X[j]) for spectrum list[j], j < min(J, counts[cidx]) (counts
// == NULL: all J): the map -> the objective (rvs_objective_fused_n, or
// rvs_template_nn_arms_n + rvs_objective_from_template_n for MLP libraries) ->
// rvs_proc_finish, on the row buffers of `o` (capacity >= J rows).
RVS_HIDDEN int rvs_internal_nm_eval(const rvs_nm_objective *o, const int32_t *list,
                                    const double *X, int J, const int32_t *counts,
                                    int cidx, double *F, hipStream_t st);

// bfgs_grad.hip: g and o fit each other (arms, vsini mode, tangents against o->ndim <=
// max_ndim: 4 for the regular-grid kernels, 6 for the chain and the MLP form) and the row
// buffers of both are there
RVS_HIDDEN int rvs_internal_grad_rows_ok(const rvs_grad_chain *g,
                                         const rvs_nm_objective *o, int max_ndim);

// an arm the fused kernels take: no resolution matrix, one wavelength grid, exact
// interpolation
static inline bool rvs_internal_arm_plain(const rvs_objective_arm &A) {
  return !A.pt.taps && A.pt.G <= 1 && !A.pt.fast_interp;
}

// bfgs_grad.hip: F [J, 1 + n] = rvs_proc_finish_grad of g->chi, g->grad on `o`; with
// fisher [J, 1 + ntan, 1 + ntan]: F [J, 1 + n + n (n + 1) / 2] = rvs_proc_finish_fisher
RVS_HIDDEN int rvs_internal_proc_finish(const rvs_nm_objective *o,
                                        const rvs_grad_chain *g, const double *fisher,
                                        const double *X, int J, const int32_t *counts,
                                        int cidx, double *F, hipStream_t st);

// a chunk of rows as the fused forms evaluate it: the map, the status words, rows()
// -- the form's own kernels, g->chi and g->grad (and fisher) of the mapped rows -- and
// the finish
template <class Rows>
int rvs_internal_fused_eval(const rvs_nm_objective *o, const rvs_grad_chain *g,
                            const double *fisher, const int32_t *list, const double *X,
                            int J, const int32_t *counts, int cidx, double *F,
                            hipStream_t st, Rows rows) {
  int rc = rvs_internal_proc_map(J, X, list, o, st);
  if (!rc) rc = rvs_internal_zero_jstatus(o, J, st);
  if (!rc) rc = rows();
  if (rc) return rc;
  return rvs_internal_proc_finish(o, g, fisher, X, J, counts, cidx, F, st);
}

// bfgs_grad.hip: (f, grad f) of the rows (list, X) through the gradient chain `g`:
// F [J, 1 + n], J <= g->cap; _ok: the descriptors fit each other (checked once per run).
// fc != NULL: the Fisher form of the last two calls (rvs_chisq_point_fisher,
// rvs_proc_finish_fisher), F [J, 1 + n + n (n + 1) / 2]
RVS_HIDDEN int rvs_internal_grad_chain_ok(const rvs_grad_chain *g,
                                          const rvs_nm_objective *o);
RVS_HIDDEN int rvs_internal_grad_chain_eval(const rvs_nm_objective *o,
                                            const rvs_grad_chain *g, const int32_t *list,
                                            const double *X, int J, const int32_t *counts,
                                            int cidx, double *F, hipStream_t st,
                                            const rvs_fisher_chain *fc = nullptr);
