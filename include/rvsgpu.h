/*
 * rvsgpu.h -- C-ABI of librvsgpu.so, the MI355X (gfx950) implementation of the
 * rvspecfit likelihood hot path.
 *
 * Conventions (they follow the reference's only C-ABI, py/rvspecfit/ffibuilder.py:10-17,
 * i.e. `construct` / `evaler` of py/rvspecfit/src/spliner.c):
 *   - extern "C", plain pointers and sizes, no torch / C++ types;
 *   - the CALLER owns every buffer; the callee never allocates or retains memory;
 *   - every pointer is a DEVICE pointer (HBM) unless the comment says "host";
 *   - all floating point data is float64 (the reference computes in float64),
 *     except the template grid `dats` and the NN weights which are float32 as in
 *     the reference's artefacts;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *     launches are asynchronous, nothing synchronises;
 *   - return value: 0 ok; <0 argument / shape / launch error (RVS_E_*).
 *     Per-spectrum conditions that the reference reports through Python
 *     exceptions are returned as bit flags in an int32 `status[]` output
 *     (RVS_ST_*); the Python layer re-raises the reference's exception types
 *     for batch-of-1 calls.
 *
 * Citations below are relative to /root/reference/py/rvspecfit/.
 */
#ifndef RVSGPU_H
#define RVSGPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVS_E_ARG (-1)     /* bad argument / unsupported shape */
#define RVS_E_LAUNCH (-2)  /* hipLaunch failure (hipGetLastError != 0) */

/* per-job status bits */
#define RVS_ST_SPLINE_RANGE 0x1   /* evaler() == -1 : eval point outside knots (spliner.c:78-83)  */
#define RVS_ST_SPLINE_GRID 0x2    /* evaler() == -2 : knots not uniform (spliner.c:87,95)          */
#define RVS_ST_NONFINITE 0x4      /* non finite -2 log L (spec_fit.py:963-974)                     */
#define RVS_ST_CHOL_FALLBACK 0x8  /* Cholesky failed, eigen (SVD) branch used (spec_fit.py:337-354) */
#define RVS_ST_OUTSIDE_NAN 0x10   /* template outside grid & not finite (spec_fit.py:392-397)      */
#define RVS_ST_CCF_FAILED 0x20    /* non finite CCF minimum (fitter_ccf.py:234-236)                 */
#define RVS_ST_ALLMASKED 0x40     /* every pixel masked in CCF preprocessing (make_ccf.py:311-315)  */
#define RVS_ST_QUAD_ASSERT 0x80   /* parabola vertex outside its bracket (spec_fit.py:1014 assert)  */
#define RVS_ST_ILLCOND 0x100      /* rvs_chisq_grid, rvs_chisq_grid_resol: normal matrix pivots span > 1e9 (long stretch of weightless pixels); re-evaluate the job with rvs_chisq_point */
#define RVS_ST_NONPOS_MEDIAN 0x200 /* rvs_ccf_models_build: median of the model row <= 0 (make_ccf.py:133-138) */
#define RVS_ST_RBF_NOTPD 0x400    /* rvs_rbf_factor: a pivot of the Cholesky factorisation is not positive (duplicate nodes: scipy's "Singular matrix") */

/* library version / build probe (host).  RVS_ABI_VERSION changes whenever the
 * meaning of an argument, a status bit or a work-size formula changes; a caller
 * compares rvs_abi_version() with the header it was built against
 * (rvspecfit_amd/_lib.py refuses a stale librvsgpu.so).
 *   2: status bit 0x100 = RVS_ST_ILLCOND; rvs_chisq_grid's int after `beta` is
 *      pack_min_jobs; rvs_chisq_continuum_work_size = 8 doubles per spectrum
 *   3: rvs_template_polylinear / rvs_objective_arm take `ptp` (the query is
 *      p / ptp as in spec_inter.py:130-132), not its reciprocal
 *   4: rvs_objective_work_size grew (the cell-search records of the objective's
 *      locate pass live in the caller's scratch)
 *   5: rvs_nn_outside added; rvs_chisq_grid packs left-over velocities from
 *      2000 jobs up by default (pack_min_jobs = 0)
 *   6: rvs_nm_objective.nn (MLP evaluators inside rvs_nm_run),
 *      rvs_template_nn_arms
 *   7: grid sets -- spectra of one arm on different wavelength grids in one batch
 *      (spec_fit.py:70-145 takes any `lam` per object): rvs_chisq_work_size_g,
 *      rvs_chisq_prepare_g, rvs_chisq_grid_g, rvs_chisq_full_g,
 *      rvs_chisq_continuum_g, rvs_ccf_preprocess_g; rvs_point_arm grew (grid_id,
 *      polys_stride, G); rvs_objective_work_size grew (the jobs' cell order);
 *      rvs_nn_outside accepts nfx = nfy = 0; rvs_basis_build, rvs_ccf_tables_build
 *      (the per-grid tables on the device)
 *   8: rvs_chisq_work_size(_g) grew by 2*S*npix doubles: rvs_chisq_prepare also
 *      leaves {1/e, s/e} per spectrum pixel (e with espec_sys in quadrature), which
 *      rvs_objective_fused / rvs_nm_run read instead of spec / espec;
 *      rvs_objective_fused_n / rvs_objective_from_template_n (job count on the
 *      device)
 *   9: rvs_option_set / rvs_option_get (the behaviour switches, no longer read from
 *      the environment at launch time); rvs_basis_build takes npoly <= 32 and
 *      npix <= 16384; espec = +inf marks padding only when G > 1
 *  10: rvs_chisq_full(_g) takes unit_template = 2 (the template given on the
 *      pixels: get_chisq0 itself); rvs_objective_fused refuses npoly > 10 on a
 *      template of 2 ntp < 8 (npoly (npoly + 3) / 2 + 1) knots
 *  11: rvs_spline_factors writes rvs_spline_factors_len(ntp) doubles (the five arrays
 *      of ntp, then the same factors in the objective kernel's chunk order); the cell
 *      record of rvs_objective_work_size grew by three doubles per (job, arm);
 *      rvs_chisq_work_size(_g) grew by 2*G*npix doubles ({lam, pix} pairs);
 *      options nm_split_min, nm_spec_max, nm_tail_window (additions: no signature
 *      changed);
 *      rvs_nm_run uses counts[5] (rows of a round that evaluates all candidates)
 *  12: rvs_bfgs_run / rvs_bfgs_run_bytes (the second minimiser's rounds on the
 *      device), rvs_chisq_grid_resol_g (resolution matrices on grid sets),
 *      rvs_template_tri_buckets (find_simplex through a bucket grid);
 *      rvs_nm_objective grew by `tri` (Delaunay libraries inside rvs_nm_run),
 *      rvs_nm_state by `stop_below`
 *  13: rvs_objective_fused(_n) / rvs_objective_from_template(_n) -- and with them
 *      rvs_nm_run / rvs_bfgs_run -- apply pt.taps (until now RVS_E_ARG) where
 *      rvs_objective_resol_ok (added) admits the arm
 *  14: removed: rvs_nm_state.stop_below (and its padding word), options "xc_ws1",
 *      "nm_glue", "nm_bucket"
 *  15: rvs_ccf_models_build, rvs_ccf_model_rows (CCF template sets from model rows);
 *      status bit 0x200 = RVS_ST_NONPOS_MEDIAN
 *  16: rvs_rebin_weights, rvs_rebin_apply, rvs_template_normalize (template libraries
 *      from high-resolution models)
 *  17: rvs_rbf_work_size, rvs_rbf_factor, rvs_rbf_solve, rvs_rbf_eval (multiquadric
 *      interpolation of template rows: regularize_grid); status bit 0x400 =
 *      RVS_ST_RBF_NOTPD
 *  18: rvs_nn_train_work_size, rvs_nn_train_grad, rvs_nn_adam_step,
 *      rvs_nn_train_epoch (training of the MLP rvs_template_nn evaluates)
 *      (still 18: rvs_template_polylinear_grad, rvs_chisq_point_grad_work_size and
 *      rvs_chisq_point_grad -- the objective's analytic gradient -- are additions;
 *      no argument, status bit or work-size formula of an existing entry point
 *      changed, so a caller built against 18 is served as before; likewise
 *      rvs_vsini_convolve_grad, the broadening with its vsini tangent row, and
 *      rvs_template_tri_grad / rvs_template_tri_buckets_grad, the Delaunay
 *      evaluator with its tangent rows; and rvs_chisq_point_fisher_work_size /
 *      rvs_chisq_point_fisher, the Fisher matrix of the marginalised fit; and
 *      rvs_template_nn_grad, the MLP evaluator with its tangent rows, with
 *      rvs_grad_arm.tri == 2 -- until now one of the non-zero values that meant
 *      Delaunay; the tree's callers write 1 for that -- naming an MLP arm of the
 *      gradient chain; and the Levenberg-Marquardt polish: rvs_proc_finish_fisher,
 *      rvs_fisher_chain_work_size, rvs_lm_begin / _pending / _feed / _result / _end,
 *      rvs_lm_run_bytes and rvs_lm_run with the new structs rvs_fisher_chain and
 *      rvs_lm_state -- rvs_grad_chain and every other struct keep their layout; and
 *      rvs_chisq_point_grad_resol / rvs_chisq_point_fisher_resol with their work
 *      sizes, the gradient and the Fisher matrix under resolution matrices:
 *      rvs_chisq_point_grad and rvs_chisq_point_fisher go on refusing taps; and the
 *      joint fit of a star's epochs: rvs_epoch_map, rvs_epoch_finish,
 *      rvs_alm_row_size, rvs_alm_begin / _pending / _feed / _result / _end,
 *      rvs_alm_run_bytes and rvs_alm_run with the new structs rvs_epoch_chain and
 *      rvs_alm_state; and rvs_chisq_grid_tab / rvs_chisq_grid_tab_work_size, the
 *      velocity grid on a per-node table of resampled templates, with the option
 *      "cg_tab"; and rvs_objective_fisher_ok / rvs_objective_fisher_work_size /
 *      rvs_objective_fisher, value, gradient and Fisher matrix in one forward-mode
 *      kernel per (job, arm), with rvs_lm_run_fused, the Levenberg-Marquardt rounds on
 *      it; and rvs_objective_grad_from_template with its _ok and _work_size,
 *      rvs_objective_grad_join, rvs_template_nn_vjp and rvs_template_nn_vjp_work_size:
 *      value and gradient on MLP libraries by one adjoint row back through the net,
 *      with rvs_bfgs_run_grad_fused_nn, the BFGS rounds on it; and
 *      rvs_template_tri_vjp (spec_inter.py:11-59 differentiated and contracted with one
 *      adjoint row), the reverse step of the Delaunay evaluator, with
 *      rvs_bfgs_run_grad_fused_tri (vel_fit.py:653-658 on that gradient), the BFGS
 *      rounds on it; and rvs_objective_grad_resol, rvs_objective_grad_from_template_resol
 *      and rvs_objective_grad_resol_ok, value and gradient in one kernel under resolution
 *      matrices, with rvs_bfgs_run_grad_fused_resol / _nn_resol / _tri_resol, the BFGS
 *      rounds on them: the entry points without the suffix go on refusing taps) */
#define RVS_ABI_VERSION 18
int rvs_abi_version(void);

/* ------------------------------------------------------------------------
 * Behaviour switches.  The entry points may be driven from several host threads
 * (vel_fit.process runs its halves on two), so no switch is read from the
 * environment at launch time.  The table is filled once, on first use, from the
 * environment variables RVS_<NAME in upper case>; afterwards only rvs_option_set
 * changes it, and a change takes effect at the next call that looks.  Every
 * setting gives the same results (to the bit, or -- xc_ws -- to a few ulp); the
 * switches exist so that tests can hold one kernel path against another.
 *   "xc_ws"          1  rvs_ccf_xcorr: the wave-specialised persistent kernels
 *                       where they apply; 0 = one block per (spectrum, template)
 *   "nm_split_min" 1024 rvs_nm_run: rounds of at least this many rows (and the test
 *                       of all simplices at the start and after a shrink, for at
 *                       least this many simplices) run their bookkeeping as a
 *                       row-parallel kernel + a one-block pack
 *   "nm_spec_max"   21  rvs_nm_run: rounds of at most this many rows (<= 64, and a
 *                       quarter of the simplices) evaluate all four candidate points
 *                       of a step in one launch, with one bookkeeping kernel per
 *                       round (same state, bit for bit); 0 = never
 *   "nm_tail_window" 16 rvs_nm_run: rounds between two looks of the host (counter
 *                       copy + stream synchronisation) once <= 256 rows are live,
 *                       if larger than sync_every
 *   "obj_inblk_max" 768 objective launches of <= this many blocks search their grid
 *                       cell inside the block (0 = never)
 *   "obj_sort"       1  objective jobs evaluated in grid-cell order
 *   "nn_pipe"        1  rvs_template_nn(_arms): the wide last layer through the kernel
 *                       whose epilogue runs under the next tile's products (K of 128,
 *                       200 or 256 inputs); 0 = the generic kernel (same bits)
 *   "cg_tab"         1  rvs_chisq_grid_tab: full waves stream the node templates
 *                       from the per-velocity table where its gate admits the
 *                       call; 0 = always rvs_chisq_grid_g's kernels (same bits)
 * Both return 0, or RVS_E_ARG for an unknown name / NULL value pointer.
 * ---------------------------------------------------------------------- */
int rvs_option_set(const char *name, int value);
int rvs_option_get(const char *name, int *value);

/* ------------------------------------------------------------------------
 * A3  polylinear template evaluation on a regular n-D grid
 *     replaces spec_inter.GridInterp.__call__ (spec_inter.py:134-194),
 *     GridOutsideCheck.__call__ (:77-92) and LogParamMapper.forward
 *     (read_grid.py:127-145), composed as SpecInterpolator.eval/outsideFlag
 *     (spec_inter.py:257-286) + the MAX_VAL guard of getCurTempl
 *     (spec_fit.py:392-397).
 *
 * dats      float32 [ngrid, ntp]  log-flux rows (interpdat_%s.npy)
 * idgrid    int64   [prod(lens)]  row of dats or -1 (C order)
 * uvecs     float64 [sum(lens)]   concatenated unique mapped grid values
 * lens      int32   [ndim] (host)
 * vecs_s    float64 [ngrid, ndim] grid points divided by ptp (KD-tree space)
 * ptp       float64 [ndim] (host) np.ptp(vec, axis=1): the query is p / ptp
 * log_mask  bit i set -> parameter i is mapped through log10
 * params    float64 [B, ndim]     physical parameters
 * templ     float64 [B, ntp]  out  exp'ed template
 * outside   float64 [B]       out  0 inside; KD distance outside; NaN if the
 *                                   template is non finite / > 1e100 outside
 * cellinfo  int32   [B, 2+2^ndim] out (nullable) {mode, nearest, vertex ids}
 *           mode 0 = polylinear, 1 = nearest neighbour, 2 = non finite params
 * weights   float64 [B, 2^ndim]  out (nullable) polylinear weights
 * ---------------------------------------------------------------------- */
int rvs_template_polylinear(const float *dats, int64_t ngrid, int ntp,
                            const int64_t *idgrid, const double *uvecs,
                            const int32_t *lens, int ndim, const double *vecs_s,
                            const double *ptp, uint32_t log_mask,
                            int exp_flag, const double *params, int B,
                            double *templ, double *outside, int32_t *cellinfo,
                            double *weights, void *stream);

/* ... and its derivative with respect to the physical parameters.  Inside a cell
 * GridInterp.__call__ (spec_inter.py:134-194) returns t = exp(sum_S w_S(p) L_S) with
 * polylinear weights w_S of the mapped parameters (LogParamMapper.forward,
 * read_grid.py:127-145), so  dt/dp_k = t * sum_S (dw_S/dp_k) L_S  -- a parameter in
 * log_mask carries the factor 1/(p_k ln 10); without exp_flag the factor t is absent.
 * templ  float64 [B, 1+ndim, ntp] out: row 0 the template (the bits of
 *        rvs_template_polylinear, as are outside / cellinfo / weights), row 1+k
 *        dt/dp_k per physical unit; the tangent rows are exactly 0 in the
 *        nearest-neighbour modes (cellinfo mode 1 and 2), where the evaluator is
 *        piecewise constant.  On a cell face the one-sided derivative of the cell
 *        the search returns.
 * Other arguments as rvs_template_polylinear. */
int rvs_template_polylinear_grad(const float *dats, int64_t ngrid, int ntp,
                                 const int64_t *idgrid, const double *uvecs,
                                 const int32_t *lens, int ndim,
                                 const double *vecs_s, const double *ptp,
                                 uint32_t log_mask, int exp_flag,
                                 const double *params, int B, double *templ,
                                 double *outside, int32_t *cellinfo,
                                 double *weights, void *stream);

/* ------------------------------------------------------------------------
 * A3 on an irregular grid: Delaunay evaluator, replaces spec_inter.TriInterp
 * (spec_inter.py:11-59) for `interpolation_type = 'triangulation'` libraries
 * (make_nd without --regulargrid): find_simplex (exhaustive, scipy's inside
 * test with eps = 100*DBL_EPSILON, lowest simplex id) + barycentric blend of
 * ndim+1 rows + exp, and the same blend of `extraflags` as outside flag
 * (+ the MAX_VAL guard of getCurTempl).  No containing simplex -> NaN template,
 * NaN outside flag.
 * dats       float64 [npts, ntp]      log-flux rows incl. the padded edge points
 * simplices  int32   [nsimplex, ndim+1]
 * transform  float64 [nsimplex, ndim+1, ndim]  scipy Delaunay.transform
 * extraflags float64 [npts]
 * simplex    int32   [B]   out (required): simplex id or 0x7fffffff
 * weights    float64 [B, ndim+1] out (nullable)
 * ---------------------------------------------------------------------- */
int rvs_template_tri(const double *dats, int ntp, const int32_t *simplices,
                     const double *transform, const double *extraflags,
                     int nsimplex, int ndim, uint32_t log_mask, int exp_flag,
                     const double *params, int B, double *templ, double *outside,
                     int32_t *simplex, double *weights, void *stream);

/* ... and its derivative with respect to the physical parameters.  Inside a simplex
 * TriInterp.__call__ (spec_inter.py:11-59) returns t = exp(sum_i b_i L_i) with the
 * barycentric coordinates b = T (q - r), b_ndim = 1 - sum_i b_i, of the mapped
 * parameters q (LogParamMapper.forward, read_grid.py:127-145).  b is affine in q, so
 * db_i/dp_k = T[i][k] s_k for i < ndim and db_ndim/dp_k = -sum_i T[i][k] s_k, with
 * s_k = 1/(p_k ln 10) for a parameter in log_mask and 1 otherwise, and
 * dt/dp_k = t * sum_i (db_i/dp_k) L_i; without exp_flag the factor t is absent.
 * templ  float64 [B, 1+ndim, ntp] out: row 0 the template (the bits of
 *        rvs_template_tri, as are outside / simplex / weights), row 1+k dt/dp_k per
 *        physical unit.  No containing simplex (a non-finite mapped parameter
 *        included): all 1+ndim rows NaN, NaN outside flag.  On a shared face the
 *        one-sided derivative of the simplex the search returns.
 * Other arguments as rvs_template_tri. */
int rvs_template_tri_grad(const double *dats, int ntp, const int32_t *simplices,
                          const double *transform, const double *extraflags,
                          int nsimplex, int ndim, uint32_t log_mask, int exp_flag,
                          const double *params, int B, double *templ,
                          double *outside, int32_t *simplex, double *weights,
                          void *stream);

/* The reverse step of the same evaluator (spec_inter.py:11-59 differentiated): ONE
 * adjoint row per job contracted with the tangent rows rvs_template_tri_grad would have
 * written (its rows 1 + k), which are not formed,
 *   gparams[b, k] = sum_n tbar[b, n] d templ[b, n] / d p_k        [B, ndim] float64
 * per physical unit of p_k, by the formulas above: per knot n the ndim sums
 * sum_i (db_i/dp_k) L_i[n], times tbar_n (times templ_n under exp_flag), summed over n.
 *   templ    float64 [B, ntp]  the value rows rvs_template_tri / _buckets wrote for params
 *   simplex  int32   [B]       the ids they wrote; the search is not repeated
 *   tbar     float64 [B, ntp]  the adjoint rows (rvs_objective_grad_from_template)
 * A row whose id is 0x7fffffff or negative (no containing simplex, a non-finite mapped
 * parameter; its templ row is NaN and is not read) has exact zeros.  float64 throughout;
 * one block per job, the threads' sums through a fixed tree, no atomics: two calls give
 * the same bits, a job has the same bits alone and inside any batch, and the result
 * scales exactly with tbar.  RVS_E_ARG before any launch for ndim outside 1..6,
 * ntp < 1, nsimplex < 1, B < 0 or a NULL array; B == 0 returns 0. */
int rvs_template_tri_vjp(const double *dats, int ntp, const int32_t *simplices,
                         const double *transform, int nsimplex, int ndim,
                         uint32_t log_mask, int exp_flag, const double *params,
                         int B, const int32_t *simplex, const double *templ,
                         const double *tbar, double *gparams, void *stream);

/* ... with find_simplex through a bucket grid instead of the exhaustive search (the
 * same answer: the lowest simplex id that passes scipy's inside test,
 * spec_inter.py:11-59 / Delaunay.find_simplex): cell c of a uniform grid over the
 * mapped parameter space lists, ascending, every simplex whose bounding box (grown by
 * 1e-9 of the grid's extent) overlaps it.  The cell of a mapped coordinate x in
 * dimension d is clamp(floor((x - lo[d]) * inv_w[d]), 0, n[d] - 1), cells in C order
 * over the dimensions.  List number ncell (behind the last cell) holds the simplices
 * whose boxes overlap too many cells to be entered in each: every query tests it as
 * well, the lower id of the two finds wins.  The struct is read on the host;
 * cell_start [ncell + 2] and cell_list [cell_start[ncell + 1]] are device arrays. */
typedef struct rvs_tri_buckets {
  const int32_t *cell_start, *cell_list;
  double lo[6], inv_w[6];
  int32_t n[6];
} rvs_tri_buckets;
int rvs_template_tri_buckets(const double *dats, int ntp, const int32_t *simplices,
                             const double *transform, const double *extraflags,
                             int nsimplex, int ndim, uint32_t log_mask,
                             int exp_flag, const rvs_tri_buckets *buckets,
                             const double *params, int B, double *templ,
                             double *outside, int32_t *simplex, double *weights,
                             void *stream);

/* ... and rvs_template_tri_grad (spec_inter.py:11-59 differentiated) behind the same
 * bucketed find_simplex: templ float64 [B, 1+ndim, ntp], every number that of
 * rvs_template_tri_grad.  Other arguments as rvs_template_tri_buckets. */
int rvs_template_tri_buckets_grad(const double *dats, int ntp,
                                  const int32_t *simplices, const double *transform,
                                  const double *extraflags, int nsimplex, int ndim,
                                  uint32_t log_mask, int exp_flag,
                                  const rvs_tri_buckets *buckets,
                                  const double *params, int B, double *templ,
                                  double *outside, int32_t *simplex, double *weights,
                                  void *stream);

/* ------------------------------------------------------------------------
 * A6  rotational broadening; replaces spec_fit.convolve_vsini /
 *     compute_vsini_kernel (spec_fit.py:495-682).  vsini[b] <= 0, NaN or
 *     R < 1e-9 copies the row (as does a non finite `outside[b]`, nullable,
 *     spec_fit.py:398-404).  lnstep = log(lam[1]/lam[0]) of the log-uniform
 *     template grid.  In place (out == templ) is NOT allowed.
 * ---------------------------------------------------------------------- */
int rvs_vsini_convolve(const double *templ, const double *vsini,
                       const double *outside, double lnstep, double eps,
                       int ntp, int B, double *out, void *stream);

/* ... with the derivative of the taps (spec_fit.py:495-682 differentiated): job b
 *     owns the R rows templ[b, 0..R-1] (a template and its parameter tangents), one
 *     vsini[b] and one outside[b]; out is [B, R + 1, ntp].  Rows r < R are
 *     templ[b, r] (*) w(vsini[b]), the bits rvs_vsini_convolve writes for those rows;
 *     row R is templ[b, 0] (*) dw/dvsini per km/s, same 'same' zero padding and
 *     summation order.  With Rv = vsini / (c lnstep) the un-normalised taps are
 *     W_k = int Lambda(k - Rv x) K(x) dx; the boundary terms of Leibniz's rule cancel
 *     (Lambda is continuous, K(+-1) = 0), so dW_k/dRv = -int_left x K + int_right x K
 *     over the value's clipped limits, and with S = W_0 + 2 sum W_k the normalised
 *     taps have dw/dRv = (W' - w S') / S.  w is C^1 across integer Rv.  The VALUE has
 *     a kink at vsini = 0+ (W_0 = 1 - Rv E|x| for small Rv): in the copy cases
 *     (vsini <= 0, NaN, Rv < 1e-9, non finite outside[b], more than 2048 one-sided
 *     taps) rows r < R are copied and row R is exactly 0 -- the derivative of the
 *     clamped function an optimiser sees, not the one-sided limit.
 *     Sums folded in a fixed order, no atomics: repeated calls agree to the bit.
 *     RVS_E_ARG for R < 1, B < 1, ntp < 1, out == templ, lnstep <= 0. */
int rvs_vsini_convolve_grad(const double *templ, const double *vsini,
                            const double *outside, double lnstep, double eps,
                            int ntp, int R, int B, double *out, void *stream);

/* ------------------------------------------------------------------------
 * A7  natural cubic spline through (knots, ys[b]); replaces `construct`
 *     (src/spliner.c:7-60).  form 0: coef[b, i, 0..3] = A,B,C,D of interval i
 *     exactly as the reference (i < ntp-1; row ntp-1 is zero padding -- in
 *     form 1 it holds {y_last, 0, 0, 0}; h is implied by knots).  form 1: the SAME cubic in powers of dl = x - x_i,
 *     {y_i, b, c, d} with S = y + dl (b + dl (c + dl d)) -- 3 fma per evaluation,
 *     the form the fused chi^2 kernels consume.  form | 2: the caller asserts
 *     that neighbouring knot spacings agree to ~1 % (uniform or log-uniform
 *     grids, what `evaler` requires anyway): both Thomas recurrences then
 *     contract by ~0.27 per row and are evaluated in independent 32-row-overlap
 *     windows (error < 1e-18 relative) instead of by exact chunk carries; this
 *     needs `factors` from rvs_spline_factors (pivots, h, 1/h of the knot grid,
 *     computed once per template grid: 5 arrays of ntp doubles, followed -- for ntp <=
 *     8192 -- by 1/h_u, 1/h_{u+1}, g_u, e_u (records of four) and c_u (pairs) once
 *     more in the order the fused objective kernel's 512 threads own their rows,
 *     5 x 8192 doubles;
 *     rvs_spline_factors_len(ntp) in all); NULL otherwise.
 * ---------------------------------------------------------------------- */
int64_t rvs_spline_factors_len(int ntp);   /* doubles `factors` must hold */
int rvs_spline_factors(const double *knots, int ntp, double *factors,
                       void *stream);
int rvs_spline_construct(const double *knots, const double *ys, int ntp, int B,
                         int form, const double *factors, double *coef,
                         void *stream);

/* A7  replaces `evaler` (src/spliner.c:71-108) for B splines sharing the
 * knots: ret[b, i] = S_b(evalx[b, i]); pos (nullable) receives the integer
 * interval index (int)((log x - log x0)/logstep) computed exactly as the
 * reference does; status[b] gets RVS_ST_SPLINE_RANGE / _GRID. */
int rvs_spline_eval(const double *knots, const double *coef, int ntp,
                    int log_step, const double *evalx, int neval, int B,
                    double *ret, int32_t *pos, int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * A7-eval + A10 + A11 fused: Doppler resample of a spline template onto the
 * observed pixels and continuum-marginalised -2 log L on a velocity grid;
 * replaces the vel loop of spec_fit.find_best over spec_fit.get_chisq
 * (spec_fit.py:797-989, 1060-1071) for ONE spectral arm.
 *
 * Two calls: rvs_chisq_prepare once per (arm, batch of spectra) builds the
 * velocity-independent per-pixel terms into `work` (rvs_chisq_work_size
 * doubles); rvs_chisq_grid may then be called many times (first guess,
 * refinement rounds, optimiser steps) on the same `work`.
 *
 * lam     [npix]        observed wavelengths of the arm (shared by the batch)
 * polysT  [npix, npoly] continuum basis, pixel-major (get_poly_basis^T)
 * spec, espec [S, npix]
 * knots   [ntp], coef [Tn, ntp, 4]   from rvs_spline_construct(form = 1)
 * knots_host3  HOST pointer to the first three knots: the uniformity test of
 *          spliner.c:84-96 is done on the host; returns -3 where evaler
 *          returns -2
 * job_spec, job_templ int32 [J] (nullable = identity): job j fits spectrum
 *          job_spec[j] with template job_templ[j]
 * vels    float64, job j uses vels + j*vel_stride (vel_stride 0 = shared grid)
 * espec_sys  systematic error added in quadrature (spec_fit.py:933-940)
 * penalty [J] (nullable) added to every velocity of job j (outside*badchi,
 *          spec_fit.py:895-896); a non finite penalty means "template not
 *          usable": the arm contributes 1000*badchi (spec_fit.py:888-893).
 * beta    out = beta*out + value  (0 first arm, 1 following arms)
 * pack_min_jobs  the Nv % 64 left-over velocities of a job (16 of the 400-point
 *          grid) share a wave with those of other jobs when J >= this
 *          (0 = library default 2000, 1 = always, < 0 = never); where a
 *          velocity is computed does not change its value.  The packed launch
 *          runs on a library-owned side stream (one per host thread and
 *          device), forked from and joined to `stream` inside the call: to the
 *          caller the call is ordered on `stream` like any other.
 * out     [J, Nv];   status int32 [J] OR-ed (caller zeroes it)
 * Device memory of the library's own: where rvs_chisq_grid_pair_cols(npoly) > 0,
 * on one wavelength grid
 * (this call, rvs_chisq_grid_g with G = 1, rvs_chisq_grid_tab) the kernels read
 * 128-byte rows {basis values, pair products of the last columns} that a small
 * kernel at the head of the call builds from polysT into a buffer kept per
 * (device, stream): npix rounded up to 1024, times 128 bytes; allocated on a
 * stream's first call and when an arm is longer than any before it on that
 * stream; the buffers of the 64 streams used last are kept (RVS_E_LAUNCH when
 * an allocation fails).  A call queues its row kernel and its grid kernels under
 * a lock of the library's, so host threads may share a stream as before.
 * ---------------------------------------------------------------------- */
int64_t rvs_chisq_work_size(int npix, int S);
int rvs_chisq_prepare(const double *lam, const double *spec,
                      const double *espec, int npix, int S,
                      const double *knots_host3, int log_step, double espec_sys,
                      double *work, void *stream);
int rvs_chisq_grid(const double *lam, const double *polysT, const double *work,
                   int npix, int npoly, int S, const double *knots,
                   const double *coef, int ntp, int Tn, int log_step,
                   const int32_t *job_spec, const int32_t *job_templ, int J,
                   const double *vels, int64_t vel_stride, int Nv,
                   const double *penalty, double badchi, double beta,
                   int pack_min_jobs, double *out, int32_t *status,
                   void *stream);

/* Grid sets (ABI 7): the S spectra of an arm observed on G different wavelength
 * grids (SDSS-style objects: every spectrum has its own `lam`, spec_fit.py:70-145,
 * tests/test_sdss.py).  lam [G, npix]: grid g in row g, a grid with fewer than
 * npix pixels padded by repeating its last wavelength; grid_id int32 [S]: the grid
 * of spectrum s; on the padding the spectra carry espec = +inf (weight 0, no term
 * in sum log e -- read as the marker ONLY when G > 1: on a single grid an infinite
 * error is data and gives the reference's log(inf), a non-finite likelihood the
 * status word reports) and the basis rows are 0; polysT of grid g starts at
 * polysT + g * polys_stride.  work: rvs_chisq_work_size_g(npix, S, G) doubles from
 * rvs_chisq_prepare_g.  G = 1 (grid_id NULL) is the shared-grid call.  With G > 1
 * the left-over velocities of a job are not packed with those of other jobs.
 * pen_scale [S] or NULL: per-spectrum factor on badchi (see rvs_point_arm). */
int64_t rvs_chisq_work_size_g(int npix, int S, int G);
int rvs_chisq_prepare_g(const double *lam, const double *spec,
                        const double *espec, int npix, int S, int G,
                        const double *knots_host3, int log_step, double espec_sys,
                        double *work, void *stream);
int rvs_chisq_grid_g(const double *lam, const double *polysT, const double *work,
                     int npix, int npoly, int S, const int32_t *grid_id, int G,
                     int64_t polys_stride, const double *knots,
                     const double *coef, int ntp, int Tn, int log_step,
                     const int32_t *job_spec, const int32_t *job_templ, int J,
                     const double *vels, int64_t vel_stride, int Nv,
                     const double *penalty, double badchi, double beta,
                     int pack_min_jobs, const double *pen_scale, double *out,
                     int32_t *status, void *stream);

/* rvs_chisq_grid_g with a node table.  When many jobs point at few templates
 * (one per CCF node) and share one velocity grid and one wavelength grid, the
 * resampled template of a (node, velocity, pixel) is the same number for every
 * job of the node: it is evaluated once into `tab` and the full waves (the
 * Nv / 64 blocks of 64 velocities of each job) stream it instead of evaluating
 * the spline; the Nv % 64 left-over velocities go through the packed launch.
 * Every value is the one rvs_chisq_grid_g gives, bit for bit.
 * order [J]          the call's jobs sorted by job_templ (a stable sort)
 * node_start [Tn+1]  first place of each template in `order` (prefix counts,
 *                    node_start[Tn] = J)
 * call_start [Tn+1], J_call  the same counts over ALL jobs that will read this
 *                    table (a caller that feeds its jobs in several calls passes
 *                    the whole list's counts to each; otherwise node_start, J):
 *                    templates no job uses are not resampled
 * min_jobs_per_node  the path is taken when J_call >= this * Tn (0 = library
 *                    default, 1 = whatever J_call is, < 0 = never)
 * tab, tab_size      rvs_chisq_grid_tab_work_size(npix, Tn, Nv, J_call,
 *                    min_jobs_per_node, pack_min_jobs) doubles
 * tab_state          0: the call fills the table first; 1: an earlier call with
 *                    the same arm, templates, velocities and call_start has
 *                    filled it
 * took               HOST int32 (nullable): 1 if the table path ran, else 0
 * pack_min_jobs      on the table path the Nv % 64 left-over velocities are ALWAYS
 *                    packed (a positive threshold is not looked at); < 0 (never
 *                    pack) or more than 50 left-over velocities, which
 *                    rvs_chisq_grid_g gives a ragged wave, decline the table
 * The path is taken only with job_templ given, vel_stride == 0, G == 1,
 * Nv >= 64, left-over velocities that can be packed, a table of at most 1 GiB
 * that fits tab_size, enough jobs per node and option "cg_tab" on; otherwise the
 * call IS rvs_chisq_grid_g (tab untouched).
 * rvs_chisq_grid_tab_work_size returns 0 where the size, the job count or the
 * option already decide against the table: the caller then needs no buffer. */
int64_t rvs_chisq_grid_tab_work_size(int npix, int Tn, int Nv, int64_t J_call,
                                     int min_jobs_per_node, int pack_min_jobs);
/* How many of the last columns of the packed normal matrix the velocity-grid
 * kernels of `npoly` functions accumulate from pair products P_i P_j of the row
 * (one wavelength grid; 0 = none: the arithmetic of a grid set; tests). */
int rvs_chisq_grid_pair_cols(int npoly);
int rvs_chisq_grid_tab(const double *lam, const double *polysT, const double *work,
                       int npix, int npoly, int S, const int32_t *grid_id, int G,
                       int64_t polys_stride, const double *knots,
                       const double *coef, int ntp, int Tn, int log_step,
                       const int32_t *job_spec, const int32_t *job_templ, int J,
                       const double *vels, int64_t vel_stride, int Nv,
                       const double *penalty, double badchi, double beta,
                       int pack_min_jobs, const double *pen_scale, double *out,
                       int32_t *status, const int32_t *order,
                       const int32_t *node_start, const int32_t *call_start,
                       int64_t J_call, int min_jobs_per_node, double *tab,
                       int64_t tab_size, int tab_state, int32_t *took,
                       void *stream);

/* A9 the same with a banded resolution matrix applied to the resampled
 * template before the fit: replaces convolve_resol / ResolMatrix
 * (spec_fit.py:54-67, 474-492) as used by get_chisq (:920-929).
 * taps [S or 1, npix, nd] row-major: taps[s, k, d] = R_s[k, k - (nd-1)/2 + d]
 * (0 outside the matrix), nd odd <= 33; taps_stride = npix*nd, or 0 when every
 * spectrum shares one matrix (the `resol_params` case).
 * status [J] as rvs_chisq_grid: RVS_ST_SPLINE_RANGE (first or last shifted pixel
 * outside the knots; those entries are NaN, with RVS_ST_NONFINITE),
 * RVS_ST_CHOL_FALLBACK (a pivot not positive) and RVS_ST_ILLCOND (pivots spanning
 * > 1e9: a long stretch of weightless pixels -- the band does not change that);
 * the caller re-evaluates jobs with either of the last two by rvs_chisq_point. */
int rvs_chisq_grid_resol(const double *lam, const double *polysT,
                         const double *work, int npix, int npoly, int S,
                         const double *knots, const double *coef, int ntp,
                         int Tn, int log_step, const double *taps, int nd,
                         int64_t taps_stride, const int32_t *job_spec,
                         const int32_t *job_templ, int J, const double *vels,
                         int64_t vel_stride, int Nv, const double *penalty,
                         double badchi, double beta, double *out,
                         int32_t *status, void *stream);
/* ... for spectra of an arm on G wavelength grids of their own (grid sets, above:
 * lam [G, npix], work from rvs_chisq_prepare_g, polysT of grid g at polysT + g *
 * polys_stride), each with its own resolution matrix (spec_fit.py:922-929 accepts
 * any SpecData.resolution; tests/test_sdss.py): taps [S, npix, nd] with npix the
 * longest grid -- the rows behind a spectrum's own pixels, and every tap that
 * refers to a pixel behind them, are zero.  pen_scale as in rvs_chisq_grid_g.
 * G = 1 (grid_id NULL) is rvs_chisq_grid_resol. */
int rvs_chisq_grid_resol_g(const double *lam, const double *polysT,
                           const double *work, int npix, int npoly, int S,
                           const int32_t *grid_id, int G, int64_t polys_stride,
                           const double *knots, const double *coef, int ntp,
                           int Tn, int log_step, const double *taps, int nd,
                           int64_t taps_stride, const int32_t *job_spec,
                           const int32_t *job_templ, int J, const double *vels,
                           int64_t vel_stride, int Nv, const double *penalty,
                           double badchi, double beta, const double *pen_scale,
                           double *out, int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * get_chisq(full_output=True) for one velocity per job and one arm
 * (spec_fit.py:941-961), and get_chisq_continuum (spec_fit.py:739-783) when
 * unit_template == 1 (template == 1, knots/coef ignored); unit_template == 2:
 * get_chisq0 itself (spec_fit.py:306-354) -- the template is given ON THE PIXELS,
 * row job_templ[j] of `coef` read as [Tn, npix] doubles (knots, ntp, vel, cform
 * ignored; espec of ones = "already divided by the uncertainty").  cform = the form of
 * the spline records (see rvs_spline_construct).  fast_interp: the template
 * value is the nearest knot at or above x instead of the spline
 * (spec_fit.py:913-918; needs cform = 1).  taps (nullable): resolution
 * matrix rows as in rvs_chisq_grid_resol, applied to the template (or to 1).
 * coeffs [J, npoly], model/raw_model [J, npix] (nullable), chisq [J] (-2logL
 * of the arm), true_chisq [J] over pixels with badmask==0, ngood int32 [J].
 * ---------------------------------------------------------------------- */
int rvs_chisq_full(const double *lam, const double *polysT, const double *spec,
                   const double *espec, const uint8_t *badmask, int npix,
                   int npoly, int S, const double *knots, const double *coef,
                   int ntp, int Tn, int log_step, int cform, int unit_template,
                   const int32_t *job_spec, const int32_t *job_templ, int J,
                   const double *vel, double espec_sys, int fast_interp,
                   const double *taps, int nd, int64_t taps_stride,
                   double *chisq, double *coeffs,
                   double *model, double *raw_model, double *true_chisq,
                   int32_t *ngood, int32_t *status, void *stream);
/* ... on grid sets (see rvs_chisq_grid_g): lam [G, npix], polysT per grid; the
 * padding of a short grid does not count in ngood / true_chisq, model is 0 there. */
int rvs_chisq_full_g(const double *lam, const double *polysT, const double *spec,
                     const double *espec, const uint8_t *badmask, int npix,
                     int npoly, int S, const double *knots, const double *coef,
                     int ntp, int Tn, int log_step, int cform, int unit_template,
                     const int32_t *job_spec, const int32_t *job_templ, int J,
                     const double *vel, double espec_sys, int fast_interp,
                     const double *taps, int nd, int64_t taps_stride,
                     double *chisq, double *coeffs, double *model,
                     double *raw_model, double *true_chisq, int32_t *ngood,
                     int32_t *status, const int32_t *grid_id, int G,
                     int64_t polys_stride, void *stream);

/* ------------------------------------------------------------------------
 * A13  get_chisq_continuum (spec_fit.py:739-783) for a whole batch of one arm:
 * continuum-only fit (template == 1), true chi^2 over pixels with badmask == 0
 * and their count.  One wave per spectrum, lanes = pixels; a Cholesky failure (numerically
 * singular basis) is flagged and gives NaN -- rvs_chisq_full(unit_template=1)
 * is the slower entry point with the eigen (SVD) fallback.
 * polysT [npix, npoly]; spec, espec [S, npix]; badmask uint8 [S, npix] (nullable)
 * unit_templ [S, npix] (nullable): R_s @ 1 when the spectra carry a resolution
 * matrix (spec_fit.py:765-767)
 * work: unused since round 2 (nullable; rvs_chisq_continuum_work_size returns 8)
 * chisq [S] (-2 log L, nullable), true_chisq [S], ngood int32 [S]
 * ---------------------------------------------------------------------- */
int64_t rvs_chisq_continuum_work_size(int npoly, int S);
int rvs_chisq_continuum(const double *polysT, const double *spec,
                        const double *espec, const uint8_t *badmask,
                        const double *unit_templ, int npix, int npoly, int S,
                        void *work, double *chisq,
                        double *true_chisq, int32_t *ngood, int32_t *status,
                        void *stream);
int rvs_chisq_continuum_g(const double *polysT, const double *spec,
                          const double *espec, const uint8_t *badmask,
                          const double *unit_templ, int npix, int npoly, int S,
                          void *work, double *chisq, double *true_chisq,
                          int32_t *ngood, int32_t *status,
                          const int32_t *grid_id, int G, int64_t polys_stride,
                          void *stream);

/* ------------------------------------------------------------------------
 * A11 at one velocity per job: the objective of the optimiser stage,
 * chisq_func0 (vel_fit.py:205-226) = get_chisq (spec_fit.py:797-989) for J
 * (spectrum, template, velocity) triples, ALL arms of the spectrum in one
 * launch.  One 256-thread block per (job, arm), threads = pixels; the residual
 * norm ||D - a.ST||^2 is formed explicitly (spec_fit.py:249) so the value can
 * be finite-differenced (Hessian, vel_fit.py:699-725).
 * Per arm (plain struct of device pointers, passed by value from the host):
 *   lam [npix], polysT [npix, npoly] (plain get_basis, NOT orthonormalised),
 *   spec, espec [S, npix], work = the rvs_chisq_prepare buffer of the arm,
 *   knots [ntp], coef [Tn, ntp, 4] form-1 records, penalty [J] (nullable;
 *   a NaN/inf entry means "template unusable": + 1000*badchi, arm skipped).
 * scratch: rvs_chisq_point_work_size(J, narm) bytes.
 * out[j] = sum over arms of (chisq + penalty).
 * ---------------------------------------------------------------------- */
#define RVS_MAX_ARMS 4
typedef struct rvs_point_arm {
  const double *lam, *polysT, *spec, *espec, *work, *knots, *coef, *penalty;
  const double *taps;   /* A9 resolution matrix rows [S or 1, npix, nd] or NULL */
  int64_t taps_stride;  /* npix*nd, or 0 when all spectra share one matrix */
  double espec_sys;     /* systematic error in quadrature (spec_fit.py:933-940);
                           `work` must have been prepared with the same value */
  int32_t npix, S, ntp, log_step, nd;
  int32_t fast_interp;  /* nearest-knot template instead of the spline (:913-918) */
  /* wavelength grids of the arm (ABI 7): G <= 1 -- one grid, lam [npix], polysT
   * [npix, npoly], work from rvs_chisq_prepare; G > 1 -- spectrum s is observed on
   * grid grid_id[s]: lam [G, npix], polysT of grid g at polysT + g*polys_stride,
   * work from rvs_chisq_prepare_g (a grid shorter than npix is padded: lam repeats
   * its last value, espec = +inf, basis rows 0).  No resolution matrix with G > 1. */
  const int32_t *grid_id;
  int64_t polys_stride;
  int32_t G, reserved_;
  /* per-spectrum factor on `badchi` [S] or NULL (read from arm 0): badchi is
   * 10 x the pixel count of the SPECTRUM (spec_fit.py:863), which differs between
   * the spectra of a grid set -- the scalar argument carries the largest, this the
   * ratio */
  const double *pen_scale;
} rvs_point_arm;
int64_t rvs_chisq_point_work_size(int J, int narm);
int rvs_chisq_point(const rvs_point_arm *arms, int narm, int npoly,
                    const int32_t *job_spec, const int32_t *job_templ, int J,
                    const double *vel, double badchi, void *scratch,
                    double *out, int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * ... with its gradient: value and derivative of get_chisq (spec_fit.py:797-989;
 * the marginalised chi^2 of get_chisq0, spec_fit.py:264-298) with respect to the
 * job's velocity and the ntan parameters its template was differentiated by.
 * One 256-thread block per (job, arm).
 *   coef of every arm: [Tn, 1+ntan, ntp, 4] form-1 records -- row 0 the template,
 *   row 1+k its tangent dt/dp_k (rvs_template_polylinear_grad through
 *   rvs_vsini_convolve and rvs_spline_construct, which are linear in the rows; a
 *   last row from rvs_vsini_convolve_grad makes vsini one more parameter).
 *   The velocity tangent is S'(x) dx/dvel from the template's own record
 *   (evalRV, spec_fit.py:403-405: x = lam sqrt((1-b)/(1+b)), b = vel/c).
 * With ST = polys*m/e, A = ST ST^T, c = A^-1 ST D, r = D/e - c.ST the value is
 * log det A + 2 sum log e + |r|^2, and for a tangent m' of the model
 *   d chi^2 = sum_pix m'/e * ( 2 (m/e) polys^T A^-1 polys  -  2 r (c.polys) ),
 * the first term being tr(A^-1 A'), the second c^T A' c - 2 c.v' of the normal
 * equations with the residual formed explicitly.  A is factored once per block;
 * every sum is folded in a fixed order (no atomics): repeated calls agree to the bit.
 * polysT may be ANY basis of the continuum space; basis_const [narm] (host, or NULL)
 * is added to the arm's value: 2 log|det R| when polysT holds the orthonormalised
 * basis Q of polys^T = Q R (the gradient does not depend on the basis).
 * grad [J, 1+ntan] out: {d/dvel, d/dp_0 ...} summed over the arms.  The penalty
 * terms enter the value as in rvs_chisq_point and are not differentiated; an arm
 * with a non finite penalty adds 1000*badchi and no gradient.  Where the
 * factorisation fails: RVS_ST_CHOL_FALLBACK | RVS_ST_NONFINITE, value and gradient NaN.
 * Restrictions (RVS_E_ARG otherwise): npoly <= 16, G <= 1, taps == NULL,
 * fast_interp == 0, 0 <= ntan <= 6.
 * scratch: rvs_chisq_point_grad_work_size(J, narm, ntan) bytes.
 * ---------------------------------------------------------------------- */
int64_t rvs_chisq_point_grad_work_size(int J, int narm, int ntan);
int rvs_chisq_point_grad(const rvs_point_arm *arms, int narm, int npoly, int ntan,
                         const int32_t *job_spec, const int32_t *job_templ, int J,
                         const double *vel, double badchi,
                         const double *basis_const, void *scratch, double *out,
                         double *grad, int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * ... and with the Fisher matrix of the fit: the expected information of the Gaussian
 * likelihood in (velocity, the ntan parameters), marginalised over the continuum
 * coefficients -- the Gauss-Newton part of the Hessian of 0.5 * (-2 log L), the
 * quantity vel_fit.hess_func differences, so that its inverse is a covariance.
 * Arguments, restrictions, value, gradient and status bits are those of
 * rvs_chisq_point_grad (the same two passes in the same block: out and grad carry the
 * same bits); a third pass forms, per arm, with s = c.polys the fitted continuum,
 * J_ki = s_k m'_ki / e_k the whitened model's Jacobian and y = L^-1 polys (A = L L^T),
 *   F_il = sum_k J_ki J_kl - sum_p B_pi B_pl,   B_pi = sum_k y_p(k) (m_k/e_k) J_ki,
 * the Schur complement of the joint Fisher matrix of (parameters, continuum).  Tangent
 * 0 is the velocity tangent, tangent i >= 1 row i of coef.  It is positive
 * semi-definite up to rounding and exactly symmetric (each entry is formed once and
 * written to both halves); every sum is folded in a fixed order (no atomics).  The
 * penalty terms and log det A are not part of it.
 * fisher [J, 1+ntan, 1+ntan] out: summed over the arms in arm order; an arm with a non
 * finite penalty adds nothing; where an arm's value is NaN its matrix is NaN.
 * fisher == NULL: RVS_E_ARG.
 * scratch: rvs_chisq_point_fisher_work_size(J, narm, ntan) bytes =
 * narm * J * ((2 + ntan + (1 + ntan)^2) * 8 + 4); 0 for what is refused (J < 1,
 * narm < 1, ntan outside 0..6).
 * ---------------------------------------------------------------------- */
int64_t rvs_chisq_point_fisher_work_size(int J, int narm, int ntan);
int rvs_chisq_point_fisher(const rvs_point_arm *arms, int narm, int npoly, int ntan,
                           const int32_t *job_spec, const int32_t *job_templ, int J,
                           const double *vel, double badchi,
                           const double *basis_const, void *scratch, double *out,
                           double *grad, double *fisher, int32_t *status,
                           void *stream);

/* ------------------------------------------------------------------------
 * ... both under banded resolution matrices: the arguments, value, gradient, Fisher
 * matrix, status bits and work sizes of rvs_chisq_point_grad / rvs_chisq_point_fisher,
 * with arms that may carry taps / taps_stride / nd as in rvs_chisq_point (arms with and
 * without a matrix may be mixed).  The model row of such an arm is m = R raw,
 *   m_k = sum_d taps[s][k][d] raw[k - (nd-1)/2 + d]   (d ascending, pixels outside
 * the arm skipped), and every tangent row is R applied to the raw tangent row -- the
 * raw velocity tangent of pixel q being S'(x_q) lam_q df/dvel, with lam of q --; the
 * rest of rvs_chisq_point_grad's mathematics is unchanged.  The block walks the pixels
 * in tiles of 256, the raw rows of a tile and its halo staged in LDS:
 *   RVS_GRAD_RESOL_LDS(ntan, nd) = (2 + ntan) * (255 + nd) * 8 bytes, any npix,
 * for the widest matrix of the call, at most RVS_GRAD_RESOL_LDS_MAX (nd <= 641 at
 * ntan = 6, nd <= 3329 at ntan = 0).  With nd = 1 and taps of 1 the results are the
 * bits of the pair above, and so is a call in which no arm has taps (it runs their
 * kernels).  RVS_E_ARG, before any launch: what the pair above refuses other than
 * taps (npoly outside 1..16, ntan outside 0..6, G > 1, fast_interp), nd even or < 1,
 * RVS_GRAD_RESOL_LDS(ntan, nd) > RVS_GRAD_RESOL_LDS_MAX.
 * ---------------------------------------------------------------------- */
#define RVS_GRAD_RESOL_LDS_MAX (56 * 1024)
#define RVS_GRAD_RESOL_LDS(ntan, nd) ((2 + (ntan)) * (255 + (int64_t)(nd)) * 8)
int64_t rvs_chisq_point_grad_resol_work_size(int J, int narm, int ntan);
int rvs_chisq_point_grad_resol(const rvs_point_arm *arms, int narm, int npoly,
                               int ntan, const int32_t *job_spec,
                               const int32_t *job_templ, int J, const double *vel,
                               double badchi, const double *basis_const,
                               void *scratch, double *out, double *grad,
                               int32_t *status, void *stream);
int64_t rvs_chisq_point_fisher_resol_work_size(int J, int narm, int ntan);
int rvs_chisq_point_fisher_resol(const rvs_point_arm *arms, int narm, int npoly,
                                 int ntan, const int32_t *job_spec,
                                 const int32_t *job_templ, int J, const double *vel,
                                 double badchi, const double *basis_const,
                                 void *scratch, double *out, double *grad,
                                 double *fisher, int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * The same objective as ONE kernel per evaluation for regular-grid libraries:
 * polylinear gather + exp (A3/A5), rotational FIR (A6), windowed natural-spline
 * solve (A7) and the chi^2 of rvs_chisq_point (A10/A11), one 512-thread block
 * per (job, arm) with the whole template in LDS (3*ntp doubles <= 154 KB); no
 * spline record goes to HBM.  Replaces, for the optimiser's ~850 calls per
 * spectrum, the chain rvs_template_polylinear -> rvs_vsini_convolve ->
 * rvs_spline_construct -> rvs_chisq_point (same arithmetic per phase).
 * Per arm: `pt` as in rvs_chisq_point (coef, penalty unused; no fast_interp;
 * taps / taps_stride / nd as there: the band runs over the pixels' spline values
 * in LDS, the sum over d ascending as rvs_chisq_point forms it), the polylinear library as in rvs_template_polylinear, the
 * rvs_spline_factors of the template grid, ln-step of the grid for the
 * rotational kernel.  params [J, ndim], vsini [J] (nullable = no rotation),
 * vel [J]; scratch: rvs_objective_work_size(J, narm) bytes;
 * out[j] = sum over arms of chisq + outside*badchi (NaN outside: + 1000*badchi).
 * outside_penalty: bit 0 = add the outside*badchi penalty; bit 1
 * (RVS_OBJ_STATUS_STORE) = status[j] is overwritten instead of OR-ed into (the
 * optimiser's per-call scratch needs no clearing launch).
 * RVS_E_ARG: ntp < 32 or > rvs_objective_max_ntp(npoly); and, from npoly = 11 on
 * (the waves' partial sums live in the template's LDS), an arm with
 * 2*npix > ntp or 2*ntp < 8*(npoly*(npoly+3)/2 + 1) -- use the chain of
 * stand-alone kernels there.  With a resolution matrix on any arm: every arm must
 * pass rvs_objective_resol_ok(npoly, npix, ntp, nd) (an arm without taps among
 * them counts as nd = 1) -- nd odd and <= 33, 2*npix <= ntp and
 * npix + nd - 1 <= ntp (spline values, their zero margins and the sigma-scaled
 * pair live in the template's LDS), and from npoly = 11 on
 * ntp >= 8*(npoly*(npoly+3)/2 + 1); else RVS_E_ARG and the chain as before (the
 * 377 diagonals of an R = 50 matrix, tests/test_sdss.py).
 * ---------------------------------------------------------------------- */
#define RVS_OBJ_STATUS_STORE 2
/* bit 2: the per-arm results stay in `scratch` ([narm, J] chi^2, [narm, J] outside,
 * [narm, J] int32 status), out / status are not written: rvs_nm_run folds the sum
 * over the arms into its own bookkeeping kernels */
#define RVS_OBJ_NO_SUM 4
typedef struct rvs_objective_arm {
  rvs_point_arm pt;
  const float *dats;
  const int64_t *idgrid;
  const double *uvecs, *vecs_s, *factors;
  int64_t ngrid;
  double lnstep;
  double ptp[6];
  int32_t lens[6];
  int32_t ntp, ndim;
  uint32_t log_mask;
  int32_t exp_flag;
} rvs_objective_arm;
int rvs_objective_max_ntp(int npoly); /* largest template grid that fits LDS */
/* 1: the objective kernel applies a resolution matrix of nd diagonals on an arm of
 * this geometry (host arithmetic only: no device is touched) */
int rvs_objective_resol_ok(int npoly, int npix, int ntp, int nd);
int64_t rvs_objective_work_size(int J, int narm);
int rvs_objective_fused(const rvs_objective_arm *arms, int narm, int npoly,
                        const double *params, const double *vsini,
                        const int32_t *job_spec, int J, const double *vel,
                        double badchi, int outside_penalty, void *scratch,
                        double *out, int32_t *status, void *stream);

/* The same objective for evaluators that are not a grid gather (the MLP of
 * rvs_template_nn): the unbroadened template of job j on arm a is row j of
 * templ[a] ([J, ntp] float64, device), its outside flag outside[a][j]
 * (SpecInterpolator.outsideFlag, spec_inter.py:257-272; the MAX_VAL guard of
 * getCurTempl, spec_fit.py:392-397, is applied here).  `templ` / `outside` are
 * HOST arrays of narm device pointers.  Of rvs_objective_arm only pt, factors,
 * lnstep and ntp are read.  Rotational broadening, spline solve and chi^2 are
 * the code of rvs_objective_fused: equal arithmetic. */
int rvs_objective_from_template(const rvs_objective_arm *arms, int narm,
                                int npoly, const double *const *templ,
                                const double *const *outside,
                                const double *vsini, const int32_t *job_spec,
                                int J, const double *vel, double badchi,
                                int outside_penalty, void *scratch, double *out,
                                int32_t *status, void *stream);

/* Both with a job count that lives on the device (ABI 8): only the first
 * min(J, njobs_dev[0]) jobs are evaluated, out[] / status[] of the others are left
 * as they are; J still sizes the launch, the scratch and every array.  The
 * lock-step optimiser (rvs_nm_run) knows on the host only an upper bound of the
 * simplices that are still running and of those that need the second point of a
 * round; the exact counts are its device counters.  NULL = all J. */
int rvs_objective_fused_n(const rvs_objective_arm *arms, int narm, int npoly,
                          const double *params, const double *vsini,
                          const int32_t *job_spec, int J,
                          const int32_t *njobs_dev, const double *vel,
                          double badchi, int outside_penalty, void *scratch,
                          double *out, int32_t *status, void *stream);
int rvs_objective_from_template_n(const rvs_objective_arm *arms, int narm,
                                  int npoly, const double *const *templ,
                                  const double *const *outside,
                                  const double *vsini, const int32_t *job_spec,
                                  int J, const int32_t *njobs_dev,
                                  const double *vel, double badchi,
                                  int outside_penalty, void *scratch, double *out,
                                  int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * The objective of rvs_objective_fused WITH its gradient, as one kernel per (job,
 * arm), by the adjoint method: the template path (gather, rotational FIR, natural
 * spline, resampling) is linear in the template row, so one adjoint row -- whatever
 * ntan is -- is carried from the pixels back to the knots in the three LDS buffers the
 * value uses, and contracted there with the tangents d t / d p_d formed per knot from
 * the vertex rows (as rvs_template_polylinear_grad forms them) and, with vsini fitted,
 * with the tap derivatives of rvs_vsini_convolve_grad.  No template row, spline record
 * or adjoint row goes to HBM; no floating point atomics: repeated calls and permuted
 * job lists agree to the bit.  Replaces the chain rvs_template_polylinear_grad ->
 * rvs_vsini_convolve(_grad) -> rvs_spline_construct -> rvs_chisq_point_grad.
 * Arms as for rvs_objective_fused; pt.polysT may be ANY basis of the continuum space
 * with basis_const [narm] (host, or NULL) added to the arm's value, as for
 * rvs_chisq_point_grad.  ntan = ndim, or ndim + 1 with vsini fitted (vsini != NULL).
 *   out [J]             sum over the arms of chisq + outside*badchi (an arm whose
 *                       outside flag is not finite: + 1000*badchi and no gradient)
 *   grad [J, 1 + ntan]  d/d(vel, parameters in library order[, vsini]), the column
 *                       order of rvs_chisq_point_grad; the penalties are not
 *                       differentiated.  Nearest-neighbour templates (outside the grid,
 *                       a missing vertex): parameter columns exactly 0; the copy
 *                       branches of the FIR (vsini <= 0, NaN, refused width): vsini
 *                       column exactly 0.  Where the factorisation fails:
 *                       RVS_ST_CHOL_FALLBACK | RVS_ST_NONFINITE, value and gradient NaN.
 *   status [J]          OR-ed into, as by rvs_chisq_point_grad
 *   scratch             rvs_objective_grad_work_size(J, narm, ntan) bytes (0 for
 *                       arguments out of range)
 * rvs_objective_grad_ok (host arithmetic only, no device is touched): 1 where the
 * kernel covers an arm of this geometry -- npoly 1..10, ndim 1..4, 32 <= ntp,
 * 2*npix <= ntp, 3*ntp doubles + 8 KB <= 160 KB of LDS.  RVS_E_ARG, before any launch:
 * an arm rvs_objective_grad_ok refuses, a resolution matrix, a grid set, fast_interp,
 * arms of different ndim, ntan other than ndim or ndim + 1, a NULL array.
 * ---------------------------------------------------------------------- */
int rvs_objective_grad_ok(int npoly, int npix, int ntp, int ndim, int vsini_grad);
int64_t rvs_objective_grad_work_size(int J, int narm, int ntan);
int rvs_objective_grad(const rvs_objective_arm *arms, int narm, int npoly, int ntan,
                       const double *params, const double *vsini,
                       const int32_t *job_spec, int J, const double *vel,
                       double badchi, const double *basis_const, void *scratch,
                       double *out, double *grad, int32_t *status, void *stream);

/* The from-template form of rvs_objective_grad, for an evaluator that is no grid gather
 * (the MLP of rvs_template_nn): the unbroadened template of (job, arm) is row j of
 * templ[a] [J, ntp] float64 with its outside flag outside[a][j], taken -- MAX_VAL guard
 * included -- as rvs_objective_from_template takes them.  Behind the row everything is the
 * kernel of rvs_objective_grad; in place of its contraction at the knots the adjoint row
 *   tbar[a][j, n] = d chi^2_a / d templ[a][j, n]                   [J, ntp] float64
 * is written out (zeros for an arm that is skipped: a non-finite outside flag), the row
 * the evaluator's own reverse pass (rvs_template_nn_vjp) contracts with its Jacobian.
 * templ, outside and tbar are HOST arrays of narm device pointers.
 *   grad [J, 1 + vsini_grad]  d/d(vel[, vsini]); value, status and the rules for skipped
 *                             arms, copy branches and a failed factorisation as for
 *                             rvs_objective_grad
 *   scratch   rvs_objective_grad_from_template_work_size(J, narm, vsini_grad) bytes
 * rvs_objective_grad_from_template_ok (host arithmetic only): rvs_objective_grad_ok's rule
 * without the ndim bound of the cell record, which this form does not read.  RVS_E_ARG,
 * before any launch: what rvs_objective_grad refuses of an arm's geometry and options,
 * vsini_grad without vsini, a NULL array or row pointer.
 * rvs_objective_grad_join assembles grad [J, 1 + ndim + vsini_grad] = (vel, parameters,
 * vsini) from grad_vv, the [J, 1 + vsini_grad] gradient of that call, and gparams [narm]
 * (host array of device pointers to [J, ndim], the arms' rvs_template_nn_vjp results),
 * summed in arm order: exactly nothing from an arm whose outside flag -- read from that
 * call's scratch -- is not finite, NaN where out[j] is; the penalties are on the value
 * only. */
int rvs_objective_grad_from_template_ok(int npoly, int npix, int ntp, int vsini_grad);
int64_t rvs_objective_grad_from_template_work_size(int J, int narm, int vsini_grad);
int rvs_objective_grad_from_template(const rvs_objective_arm *arms, int narm, int npoly,
                                     int vsini_grad, const double *const *templ,
                                     const double *const *outside, const double *vsini,
                                     const int32_t *job_spec, int J, const double *vel,
                                     double badchi, const double *basis_const,
                                     void *scratch, double *const *tbar, double *out,
                                     double *grad, int32_t *status, void *stream);
int rvs_objective_grad_join(int narm, int J, int ndim, int vsini_grad, const void *scratch,
                            const double *const *gparams, const double *out,
                            const double *grad_vv, double *grad, void *stream);

/* rvs_objective_grad and rvs_objective_grad_from_template under per-spectrum resolution
 * matrices (A9): arms may carry pt.taps / pt.taps_stride / pt.nd as for rvs_objective_fused
 * (arms with and without a matrix may be mixed: an arm without one is a band of one
 * diagonal).  The band runs over the pixels' spline values in LDS,
 *   m_k = sum_d taps[s][k][d] raw[k - (nd-1)/2 + d]    (d ascending, s = job_spec[j]),
 * the products of rvs_objective_fused in its order, so the value is its value; the
 * band's transpose is applied to the one adjoint row,
 *   rawbar_j = sum_d taps[s][j + (nd-1)/2 - d][d] mbar[j + (nd-1)/2 - d]   (d ascending),
 * and the velocity component is formed behind it.  Every other argument, the outputs,
 * the scratch sizes and the rules for skipped arms are those of the call without the
 * suffix; with nd = 1 and taps of 1 the results are its bits.
 * rvs_objective_grad_resol_ok (host arithmetic only): 1 where the kernel covers an arm of
 * this geometry under a band of nd diagonals -- nd odd, 1..33; what rvs_objective_grad_ok
 * asks (ndim = 0: what rvs_objective_grad_from_template_ok asks, for the from-template
 * form); and 2*npix + nd - 1 <= ntp: the sigma-scaled row and the zero-padded row of the
 * band share one buffer of ntp doubles.  RVS_E_ARG, before any launch: what the call
 * without the suffix refuses except pt.taps, an arm rvs_objective_grad_resol_ok refuses,
 * a taps_stride that is neither 0 nor >= npix*nd. */
int rvs_objective_grad_resol_ok(int npoly, int npix, int ntp, int ndim, int nd,
                                int vsini_grad);
int rvs_objective_grad_resol(const rvs_objective_arm *arms, int narm, int npoly, int ntan,
                             const double *params, const double *vsini,
                             const int32_t *job_spec, int J, const double *vel,
                             double badchi, const double *basis_const, void *scratch,
                             double *out, double *grad, int32_t *status, void *stream);
int rvs_objective_grad_from_template_resol(
    const rvs_objective_arm *arms, int narm, int npoly, int vsini_grad,
    const double *const *templ, const double *const *outside, const double *vsini,
    const int32_t *job_spec, int J, const double *vel, double badchi,
    const double *basis_const, void *scratch, double *const *tbar, double *out,
    double *grad, int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * The objective of rvs_objective_grad WITH the Fisher matrix of the marginalised fit
 * (rvs_chisq_point_fisher's F = J^T (1 - U U^T) J), as one kernel per (job, arm), in
 * FORWARD mode: behind the value phases of rvs_objective_grad (the same value and
 * status) each of the K = 1 + ntan tangent rows -- the velocity's from the spline's
 * derivative, a parameter's gathered at the knots as rvs_template_polylinear_grad forms
 * it, vsini's from the tap derivatives of rvs_vsini_convolve_grad -- goes through the
 * value's own FIR, spline solve and resampling, one at a time, in the LDS buffers the
 * value has left.  The pixel-side state (the pixel adjoint, m/e and the K columns J_ki)
 * lives in a work row of (K + 2) npix doubles per (job, arm), written and read back by
 * the thread that owns the pixel.  No template row, tangent row or spline record goes to
 * HBM; no floating point atomics: repeated calls, permuted job lists and another work
 * size agree to the bit.  Replaces the chain rvs_template_polylinear_grad ->
 * rvs_vsini_convolve(_grad) -> rvs_spline_construct -> rvs_chisq_point_fisher (the
 * Jacobian of spec_fit.py:888-896's chi^2 that the reference takes by differences).
 * Arguments as for rvs_objective_grad, and
 *   fisher [J, K, K]    ordered (vel, parameters in library order[, vsini]), exactly
 *                       symmetric, as rvs_chisq_point_fisher delivers it
 *                       (rvs_proc_finish_fisher consumes it unchanged); rows and columns
 *                       exactly 0 where the gradient's column is; NaN where the value is;
 *                       an arm whose outside flag is not finite adds nothing
 *   work, work_bytes    rvs_objective_fisher_work_size(J, narm, ntan, npix_max) bytes
 *                       (npix_max: the largest pt.npix of the arms; 0 for arguments out
 *                       of range) hold all J jobs in one launch.  A smaller buffer is
 *                       taken too, down to the size of ONE job,
 *                       rvs_objective_fisher_work_size(1, narm, ntan, npix_max): the jobs
 *                       then go in launches of as many as fit, with the same results to
 *                       the bit.
 * rvs_objective_fisher_ok (host arithmetic only): rvs_objective_grad_ok's rule -- npoly
 * 1..10, ndim 1..4, 32 <= ntp, 2*npix <= ntp, 3*ntp doubles + 8 KB <= 160 KB of LDS.
 * RVS_E_ARG, before any launch: everything rvs_objective_grad refuses, and a work buffer
 * below the one-job size.
 * ---------------------------------------------------------------------- */
int rvs_objective_fisher_ok(int npoly, int npix, int ntp, int ndim, int vsini_grad);
int64_t rvs_objective_fisher_work_size(int J, int narm, int ntan, int npix_max);
int rvs_objective_fisher(const rvs_objective_arm *arms, int narm, int npoly, int ntan,
                         const double *params, const double *vsini,
                         const int32_t *job_spec, int J, const double *vel,
                         double badchi, const double *basis_const, void *work,
                         int64_t work_bytes, double *out, double *grad, double *fisher,
                         int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * Host side of the second minimiser of vel_fit.process (vel_fit.py:653-658:
 * scipy.optimize.minimize(method='BFGS', options={'hess_inv0': ...})): S
 * independent BFGS runs (scipy's _minimize_bfgs with its wolfe1 / wolfe2 line
 * searches and 2-point forward-difference gradients) advanced in lock-step.
 * The caller owns the objective:
 *     h = rvs_bfgs_begin(S, n, x0 [S,n], hess_inv0 [n,n] or NULL, gtol, c1, c2,
 *                        xrtol, maxiter (<= 0: 200 n))
 *     while ((rows = rvs_bfgs_pending(h, idx, X, cap)) > 0) {
 *         F[r] = objective(spectrum idx[r], point X[r, :]),  r < rows
 *         rvs_bfgs_feed(h, F, rows);
 *     }
 *     rvs_bfgs_result(h, x [S,n], fun [S], nit, nfev, status [S] (scipy's
 *                     warnflag), hess_inv [S,n,n] or NULL, &rounds);
 *     rvs_bfgs_end(h);
 * cap >= S (n + 1) rows always suffices.  n <= 16.  No GPU work in here.
 * ---------------------------------------------------------------------- */
void *rvs_bfgs_begin(int S, int n, const double *x0, const double *hess_inv0,
                     double gtol, double c1, double c2, double xrtol,
                     int maxiter);
int64_t rvs_bfgs_pending(void *h, int64_t *idx, double *X, int64_t cap_rows);
int rvs_bfgs_feed(void *h, const double *F, int64_t nrows);
int rvs_bfgs_result(void *h, double *x, double *fun, int32_t *nit,
                    int32_t *nfev, int32_t *status, double *hess_inv,
                    int64_t *rounds);
void rvs_bfgs_end(void *h);

/* The same runs around an objective that returns its gradient: scipy's
 * minimize(fun, x0, method='BFGS', jac=True, options={'hess_inv0': ...}), where
 * MemoizeJac calls `fun` once per new x and ScalarFunction hands out the value and
 * the gradient of that call.  Every pending request is ONE row per run, and its
 * reply is the row F[r, 0 .. n] = (f, df/dx_0 .. df/dx_{n-1}):
 *     h = rvs_bfgs_begin_jac(...)                     arguments of rvs_bfgs_begin
 *     while ((rows = rvs_bfgs_pending(h, idx, X, cap)) > 0) {     cap >= S suffices
 *         F[r, :] = (objective, gradient)(spectrum idx[r], point X[r, :])
 *         rvs_bfgs_feed_jac(h, F [rows, 1 + n], rows);
 *     }
 *     rvs_bfgs_result_jac(h, x, fun, nit, nfev, njev, status, hess_inv, &rounds);
 *     rvs_bfgs_end(h);
 * nfev / njev are scipy's: values and gradients ScalarFunction handed out (both
 * count an x once; the objective itself ran once per x).  rvs_bfgs_feed on a handle
 * of rvs_bfgs_begin_jac, rvs_bfgs_feed_jac on one of rvs_bfgs_begin, a row count
 * other than the pending one and a NULL array: RVS_E_ARG. */
void *rvs_bfgs_begin_jac(int S, int n, const double *x0, const double *hess_inv0,
                         double gtol, double c1, double c2, double xrtol,
                         int maxiter);
int rvs_bfgs_feed_jac(void *h, const double *F, int64_t nrows);
int rvs_bfgs_result_jac(void *h, double *x, double *fun, int32_t *nit,
                        int32_t *nfev, int32_t *njev, int32_t *status,
                        double *hess_inv, int64_t *rounds);

/* ------------------------------------------------------------------------
 * The tables that depend only on a wavelength grid, for G grids at once (one per
 * arm on the fast path; one per SPECTRUM for SDSS-style objects): built on the
 * device because on the host they cost ~10 ms per grid (LAPACK QR, searches).
 *
 * rvs_basis_build: the continuum basis get_basis (spec_fit.py:148-176) -- rbf != 0:
 * 1, x, x^2 and npoly-3 Gaussians at `cen` (device, np.linspace(-1, 1, npoly-3));
 * rbf == 0: Chebyshev T_i by numpy's Clenshaw recursion -- on x = the grid's own
 * range mapped to [-1, 1]; raw [G, npix+1, npoly] pixel-major (rows from a grid's
 * pixel count on are 0); ortho (nullable) the same function space orthonormalised
 * over the grid's pixels (modified Gram-Schmidt, twice) with logdet[g] =
 * 2 sum log R_jj, what the velocity-grid kernel reads (see rvs_chisq_grid).
 * lam [G, npix]; npix_g int32 [G] or NULL (every grid has npix pixels).
 * Limits: npoly <= 32 (what rvs_chisq_full takes), npix <= 16384; RVS_E_ARG beyond. */
int rvs_basis_build(const double *lam, const int32_t *npix_g, int G, int npix,
                    int npoly, int rbf, const double *cen, double *raw,
                    double *ortho, double *logdet, void *stream);
/* rvs_ccf_tables_build: the grid-dependent tables of rvs_ccf_preprocess(_g):
 * xind / rw [G, nfft] (make_ccf.py:355-357, 394-399; ccf_lam [nfft] = the FFT grid's
 * wavelengths, device), and with `continuum` the B-spline form of the k = 2
 * interpolating spline through the continuum nodes (make_ccf.py:155-164; FITPACK
 * knots and fpbspl): Eb [G, npix, 3], El [G, npix], istart [G, nnode], bin_start
 * [G, nnode + 1] (make_ccf.py:128-143, scipy.stats.binned_statistic ranges) from
 * nodes [G, nnode] / edges [G, nnode + 1] / nnode_g [G] (make_ccf.py:123-131,
 * computed by the caller: a log and an exp per node).  The collocation matrix and
 * its inverse (Cinv) stay with the caller (nnode <= 24). */
int rvs_ccf_tables_build(const double *lam, const int32_t *npix_g, int G, int npix,
                         const double *ccf_lam, int nfft, int continuum,
                         const double *nodes, const double *edges,
                         const int32_t *nnode_g, int nnode, int32_t *xind,
                         double *rw, double *Eb, int32_t *El, int32_t *istart,
                         int32_t *bin_start, void *stream);

/* ------------------------------------------------------------------------
 * A12  grid summary; replaces the tail of spec_fit.find_best
 * (spec_fit.py:1072-1092) and _quadratic_interp_min (:992-1015).
 * chisq [G, Np, Nv] (velocity fastest); vels + g*vel_stride -> [Nv];
 * nvel (nullable int32 [G]) = number of valid velocities of group g.
 * res [G, 8] = best_chi, best_vel, vel_err, kurtosis, skewness, i1 (vel idx),
 *              i2 (template idx), sum_i exp(-(chisq[i2, i] - best_chi) / 2);
 * probs [G, Nv] (nullable); entries from nvel[g] on are 0 and are never read
 * from chisq or vels.  status (nullable int32 [G], OR-ed into) gets
 * RVS_ST_QUAD_ASSERT where the reference's assert would have fired.
 * A group with nvel[g] < 1 (a refinement window that closed) reads neither
 * chisq nor vels: best_chi = +inf, best_vel = vel_err = kurtosis = skewness =
 * NaN, i1 = i2 = -1, res[7] = 0, probs[g, :] = 0, status untouched (vel_fit's
 * `lost` mask overwrites the same four numbers with NaN).
 * RVS_E_ARG for G, Np or Nv < 1.
 * ---------------------------------------------------------------------- */
int rvs_grid_moments(const double *chisq, const double *vels,
                     int64_t vel_stride, const int32_t *nvel, int G, int Np,
                     int Nv, int quadratic, double *res, double *probs,
                     int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * A15  CCF pre-processing of one arm; replaces make_ccf.preprocess_data
 * (make_ccf.py:330-414) with interp_masker (:288-327), get_continuum
 * (:105-152) and fit_resid (:155-164).  The k=2 interpolating continuum
 * spline is linear in its node values p: with C the B-spline collocation
 * matrix at the nodes, S(lam_k) = sum_{q<3} Eb[k,q] * (C^-1 p)[El[k]+q].  The
 * robust soft-L1 fit is a device Levenberg-Marquardt on the same objective.
 *
 * Eb float64 [npix, 3], El int32 [npix]   B-spline basis of every pixel
 * Cinv float64 [2, nnode, nnode]          inverse collocation matrix C^-1, then C
 * istart int32 [nnode-1]                  first pixel of every knot interval
 * bin_start int32 [nnode+1]  pixel ranges of the binned-median start
 * xind int32 [nfft], rw float64 [nfft]   rebin tables (xind<0: no coverage)
 * outputs: proc_spec, proc_ivar [B, nfft]; sse [B] = sum proc_spec^2 proc_ivar;
 *          cont [B, npix] (nullable), pfit [B, nnode] (nullable)
 * ---------------------------------------------------------------------- */
int rvs_ccf_preprocess(const double *lam, const double *spec,
                       const double *espec, const uint8_t *badmask, int npix,
                       int B, int continuum, const double *Eb, const int32_t *El,
                       const double *Cinv, const int32_t *istart, int nnode,
                       const int32_t *bin_start, const int32_t *xind,
                       const double *rw, int nfft, double maxerr,
                       double *proc_spec, double *proc_ivar, double *sse,
                       double *cont, double *pfit, int32_t *status,
                       void *stream);
/* ... on grid sets: spectrum b is observed on grid grid_id[b] with npix_g[g]
 * pixels and nnode_g[g] continuum nodes (make_ccf.py:123-131: the node count
 * follows the grid's wavelength range).  Every table holds one slice per grid:
 * lam [G, npix], Eb [G, npix, 3], El [G, npix], Cinv [G, 2, nnode, nnode] (grid g's
 * two nnode_g x nnode_g matrices packed at the start of its slice), istart
 * [G, nnode], bin_start [G, nnode + 1], xind / rw [G, nfft]; npix / nnode = the
 * largest grid = the row strides of spec, espec, badmask, cont / pfit. */
int rvs_ccf_preprocess_g(const double *lam, const double *spec, const double *espec,
                         const uint8_t *badmask, int npix, int B, int continuum,
                         const double *Eb, const int32_t *El, const double *Cinv,
                         const int32_t *istart, int nnode,
                         const int32_t *bin_start, const int32_t *xind,
                         const double *rw, int nfft, double maxerr,
                         double *proc_spec, double *proc_ivar, double *sse,
                         double *cont, double *pfit, int32_t *status,
                         const int32_t *grid_id, const int32_t *npix_g,
                         const int32_t *nnode_g, void *stream);

/* ------------------------------------------------------------------------
 * A14  FFT cross-correlation of one arm against T templates; replaces the
 * per-arm body of fitter_ccf.fit (fitter_ccf.py:112-161, 189-216).
 *
 * tfft, tfft2 complex128 [T, nfft/2+1] (ccfdat_%s.npz 'fft','fft2')
 * twid complex128 [nfft/2]   exp(+2 pi i k / nfft)
 * lag_pos int32 [nlag]  position of lag n = subind[l] in the LDS image of the
 *         half-size inverse FFT viewed as doubles: with p = rvs_ccf_fft_pos(nfft,
 *         n>>1) (digit-reversed output order of the radix-8 DIF passes),
 *         lag_pos = 2*p + (n&1)   (the image is not padded since round 2)
 * lag_vel float64 [nlag] ascending lag velocities (fitter_ccf.py:136-154)
 * ilo int32 [nvel], vgrid float64 [nvel]        linear-interp tables
 * chisq [B, T, nvel]: out = beta*out + interp(-2 c0 + c1) (continuum) or
 *                      interp(-c0^2/c1)
 * prune uint8 [n2/64 + n2/8], n2 = nfft/2 (nullable; used when n2 is a power of
 *         8): only the lags in lag_pos are read back, so the last two radix-8
 *         passes compute selected outputs only.  With p as above,
 *         prune[n2/64 + (p>>3)] has bit (p&7) set for every needed p, and
 *         prune[p>>6] has bit ((p>>3)&7) set (the outputs of the second-last
 *         pass that feed a needed 8-group).  Values are bit-identical to the
 *         unpruned transform.
 * work  complex128 [B, 2, nfft/2+1] scratch for conj rfft of spec*ivar, ivar (not
 *         touched by the persistent kernel of nfft 8192, whose block transforms its
 *         own spectrum in LDS; every other kernel reads it back)
 * Kernels behind the call (same interface, results equal to a few ulp): at nfft
 * 8192 (with `prune`) and 4096, nlag and nvel <= 512, T >= 2, one persistent
 * wave-specialised block per spectrum walks the T templates (ccf_xcorr_ws_kernel /
 * _ws2_kernel, csrc/ccf_fft.hip; without continuum normalisation it takes one of the
 * two correlations per iteration); otherwise one block per (spectrum, template).
 * rvs_option_set("xc_ws", 0) forces the latter.
 * ---------------------------------------------------------------------- */
int rvs_ccf_fft_pos(int nfft, int f);  /* host helper, see lag_pos */
/* doubles of `work` that rvs_ccf_xcorr with these shapes reads or writes (host; added
 * under ABI 18): 0 where the persistent kernel of nfft 8192 runs (work may be NULL
 * then), else B * 2 * (nfft/2 + 1) * 2.  has_prune: `prune` will not be NULL. */
int64_t rvs_ccf_xcorr_work_size(int nfft, int B, int T, int nlag, int nvel,
                                int has_prune);
int rvs_ccf_xcorr(const double *proc_spec, const double *proc_ivar, int nfft,
                  int B, const double *tfft, const double *tfft2, int T,
                  const double *twid, int continuum, const int32_t *lag_pos,
                  const double *lag_vel, int nlag, const int32_t *ilo,
                  const double *vgrid, int nvel, double beta,
                  const uint8_t *prune, double *chisq, double *work,
                  void *stream);

/* ------------------------------------------------------------------------
 * CCF template sets; replaces make_ccf.preprocess_model (make_ccf.py:167-221) with
 * get_continuum / fit_resid (:105-164) for M model rows (template x vsini) at once,
 * and the two np.fft.rfft of ccf_executor (:474-475).  One block per row.
 *
 * rows float64 [M, ntp]  flux on the library's template grid (already broadened by
 *        rvs_vsini_convolve where vsini is neither None nor 0)
 * f32row uint8 [M] (nullable)  != 0: the row holds float32 numbers -- np.exp of a
 *        float32 array (make_ccf.py:464-465) that no vsini kernel touched; numpy then
 *        takes medians, m * 1e-5 and (without continuum) interp1d's y_hi - y_lo in
 *        float32, and so does the kernel
 * erows float64 [M, ntp] (nullable)  the errors of get_continuum's caller; NULL:
 *        preprocess_model's max(1e-5 m, 1e-2 median(m))
 * Eb, El, Cinv, istart, nnode, bin_start  the tables of rvs_ccf_preprocess for the
 *        TEMPLATE grid (nodes from its own lam.min() / lam.max(), make_ccf.py:
 *        123-131); nnode <= 48.  Not read when continuum == 0.
 * lnlam float64 [ntp] = log(lam); logl float64 [npoints] = the FFT grid;
 * ihi int32 [npoints]  clip(searchsorted(lnlam, logl), 1, ntp - 1), or -1 where logl
 *        lies outside [lnlam[0], lnlam[ntp-1]] (interp1d fill_value = 1)
 * twid complex128 [npoints/2]  exp(+2 pi i k / npoints), as rvs_ccf_xcorr's
 * outputs: model [M, npoints]; fft, fft2 complex128 [M, npoints/2 + 1] = rfft(model),
 *        rfft(model^2) in numpy's order and sign (both NULL: no transforms; else
 *        npoints must be a power of two, 64 ... 16384); cont [M, ntp] (nullable): the
 *        fitted continuum, get_continuum's return value (before the floor at a
 *        hundredth of its median); pfit [M, nnode] (nullable): its node values;
 *        status int32 [M] (nullable, OR-ed into): RVS_ST_NONPOS_MEDIAN
 * Limits: 12 <= ntp <= RVS_CCF_MODEL_MAX_NTP (the row and the model values of the
 * fit's last evaluation live in LDS); RVS_E_ARG beyond, before any launch.
 * ---------------------------------------------------------------------- */
#define RVS_CCF_MODEL_MAX_NTP 9216
/* the rows of a call: rows[b] = dats[sel[b]] (dats float32 [ngrid, ntp], sel int64 [M]
 * on the device; a row number outside the library gives NaN), through numpy's float32
 * exp when exp_flag (specs[inds], np.exp(specs): make_ccf.py:459-465).  An entry point
 * of its own because that exp is neither expf nor torch's: numpy's float32 exp is not
 * correctly rounded, the non-normalised sets are held to the reference at 1e-12, and
 * rvs_vsini_convolve stands between this step and rvs_ccf_models_build. */
int rvs_ccf_model_rows(const float *dats, int64_t ngrid, const int64_t *sel,
                       int exp_flag, int ntp, int M, double *rows, void *stream);
int rvs_ccf_models_build(const double *rows, const uint8_t *f32row,
                         const double *erows, int ntp, int M, int continuum,
                         const double *Eb, const int32_t *El, const double *Cinv,
                         const int32_t *istart, int nnode, const int32_t *bin_start,
                         const double *lnlam, const double *logl, const int32_t *ihi,
                         int npoints, const double *twid, double *model, double *fft,
                         double *fft2, double *cont, double *pfit, int32_t *status,
                         void *stream);

/* argmin over (template, velocity) + 3-point parabola (fitter_ccf.py:218-236).
 * sse [B] is added to every entry (total_sse).  res [B,4] = best_id, best_vel,
 * best_pix, min value; best_ccf [B, nvel]. */
int rvs_ccf_select(const double *chisq, const double *sse, int narm_sse, int B,
                   int T, const double *vgrid, int nvel, double *res,
                   double *best_ccf, int32_t *status, void *stream);

/* rvs_ccf_xcorr of the LAST arm of a chunk and rvs_ccf_select in one call (added under
 * ABI 18): the persistent block of a spectrum keeps the minimum of what it stores to
 * chisq (+ the sum of sse [narm, B] over the arms) and, behind its walk, does the
 * selection for its spectrum -- res, best_ccf and status with the bits rvs_ccf_select
 * gives on the chisq the call leaves behind (which is still written in full).
 * Arguments as the two calls'.  RVS_E_ARG, before any launch, where rvs_ccf_xcorr
 * would not take the persistent kernel of nfft 8192 (another nfft, no `prune`, nlag or
 * nvel > 512, T < 2, option "xc_ws" 0) and for sse, res or best_ccf NULL: the caller
 * then makes the two calls. */
int rvs_ccf_xcorr_select(const double *proc_spec, const double *proc_ivar, int nfft,
                         int B, const double *tfft, const double *tfft2, int T,
                         const double *twid, int continuum, const int32_t *lag_pos,
                         const double *lag_vel, int nlag, const int32_t *ilo,
                         const double *vgrid, int nvel, double beta,
                         const uint8_t *prune, double *chisq, double *work,
                         const double *sse, int narm, double *res, double *best_ccf,
                         int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * A4  NN template evaluator; replaces NNInterpolator.forward
 * (nn/NNInterpolator.py:14-91), Mapper.forward (:159-171) and
 * RVSInterpolator.__call__ (nn/RVSInterpolator.py:36-42): float32 MLP
 * (Linear+SiLU)*(nlayer-1), Linear, on f32-input MFMA, float64
 * exp(clip(.,-300,300)) epilogue.
 * W[l] float32 [dout_l, din_l] row-major (torch Linear.weight), b[l] [dout_l]
 * ---------------------------------------------------------------------- */
int rvs_template_nn(const double *params, int B, int ndim, uint32_t log_mask,
                    const double *M, const double *S, int nlayer,
                    const float *const *W, const float *const *b,
                    const int32_t *dims, float *act0, float *act1,
                    double *templ, void *stream);

/* rvs_template_nn with the derivative of the template by every physical parameter, in
 * forward mode: templ [B, 1 + ndim, ntp] (ntp = dims[nlayer]), row 0 the template,
 * row 1 + k d template / d p_k.  Arguments as rvs_template_nn; act1 holds
 * B (1 + ndim) rows of the widest layer (the last hidden layer's rows: the hidden stack
 * is one launch, so no second image is needed); act0 is not used and may be any
 * non-NULL pointer.
 *   Input.   Mapper.forward is x_d = (f32(q_d) - M_d) / S_d, q_d = log10(p_d) for a
 *            parameter in log_mask, else p_d.  The float32 casts are taken as the
 *            identity: dx_d / dp_k = delta_dk s_k / S_k, s_k = 1 / (p_k ln 10) under
 *            the logarithm and 1 otherwise, at the float64 p_k.  The tangent of
 *            parameter k enters the network as the one-hot e_k (the first layer's
 *            tangent is column k of W[0]); s_k / S_k is applied in float64 by the
 *            last epilogue, so no float32 value is scaled by it.
 *   Hidden.  z = W a + b, sigma = 1 / (1 + expf(-z)), a+ = z sigma:
 *            adot+ = sigma (1 + z (1 - sigma)) (W adot) -- the same product without
 *            the bias, times the SiLU derivative at the VALUE row's z of the column.
 *   Last.    y = W a + b, ydot_k = W adot_k.  Row 0: t = exp(clip(y, -300, 300)) in
 *            float64; row 1 + k: t ydot_k s_k / S_k, and exactly 0 where |y| > 300
 *            (the clip is flat there).
 *   A job whose mapped parameters are not all finite (NaN, a non-positive value under
 *   the logarithm) has NaN in all 1 + ndim rows, as rvs_template_tri_grad has.
 * Row 0 carries the bits of rvs_template_nn for the same arguments (finite jobs): the
 * value row goes through the same products in the same order.  The tangents are
 * float32 arithmetic: exact to float32 rounding, not to float64's.  No float atomics:
 * two calls give the same bits.  The rows of a job lie in one block tile of either
 * kernel (csrc/nn.hip); the call's HBM traffic beyond the weights is the float32 rows
 * of the last hidden layer and the B (1 + ndim) ntp doubles it writes.
 * Scope (RVS_E_ARG beyond, before any launch): the networks of rvs_template_nn's
 * fused hidden stack -- 3 <= nlayer <= 7, every hidden width <= 256 and, from the
 * second layer's input on, a multiple of 32 (the last layer's input excepted) --
 * with ndim <= 6 and B (1 + ndim) < 2^28. */
int rvs_template_nn_grad(const double *params, int B, int ndim, uint32_t log_mask,
                         const double *M, const double *S, int nlayer,
                         const float *const *W, const float *const *b,
                         const int32_t *dims, float *act0, float *act1,
                         double *templ /* [B, 1 + ndim, ntp] */, void *stream);

/* The reverse pass of the same network: ONE adjoint row per job back through the net,
 * whatever ndim is (rvs_template_nn_grad sends ndim rows forward),
 *   gparams[j, k] = sum_n tbar[j, n] d templ[j, n] / d p_k        [B, ndim] float64
 * for templ [B, ntp], the value rows rvs_template_nn / rvs_template_nn_arms wrote for
 * `params`, and tbar [B, ntp], the adjoint rows d chi^2 / d templ that
 * rvs_objective_grad_from_template writes.  Network arguments as rvs_template_nn.
 *   Last.    ybar_n = tbar_n templ_n in float64, exactly 0 where templ_n is one of the
 *            clip's own two values exp(+-300) (the clip is flat there).  Each row is
 *            divided by the power of two 2^e, e = the exponent of max_n |ybar_n|, before
 *            the float32 cast, and 2^e is multiplied back in float64: exact both ways, so
 *            the result scales exactly with tbar.  abar = ybar W_L on the float32-input
 *            MFMA, ntp cut into runs of 256 pixels, one partial sum per run in `work`,
 *            added in run order: no float atomics, and the partition does not depend on B.
 *   Hidden.  The forward pass of the job's row is computed again, every layer's z kept in
 *            LDS; delta_l = abar_l sigma (1 + z (1 - sigma)), abar_{l-1} = delta_l W_l.
 *   Input.   gparams_k = xbar_k s_k / S_k in float64, s_k as for rvs_template_nn_grad; NaN
 *            in all components of a job whose mapped parameters are not all finite.
 * Float32 arithmetic: exact to float32 rounding of the sum over the pixels.  Two calls
 * give the same bits; a job has the same bits alone and inside any batch.
 *   work     rvs_template_nn_vjp_work_size(B, nlayer, dims) bytes (0 out of scope)
 * Scope (RVS_E_ARG beyond, before any launch): that of rvs_template_nn_grad -- 3 <=
 * nlayer <= 7, hidden widths <= 256 and multiples of 32 from the second layer's input on
 * (the last layer's input excepted), ndim <= 6. */
int64_t rvs_template_nn_vjp_work_size(int B, int nlayer, const int32_t *dims);
int rvs_template_nn_vjp(const double *params, int B, int ndim, uint32_t log_mask,
                        const double *M, const double *S, int nlayer,
                        const float *const *W, const float *const *b,
                        const int32_t *dims, const double *templ, const double *tbar,
                        void *work, double *gparams, void *stream);

/* Outside flag of an NN library; replaces OutsideInterpolator.__call__
 * (nn/RVSInterpolator.py:63-71) as SpecInterpolator.outsideFlag calls it on the
 * Mapper-transformed point (spec_inter.py:257-272, nn/NNInterpolator.py:159-171):
 * outside[j] = max(max_f xeqs[f].(p0,p1,1), max_f yeqs[f].(p2..,1), 0)^2.
 * xeqs [nfx, 3], yeqs [nfy, ndim-1]: scipy.spatial.ConvexHull(...).equations of
 * the first two / the remaining mapped coordinates of the training points
 * (built once by the caller); params, M, S, log_mask as rvs_template_nn;
 * mapped != 0: params ARE the Mapper's float64 output (M, S, log_mask unused).
 * A NaN parameter gives NaN (the arm is then skipped, spec_fit.py:888-893).
 * nfx == nfy == 0: a library without hulls (no outside check) -- outside[] is
 * zeroed on `stream`, nothing else is read. */
int rvs_nn_outside(const double *params, int B, int ndim, uint32_t log_mask,
                   const double *M, const double *S, int mapped,
                   const double *xeqs, int nfx, const double *yeqs, int nfy,
                   double *outside, void *stream);

/* ------------------------------------------------------------------------
 * the optimiser stage of vel_fit.process
 * (vel_fit.py:596-650).  S Nelder-Mead simplices (scipy's algorithm, which the
 * reference calls through scipy.optimize.minimize(method='Nelder-Mead',
 * options={fatol, xatol, initial_simplex, maxiter, maxfev=inf}), :627-637) live
 * in device memory and advance in lock-step; between the calls below the
 * caller evaluates the objective on (list, X) with the entry points above.
 *   sim [S, N+1, N], fsim [S, N+1] ordered ascending on entry; nit, nfev [S];
 *   flags [S]: bit0 active, bit1 converged, bit2 shrink pending;
 *   counts int32[8] (device): [0] |list1|, [1] |list2|, [2] |list3|,
 *   [3] simplices stepping this round, [4] simplices parked for a shrink,
 *   [5] rvs_nm_run: rows of a round that evaluates all four candidate points.
 * Every call takes `jbound`, a host-side upper bound of the job count (the
 * live count is read from `counts` on the device), so no host synchronisation
 * is needed inside a round; list/X entries in [count, jbound) are padded with
 * a copy of entry 0.
 * ---------------------------------------------------------------------- */
int rvs_nm_begin(int S, int N, double xatol, double fatol, int maxiter,
                 const double *sim, const double *fsim, const int32_t *nit,
                 int32_t *flags, int32_t *list1, double *X1, int32_t *counts,
                 int jbound, void *stream);
int rvs_nm_decide(int N, const double *sim, const double *fsim,
                  const int32_t *list1, const double *F1, int32_t *cases,
                  int32_t *pos2, int32_t *list2, double *X2, int32_t *counts,
                  int jbound, void *stream);
int rvs_nm_update(int N, double *sim, double *fsim, int32_t *nit, int32_t *nfev,
                  const int32_t *list1, const double *X1, const double *F1,
                  const int32_t *cases, const int32_t *pos2, const double *X2,
                  const double *F2, int32_t *flags, int32_t *counts, int jbound,
                  void *stream);
int rvs_nm_collect(int S, const int32_t *flags, int32_t *list3, int32_t *counts,
                   void *stream);
int rvs_nm_shrink_point(int N, int k, double *sim, const int32_t *list3,
                        double *X3, const int32_t *counts, int jbound,
                        void *stream);
int rvs_nm_shrink_store(int N, int k, double *sim, double *fsim, int32_t *nit,
                        int32_t *nfev, int32_t *flags, const int32_t *list3,
                        const double *F3, int32_t *counts, int jbound,
                        void *stream);

/* vel_fit.ParamMapper.forward + the range/finiteness guard of chisq_func +
 * VSiniMapper.to_vsini + the priors of chisq_func0 (vel_fit.py:95-254) for J
 * rows X [J, n] = (vel, [vsini], free stellar parameters).  src [ndim] (host):
 * column of X feeding stellar parameter i or -1 (fixed: fixed[S, ndim]);
 * vsini_col < 0: vsini_fixed[S]; vsini == NULL: no rotation.  Rows that
 * chisq_func answers with 1e30 get bad = 1 and harmless inputs (vel 0, safe[S,
 * ndim]).  rvs_proc_finish: F = bad ? 1e30 : chi + extra; job status bits of
 * the live rows (j < counts[cidx], or all when counts == NULL) are OR-ed into
 * spec_status[job_spec[j]]. */
int rvs_proc_map(int J, int n, int ndim, const double *X, const int32_t *list,
                 const int32_t *src, int vsini_col, const double *fixed,
                 const double *vsini_fixed, const double *safe,
                 const double *prior_mean, const double *prior_isig,
                 double min_vel, double max_vel, double max_vsini,
                 int32_t *job_spec, double *vel, double *vsini, double *params,
                 double *extra, int32_t *bad, void *stream);
int rvs_proc_finish(int J, const int32_t *counts, int cidx, const double *chi,
                    const double *extra, const int32_t *bad,
                    const int32_t *job_spec, const int32_t *job_status,
                    double *F, int32_t *spec_status, void *stream);

/* The rounds themselves, driven from C (what a caller of the entry points above
 * does per round, with the fused objective as chisq_func): blocks the calling
 * host thread until every simplex has stopped.  `m` holds the state arrays of
 * rvs_nm_* (fsim ordered, as for rvs_nm_begin), `o` the arguments of
 * rvs_proc_map / rvs_objective_fused / rvs_proc_finish and their row buffers
 * (capacity S rows; scratch: rvs_objective_work_size(S, narm) bytes).
 * stats (nullable) int64[3] = rounds, objective calls, rows evaluated. */
typedef struct rvs_nm_state {
  double *sim, *fsim, *X1, *X2, *F1, *F2;
  int32_t *nit, *nfev, *flags, *list1, *list2, *list3, *cases, *pos2, *counts;
  int32_t S, N;
} rvs_nm_state;
/* One arm's MLP evaluator for rvs_nm_run: the arguments of rvs_template_nn and
 * rvs_nn_outside (xeqs == NULL: no hull, outside = 0), and the buffers the
 * round's template rows / outside flags go to ([>= S, ntp] / [>= S], device). */
typedef struct rvs_nm_nn_arm {
  const double *M, *S;
  const float *const *W, *const *b; /* HOST arrays of nlayer device pointers */
  const int32_t *dims;              /* HOST [nlayer + 1] */
  float *act0, *act1;
  double *templ, *outside;
  const double *xeqs, *yeqs;
  int32_t nlayer, nfx, nfy;
  uint32_t log_mask;
} rvs_nm_nn_arm;

/* rvs_template_nn + rvs_nn_outside of narm MLPs at the same B rows of `params`
 * (an optimiser round: a few hundred rows per arm, where three dependent launch
 * chains cost more than their arithmetic): three launches in all when the
 * networks have one shape up to the output width, else arm by arm.  Results in
 * arms[a].templ / .outside; same values as the per-arm calls. */
int rvs_template_nn_arms(const double *params, int B, int ndim, int narm,
                         const rvs_nm_nn_arm *arms, void *stream);
/* ... of the first min(B, njobs_dev[0]) rows only (a count on the device, as in
 * rvs_objective_fused_n; the grouped launches honour it, the arm-by-arm fallback
 * evaluates all B rows).  NULL = all B. */
int rvs_template_nn_arms_n(const double *params, int B, const int32_t *njobs_dev,
                           int ndim, int narm, const rvs_nm_nn_arm *arms,
                           void *stream);

/* One arm's Delaunay evaluator for rvs_nm_run / rvs_bfgs_run: the arguments of
 * rvs_template_tri_buckets and the buffers the round's template rows / outside flags /
 * simplex ids go to ([>= rows, ntp] / [>= rows] / int32 [>= rows], device). */
typedef struct rvs_nm_tri_arm {
  const double *dats, *transform, *extraflags;
  const int32_t *simplices;
  double *templ, *outside;
  int32_t *simplex;
  rvs_tri_buckets buckets;
  int32_t ntp, nsimplex, exp_flag;
  uint32_t log_mask;
} rvs_nm_tri_arm;

typedef struct rvs_nm_objective {
  const rvs_objective_arm *arms;
  const double *fixed, *vsini_fixed, *safe, *prior_mean, *prior_isig;
  double *vel, *vsini, *params, *extra, *chi;
  int32_t *job_spec, *bad, *jstatus, *status;
  void *scratch;
  double min_vel, max_vel, max_vsini, badchi;
  int32_t narm, npoly, n, ndim, vsini_col;
  int32_t src[8];
  /* NULL: regular-grid libraries, rvs_objective_fused.  Else [narm]: MLP
   * libraries -- a round's objective is rvs_template_nn + rvs_nn_outside per
   * arm, then rvs_objective_from_template (vel_fit.py:505-737 with
   * nn/RVSInterpolator.py:36-71 as the evaluator) */
  const rvs_nm_nn_arm *nn;
  /* NULL, or [narm]: Delaunay libraries on every arm (spec_inter.py:11-59) -- a
   * round's objective is rvs_template_tri_buckets per arm, then
   * rvs_objective_from_template.  At most one of nn / tri is set. */
  const rvs_nm_tri_arm *tri;
} rvs_nm_objective;
int rvs_nm_run(const rvs_nm_state *m, const rvs_nm_objective *o, double xatol,
               double fatol, int maxiter, int sync_every, int64_t *stats,
               void *stream);

/* The second minimiser of vel_fit.process (vel_fit.py:653-658: scipy's BFGS from the
 * simplex optimum, `second_minimizer`, the default of utils.py:26) with its rounds
 * on the device: the S runs are the state machines of rvs_bfgs_begin / _pending /
 * _feed (one source, csrc/bfgs_machine.h), one thread per spectrum; the rows they
 * ask for -- a value, the n forward-difference points of a gradient, or both -- are
 * gathered into one list per round and evaluated by the objective of rvs_nm_run in
 * chunks of `cap` rows (the row capacity of o's buffers), the row counts staying on
 * the device.  Blocks the calling host thread until every run has ended.
 *   runs      S * rvs_bfgs_run_bytes() bytes of device memory (8-byte aligned)
 *   x0 [S, n] start points, hess_inv0 [n, n] (device; NULL = identity)
 *   x [S, n], fun [S], hess_inv [S, n, n] (nullable), nit / nfev / status [S]
 *             (scipy's warnflag): results
 *   nreq, off [S]; list [S (n + 1)]; X [S (n + 1), n]; F [S (n + 1)]; counts [32]:
 *             work arrays (list zero-filled by the caller)
 *   n = o->n <= 8; S (n + 1) <= 24 cap; maxiter <= 0: 200 n
 * stats (nullable) int64[3] = rounds, objective calls, rows launched. */
typedef struct rvs_bfgs_state {
  void *runs;
  const double *x0, *hess_inv0;
  double *x, *fun, *hess_inv;
  int32_t *nit, *nfev, *status;
  int32_t *nreq, *off, *list, *counts;
  double *X, *F;
  double gtol, c1, c2, xrtol;
  int32_t S, n, cap, maxiter;
} rvs_bfgs_state;
int64_t rvs_bfgs_run_bytes(void);
int rvs_bfgs_run(const rvs_bfgs_state *b, const rvs_nm_objective *o,
                 int sync_every, int64_t *stats, void *stream);

/* ------------------------------------------------------------------------
 * The second minimiser on the analytic gradient: scipy's
 * minimize(vel_fit.chisq_func_grad, x, method='BFGS', jac=True, hess_inv0=...) for S
 * spectra, the rounds on the device.
 *
 * rvs_proc_finish_grad is to vel_fit.chisq_func_grad what rvs_proc_finish is to
 * chisq_func: from the gradient chain's chi [J] and grad [J, 1 + ntan] -- ordered
 * (vel, stellar parameters in library order, vsini last when it is fitted: ntan =
 * ndim or ndim + 1) -- and what rvs_proc_map wrote for the rows X [J, n], it forms
 * F [J, 1 + n]: F[j, 0] = bad ? 1e30 : chi + extra as rvs_proc_finish does, then the
 * derivative by every column of X: the velocity's copied; a fitted parameter's taken
 * through src (HOST [ndim], as for rvs_proc_map), plus 2 (p - mean) isig^2 where
 * prior_isig is not 0; the vsini column's (d/dvsini if 0 < x < max_vsini, else 0)
 * + 2 (x - clamp(x, 0, max_vsini)).  A bad row is (1e30, zeros).  Status bits of the
 * live rows are OR-ed into spec_status[job_spec[j]] as by rvs_proc_finish.
 * RVS_E_ARG: a NULL array, n > 8, ndim > 6, ntan != ndim + (vsini_col >= 0), a src
 * entry that is 0, vsini_col or >= n, columns of X without a source. */
int rvs_proc_finish_grad(int J, int n, int ndim, int ntan, const int32_t *counts,
                         int cidx, const double *chi, const double *grad,
                         const double *X, const double *params, const double *extra,
                         const int32_t *bad, const int32_t *job_spec,
                         const int32_t *job_status, const int32_t *src,
                         int vsini_col, const double *prior_mean,
                         const double *prior_isig, double max_vsini, double *F,
                         int32_t *spec_status, void *stream);

/* One arm of the gradient chain: its template library -- tri == 0: a regular grid,
 * the arguments of rvs_template_polylinear_grad (dats float32; lens, ptp HOST arrays);
 * tri == 1: a Delaunay library, the arguments of rvs_template_tri_buckets_grad
 * (buckets.cell_start != NULL) or rvs_template_tri_grad (dats float64); tri == 2: an
 * MLP library -- dats points to a HOST rvs_nm_nn_arm with the arguments of
 * rvs_template_nn_grad and rvs_nn_outside, whose act1 holds cap (1 + ndim) rows of the
 * widest layer (float32; the caller's, NOT counted by rvs_grad_chain_work_size, whose
 * formula is unchanged; act0 any non-NULL pointer) and whose templ / outside are
 * not read (the rows go to this struct's).  xeqs == NULL: no hull, outside is zeroed for
 * every job -- a job with a non-finite mapped parameter then has NaN rows and a clean
 * flag, and its chi^2 is whatever rvs_chisq_point_grad makes of NaN rows (status
 * RVS_ST_NONFINITE), as on the value path; with a hull rvs_nn_outside answers NaN and
 * the job takes the penalty.  (Any other non-zero tri means Delaunay, as before 2 had
 * a meaning of its own.) -- the knots and
 * rvs_spline_factors of its template grid, and the caller's row buffers for `cap` rows
 * with K = 1 + ntan template rows each:
 *   templ   [cap, K, ntp]     the evaluator's rows (1 + ndim per job)
 *   templ2  [cap, K, ntp]     the broadened rows (vsini_mode != 0)
 *   coef    [cap, K, ntp, 4]  form-1 spline records: rvs_point_arm.coef of the arm
 *   outside, penalty [cap]    penalty: rvs_point_arm.penalty of the arm
 *   simplex int32 [cap]       (Delaunay)
 *   vs_rows, out_rows [cap (1 + ndim)]  (vsini_mode == 1: vsini / outside per row) */
typedef struct rvs_grad_arm {
  const void *dats;
  const int64_t *idgrid;
  const double *uvecs, *vecs_s;
  const int32_t *lens;
  const double *ptp;
  const double *transform, *extraflags;
  const int32_t *simplices;
  const double *knots, *factors;
  double *templ, *templ2, *coef, *outside, *penalty, *vs_rows, *out_rows;
  int32_t *simplex;
  rvs_tri_buckets buckets;
  int64_t ngrid;
  double lnstep;
  int32_t tri, nsimplex, ntp, exp_flag, spline_form;
  uint32_t log_mask;
} rvs_grad_arm;

/* The chain for the rows of a round: arms / point / basis_const are HOST arrays [narm];
 * `point` are the descriptors rvs_chisq_point_grad takes (polysT the orthonormalised
 * basis, basis_const its log-determinant constant, coef / penalty the arm's buffers
 * above); pen_scale as rvs_point_arm.pen_scale (device [S] or NULL).
 *   vsini_mode  0 no rotation; 1 vsini fixed (rvs_vsini_convolve over the 1 + ndim
 *               rows); 2 vsini fitted (rvs_vsini_convolve_grad, ntan = ndim + 1)
 *   point_work  rvs_chisq_point_grad_work_size(cap, narm, ntan) bytes
 *   chi [cap], grad [cap, 1 + ntan]   the chain's results of a chunk
 *   njev [S]    out: gradients handed out per run (scipy's njev)
 * rvs_grad_chain_work_size: bytes of all of these buffers together, for choosing cap
 * (ntp HOST [narm]); 0 for arguments out of range. */
typedef struct rvs_grad_chain {
  const rvs_grad_arm *arms;
  const rvs_point_arm *point;
  const double *basis_const;
  const double *pen_scale;
  void *point_work;
  double *chi, *grad;
  int32_t *njev;
  int32_t narm, ntan, cap, vsini_mode;
} rvs_grad_chain;
int64_t rvs_grad_chain_work_size(int cap, int narm, int ntan, const int32_t *ntp,
                                 int vsini_mode);

/* rvs_bfgs_run with the machine of rvs_bfgs_begin_jac: a run asks for ONE row per
 * request and reads (f, grad f) = F[row, 0 .. n]; a round is advance -> scan -> emit
 * (the kernels of rvs_bfgs_run) -> per chunk of g->cap rows rvs_proc_map, the gradient
 * chain (per arm the template rows and their tangents, the broadening, the spline
 * records; rvs_chisq_point_grad over all arms) and rvs_proc_finish_grad, with no
 * interpreter in between; the host looks at the counters as rvs_bfgs_run does.
 * `b` as for rvs_bfgs_run (its buffers at their sizes there; b->cap is not read);
 * `o`: the mapping's tables and row buffers (capacity >= g->cap rows), narm, npoly,
 * badchi, status; o->arms / nn / tri / chi / scratch are not read.
 * n = o->n <= 8, ndim <= 6, S <= 24 g->cap.  stats as for rvs_bfgs_run. */
int rvs_bfgs_run_grad(const rvs_bfgs_state *b, const rvs_nm_objective *o,
                      const rvs_grad_chain *g, int sync_every, int64_t *stats,
                      void *stream);

/* rvs_bfgs_run_grad with the rows' (value, gradient) from ONE rvs_objective_grad call
 * per chunk in place of the per-arm template, broadening and spline stages and the
 * rvs_chisq_point_grad call; rvs_proc_map and rvs_proc_finish_grad are unchanged.
 * garms [narm] (HOST): the arms of rvs_objective_grad (pt.polysT the orthonormalised
 * basis), basis_const [narm] (HOST, or NULL), gwork:
 * rvs_objective_grad_work_size(g->cap, narm, g->ntan) bytes.  From `g` only chi, grad,
 * njev, cap, ntan, vsini_mode and narm are read (no row buffer is needed).  RVS_E_ARG
 * also for what rvs_objective_grad refuses. */
int rvs_bfgs_run_grad_fused(const rvs_bfgs_state *b, const rvs_nm_objective *o,
                            const rvs_grad_chain *g, const rvs_objective_arm *garms,
                            const double *basis_const, void *gwork, int sync_every,
                            int64_t *stats, void *stream);

/* rvs_bfgs_run_grad_fused on MLP libraries: per chunk rvs_proc_map, the rows' templates
 * and outside flags from the networks of o->nn (rvs_template_nn_arms_n),
 * rvs_objective_grad_from_template, rvs_template_nn_vjp per arm, rvs_objective_grad_join,
 * rvs_proc_finish_grad.  garms [narm] (HOST) as for rvs_objective_grad_from_template,
 * gwork: rvs_objective_grad_from_template_work_size(g->cap, narm, vsini fitted) bytes.
 * The adjoint rows and the reverse pass's work are the caller's, HOST arrays of narm
 * device pointers: tbar [cap, ntp], vjp_work (rvs_template_nn_vjp_work_size(g->cap, ...)
 * bytes), gparams [cap, ndim]; grad_vv [cap, 1 + (vsini fitted)].  From `g` what
 * rvs_bfgs_run_grad_fused reads; no struct changed.  ndim <= 6.  RVS_E_ARG also for what
 * rvs_objective_grad_from_template and rvs_template_nn_vjp refuse. */
int rvs_bfgs_run_grad_fused_nn(const rvs_bfgs_state *b, const rvs_nm_objective *o,
                               const rvs_grad_chain *g, const rvs_objective_arm *garms,
                               const double *basis_const, void *gwork,
                               double *const *tbar, void *const *vjp_work,
                               double *const *gparams, double *grad_vv, int sync_every,
                               int64_t *stats, void *stream);

/* rvs_bfgs_run_grad_fused on Delaunay libraries (vel_fit.py:653-658 with
 * spec_inter.py:11-59 as the evaluator): per chunk rvs_proc_map, the rows' templates,
 * outside flags and simplex ids from the triangulations of o->tri into the buffers of
 * o->tri[a] (the bucketed find_simplex of rvs_template_tri_buckets),
 * rvs_objective_grad_from_template, rvs_template_tri_vjp per arm,
 * rvs_objective_grad_join, rvs_proc_finish_grad.  garms, gwork, tbar, gparams, grad_vv as
 * for rvs_bfgs_run_grad_fused_nn; the reverse step needs no work buffer.  No struct
 * changed.  RVS_E_ARG for o->tri == NULL, an arm without its row buffers or bucket
 * grid, ndim > 6, and what rvs_objective_grad_from_template refuses.
 * On an MI355X (medians, the legs alternating in one job): the gradient of
 * 8192 jobs on three DESI-shape Delaunay arms through this sequence 7.97 ms against
 * 20.43 ms on the chain and 19.70 ms for the six differenced value calls; the polish of
 * 2000 spectra 0.173 s against 0.476 s (rvs_bfgs_run_grad) and 0.356 s (rvs_bfgs_run). */
int rvs_bfgs_run_grad_fused_tri(const rvs_bfgs_state *b, const rvs_nm_objective *o,
                                const rvs_grad_chain *g, const rvs_objective_arm *garms,
                                const double *basis_const, void *gwork,
                                double *const *tbar, double *const *gparams,
                                double *grad_vv, int sync_every, int64_t *stats,
                                void *stream);

/* The three runs above under resolution matrices: the rows' (value, gradient) from
 * rvs_objective_grad_resol / rvs_objective_grad_from_template_resol, garms with pt.taps /
 * pt.nd as those calls take them; every other argument as for the run without the
 * suffix.  RVS_E_ARG also for an arm rvs_objective_grad_resol_ok refuses. */
int rvs_bfgs_run_grad_fused_resol(const rvs_bfgs_state *b, const rvs_nm_objective *o,
                                  const rvs_grad_chain *g, const rvs_objective_arm *garms,
                                  const double *basis_const, void *gwork, int sync_every,
                                  int64_t *stats, void *stream);
int rvs_bfgs_run_grad_fused_nn_resol(const rvs_bfgs_state *b, const rvs_nm_objective *o,
                                     const rvs_grad_chain *g,
                                     const rvs_objective_arm *garms,
                                     const double *basis_const, void *gwork,
                                     double *const *tbar, void *const *vjp_work,
                                     double *const *gparams, double *grad_vv,
                                     int sync_every, int64_t *stats, void *stream);
int rvs_bfgs_run_grad_fused_tri_resol(const rvs_bfgs_state *b, const rvs_nm_objective *o,
                                      const rvs_grad_chain *g,
                                      const rvs_objective_arm *garms,
                                      const double *basis_const, void *gwork,
                                      double *const *tbar, double *const *gparams,
                                      double *grad_vv, int sync_every, int64_t *stats,
                                      void *stream);

/* ------------------------------------------------------------------------
 * The second minimiser as Levenberg-Marquardt on the Fisher matrix
 * (config['second_minimizer_lm']): Nielsen's damping with Marquardt's diagonal scaling
 * on (value, gradient, Gauss-Newton Hessian) rows, for S spectra.
 *
 * rvs_proc_finish_fisher is rvs_proc_finish_grad (its arguments, checks, value, gradient
 * and status handling: the same statements, the same bits) with the chain's
 * fisher [J, K, K], K = 1 + ntan, ordered (vel, library parameters, vsini last), and
 * forms F [J, 1 + n + n (n + 1) / 2] = (f, grad f over X's columns, H: the lower
 * triangle row-major over X's columns), H the Gauss-Newton Hessian of chisq_func in the
 * optimiser's coordinates: H_ab = 2 fisher[row of a, row of b] (the matrix is in the
 * 0.5 chi^2 convention); fixed parameters have no row or column; + 2 isig^2 on the
 * diagonal of a parameter with a prior; the vsini row and column are the matrix's where
 * 0 < x < max_vsini, else 0, with + 2 on its diagonal where x is outside
 * [0, max_vsini] (the clamp penalty's second derivative).  log det A and the outside
 * penalties add nothing.  A bad row is (1e30, zeros, zeros).  One thread per row, no
 * float atomics.  RVS_E_ARG as rvs_proc_finish_grad, and for fisher == NULL. */
int rvs_proc_finish_fisher(int J, int n, int ndim, int ntan, const int32_t *counts,
                           int cidx, const double *chi, const double *grad,
                           const double *fisher, const double *X, const double *params,
                           const double *extra, const int32_t *bad,
                           const int32_t *job_spec, const int32_t *job_status,
                           const int32_t *src, int vsini_col, const double *prior_mean,
                           const double *prior_isig, double max_vsini, double *F,
                           int32_t *spec_status, void *stream);

/* What the Fisher form of the gradient chain needs beside an rvs_grad_chain (which is
 * unchanged; its point_work is not used by this form):
 *   fisher_work  rvs_chisq_point_fisher_work_size(cap, narm, ntan) bytes
 *   fisher       [cap, 1 + ntan, 1 + ntan]
 * rvs_fisher_chain_work_size: rvs_grad_chain_work_size plus these two; 0 for arguments
 * out of range. */
typedef struct rvs_fisher_chain {
  void *fisher_work;
  double *fisher;
} rvs_fisher_chain;
int64_t rvs_fisher_chain_work_size(int cap, int narm, int ntan, const int32_t *ntp,
                                   int vsini_mode);

/* The machine on the host (csrc/lm_machine.h, one source with rvs_lm_run), shaped like
 * the rvs_bfgs_*_jac family: begin -> { pending -> the caller's objective -> feed } ->
 * result -> end.  A request is ONE row per live run; its reply is a row of
 * rvs_proc_finish_fisher, F [rows, 1 + n + n (n + 1) / 2].
 *   begin    x0 [S, n], n <= 8; gtol: ends where max |g_i| <= gtol (scipy BFGS's
 *            test); xtol, tau, mu_max <= 0: 1e-10, 1e-3, 1e16; maxiter <= 0: 200 n.
 *            NULL for bad arguments
 *   pending  idx [cap_rows], X [cap_rows, n] out; returns the rows (0: all runs ended),
 *            -1 for a NULL argument, -2 where cap_rows is too small
 *   feed     nrows must be what pending returned
 *   result   x [S, n], fun [S], grad [S, n], hess [S, n, n] (nullable: H at x), mu [S],
 *            nit, nfev (rows), status [S] (0 converged, 1 maxiter, 2 no decrease can be
 *            found / a bad first row), rounds (nullable); RVS_E_ARG while runs live */
void *rvs_lm_begin(int S, int n, const double *x0, double gtol, double xtol, double tau,
                   double mu_max, int maxiter);
int64_t rvs_lm_pending(void *h, int64_t *idx, double *X, int64_t cap_rows);
int rvs_lm_feed(void *h, const double *F, int64_t nrows);
int rvs_lm_result(void *h, double *x, double *fun, double *grad, double *hess,
                  double *mu, int32_t *nit, int32_t *nfev, int32_t *status,
                  int64_t *rounds);
void rvs_lm_end(void *h);

/* The same runs with their rounds on the device: a round is advance (one thread per
 * run: the scaled Cholesky factor and the two triangular solves) -> scan -> emit (the
 * kernels of rvs_bfgs_run_grad) -> per chunk of g->cap rows the gradient chain with
 * rvs_chisq_point_fisher and rvs_proc_finish_fisher as its last two calls; the host
 * looks at the counters as rvs_bfgs_run does.
 *   runs      S * rvs_lm_run_bytes() bytes of device memory (8-byte aligned)
 *   x0 [S, n] start points (device)
 *   x, grad [S, n], fun, mu [S], hess [S, n, n] (nullable), nit / nfev / status [S]:
 *             results, as rvs_lm_result's
 *   nreq, off, list [S]; X [S, n]; F [S, 1 + n + n (n + 1) / 2]; counts [32]: work
 *             arrays (list zero-filled by the caller)
 *   gtol, xtol, tau, mu_max, maxiter as for rvs_lm_begin
 * `o`, `g` as for rvs_bfgs_run_grad (g->njev is not written), `fc` the Fisher buffers
 * for g->cap rows.  n = o->n <= 8, ndim <= 6, S <= 24 g->cap.  stats as for
 * rvs_bfgs_run. */
typedef struct rvs_lm_state {
  void *runs;
  const double *x0;
  double *x, *fun, *grad, *hess, *mu;
  int32_t *nit, *nfev, *status;
  int32_t *nreq, *off, *list, *counts;
  double *X, *F;
  double gtol, xtol, tau, mu_max;
  int32_t S, n, maxiter, reserved_;
} rvs_lm_state;
int64_t rvs_lm_run_bytes(void);
int rvs_lm_run(const rvs_lm_state *b, const rvs_nm_objective *o,
               const rvs_grad_chain *g, const rvs_fisher_chain *fc, int sync_every,
               int64_t *stats, void *stream);
/* rvs_lm_run with the rows' (value, gradient, Fisher matrix) from ONE rvs_objective_fisher
 * call per chunk of g->cap rows, between rvs_proc_map and rvs_proc_finish_fisher, in the
 * place of rvs_lm_run's chain (rvs_template_polylinear_grad -> rvs_vsini_convolve(_grad)
 * -> rvs_spline_construct -> rvs_chisq_point_fisher): the polish of vel_fit.py:653-658
 * as rvs_bfgs_run_grad_fused runs it, on Levenberg-Marquardt steps.  The same machine
 * (lm_machine.h), rounds, counts and results as rvs_lm_run.  Of g only cap, narm, ntan,
 * vsini_mode, chi [cap] and grad [cap, 1 + ntan] are read; garms / basis_const as for
 * rvs_objective_fisher.  fwork: g->cap * (1 + ntan)^2 doubles (the chunk's matrices)
 * followed by rvs_objective_fisher's work buffer -- fwork_bytes at least those matrices
 * plus rvs_objective_fisher_work_size(1, narm, ntan, npix_max); more than the size for
 * cap jobs is of no use.  RVS_E_ARG: what rvs_lm_run or rvs_objective_fisher refuse. */
int rvs_lm_run_fused(const rvs_lm_state *b, const rvs_nm_objective *o,
                     const rvs_grad_chain *g, const rvs_objective_arm *garms,
                     const double *basis_const, void *fwork, int64_t fwork_bytes,
                     int sync_every, int64_t *stats, void *stream);

/* ------------------------------------------------------------------------
 * The joint fit of a star's epochs (vel_fit.process_epochs): one set of stellar
 * parameters (and one vsini) per star, one velocity per epoch.  Epochs are rows of one
 * batch sorted by star: star n of a call owns the epochs eoff[n] .. eoff[n + 1] - 1
 * (eoff device int32 [N + 1], eoff[0] = 0, S = eoff[N] epochs in all).  Its optimiser
 * vector is z = (theta [m], v [E]): theta in the columns of the fitted parameters
 * without the velocity -- [vsini,] free stellar parameters -- velocities in km/s.  The two kernels take
 * m <= 6 (ntan <= 6, the limit of the gradient chain); the host machines m <= 7.
 *
 * rvs_epoch_map is the counterpart of rvs_proc_map: theta [N, m] and velin [S] -> per
 * star star_id[n] = list[n] (the row of fixed / vsini_fixed / safe / prior_mean /
 * prior_isig [., ndim]), vsini [N] (nullable: no rotation), params [N, ndim], extra [N]
 * (the priors plus the vsini clamp penalty, counted ONCE per star) and bad [N] (a
 * non-finite parameter, or ANY epoch's velocity outside [min_vel, max_vel]; the star's
 * parameters are then `safe` and its velocities 0); per epoch vel [S] and, where
 * job_templ is not NULL, job_templ[e] = n, the star's row (rvs_chisq_point_fisher's
 * job_templ).  src [ndim] (HOST): column of THETA feeding library parameter i or -1;
 * vsini_col: column of theta or -1.  The statements per parameter are rvs_proc_map's.
 *
 * rvs_epoch_finish turns the per-epoch rows of rvs_chisq_point_fisher -- chi [S],
 * grad [S, K], fisher [S, K, K], K = 1 + ntan, computed with job_templ = the star's row
 * -- into the star's arrow row at F + rowoff[n] (rowoff device int64 [N]):
 *   f, g_theta [m], Htt packed (lower triangle row-major, m (m + 1) / 2),
 *   then per epoch (g_e, h_e, c_e [m])
 * rvs_alm_row_size(m, E) = 1 + m + m (m + 1) / 2 + E (2 + m) doubles (0 for m outside
 * 1 .. 7 or E < 1).  f = sum_e chi_e + extra; g_theta, Htt from the sums over the star's
 * epochs of grad and fisher, taken in epoch order as additions only, then mapped entry by
 * entry as rvs_proc_finish_fisher maps them (factor 2 on the finished sum of the Fisher
 * matrices, + 2 isig^2 and 2 (p - mean) isig^2 of a prior, the vsini column zeroed
 * outside (0, max_vsini), the clamp penalty's 2 (x - clamp) and + 2); g_e = d/dv_e,
 * h_e = 2 fisher_e[0, 0], c_e[i] = 2 fisher_e[row of theta_i, 0].  A bad star's row is
 * 1e30 followed by zeros.  Status bits of the epochs of the live stars (n <
 * counts[cidx], or all when counts == NULL) are OR-ed into star_status[star_id[n]].  One
 * wave per star, no float atomics, no FMA contraction: tests/epochs_truth.py gives the
 * same bits.  RVS_E_ARG: a NULL array, m > 7, ndim > 6, ntan > 6 (so m <= 6),
 * ntan != ndim + (vsini_col >= 0), a src entry that is vsini_col or >= m, columns of
 * theta without exactly one source. */
int rvs_epoch_map(int N, int S, int m, int ndim, const double *theta,
                  const double *velin, const int32_t *eoff, const int32_t *list,
                  const int32_t *src, int vsini_col, const double *fixed,
                  const double *vsini_fixed, const double *safe,
                  const double *prior_mean, const double *prior_isig, double min_vel,
                  double max_vel, double max_vsini, int32_t *star_id,
                  int32_t *job_templ, double *vel, double *vsini, double *params,
                  double *extra, int32_t *bad, void *stream);
int rvs_epoch_finish(int N, int m, int ndim, int ntan, const int32_t *counts, int cidx,
                     const int32_t *eoff, const int64_t *rowoff, const double *chi,
                     const double *grad, const double *fisher, const double *theta,
                     const double *params, const double *extra, const int32_t *bad,
                     const int32_t *star_id, const int32_t *job_status,
                     const int32_t *src, int vsini_col, const double *prior_mean,
                     const double *prior_isig, double max_vsini, double *F,
                     int32_t *star_status, void *stream);
int64_t rvs_alm_row_size(int m, int E);

/* Levenberg-Marquardt on the arrow rows, the machines on the host (csrc/alm_machine.h):
 * the algorithm of rvs_lm_* over z, the dense Cholesky replaced by the elimination of
 * the velocities (a Cholesky of the m x m Schur complement).  begin -> { pending -> the
 * caller's objective -> feed } -> result -> end, with ragged buffers: star s (E_s =
 * eoff[s + 1] - eoff[s] epochs, eoff HOST int32 [N + 1]) has its vector at
 * s m + eoff[s] (m + E_s entries) and its row at s (1 + m + m (m + 1) / 2) +
 * eoff[s] (2 + m).
 *   begin    x0 ragged [N m + S]; gtol, xtol, tau, mu_max, maxiter as rvs_lm_begin
 *            (maxiter <= 0: 200 (m + E_s)).  NULL for bad arguments, a star without
 *            epochs among them
 *   pending  idx [N], X [cap_values] out: the pending stars ascending and their vectors
 *            one behind the other; returns the stars (0: all runs ended), -1 for a NULL
 *            argument, -2 where cap_values is too small
 *   feed     F: the rows of those stars one behind the other; nstars must be what
 *            pending returned
 *   result   x, grad ragged as x0; row (nullable) ragged: the row at x; fun, mu, nit,
 *            nfev, status [N] and rounds as rvs_lm_result */
void *rvs_alm_begin(int N, int m, const int32_t *eoff, const double *x0, double gtol,
                    double xtol, double tau, double mu_max, int maxiter);
int64_t rvs_alm_pending(void *h, int64_t *idx, double *X, int64_t cap_values);
int rvs_alm_feed(void *h, const double *F, int64_t nstars);
int rvs_alm_result(void *h, double *x, double *fun, double *grad, double *row,
                   double *mu, int32_t *nit, int32_t *nfev, int32_t *status,
                   int64_t *rounds);
void rvs_alm_end(void *h);

/* The same runs with their rounds inside the library: rvs_alm_run.  A round is
 *   advance  one thread per star (csrc/alm_machine.h, the source of rvs_alm_begin): the
 *            reply of the last request -> the run -> the vector it asks for next
 *   look     nreq [N] is read by the host, which lays the pending stars out in chunks of
 *            whole stars (at most cap_star stars and cap_epoch epochs each) and uploads a
 *            chunk's tables (row offsets, local eoff, the star list, job_spec) in one copy
 *   chunk    emit (the stars' vectors -> theta, velin) -> rvs_epoch_map -> per arm the
 *            template / broadening / spline stage of rvs_bfgs_run_grad's chain over the
 *            chunk's STARS -> the epochs' penalties -> rvs_chisq_point_fisher (or
 *            _resol) with job_templ = the star's row -> rvs_epoch_finish into F
 * with no interpreter in between.  The rows are those of the same entry points called
 * from Python (optimizer.EpochChain.rows), so x, fun, nit, nfev and status are the bits
 * of rvs_alm_begin / _pending / _feed around them.
 *
 * rvs_epoch_chain: arms / point / basis_const HOST arrays [narm] as in rvs_grad_chain,
 * with the arm's templ, templ2, coef, outside, simplex, vs_rows, out_rows for cap_star
 * rows and its penalty for cap_epoch jobs; fisher_work:
 * rvs_chisq_point_fisher_work_size(cap_epoch, narm, ntan) bytes; chi [cap_epoch], grad
 * [cap_epoch, K], fisher [cap_epoch, K, K]; the mapping's tables per star (fixed,
 * vsini_fixed, safe, prior_mean, prior_isig: rows star 0 .. N - 1) and its buffers theta
 * [cap_star, m], vsini, extra [cap_star], params [cap_star, ndim], star_id, bad int32
 * [cap_star], velin, vel [cap_epoch], job_templ, jstatus int32 [cap_epoch]; status int32
 * [N] (OR-ed into).  The epochs are rows eoff[n] .. eoff[n + 1] - 1 of the arms' spectra.
 *
 * rvs_alm_state: runs N * rvs_alm_run_bytes() bytes; state 5 (N m + S) + S + (the rows'
 * total) doubles; eoff HOST and eoff_dev device int32 [N + 1]; x0, x, grad ragged [N m +
 * S]; row, F ragged (the rows' total; row nullable); fun, mu [N]; nit, nfev, status, nreq
 * int32 [N]; tab int32 [6 N + S + 16] (8-byte aligned); chi_x [S] (nullable; with it
 * chi_trial [S], a work array): out, the chi of every epoch at its star's x (untouched
 * for a star whose first row is bad).  gtol ... maxiter as
 * rvs_alm_begin.  stats (nullable) int64[3] = rounds, chunks evaluated, star rows.
 * RVS_E_ARG: a NULL array, m outside 1 .. 6, a star without epochs or with more than
 * cap_epoch. */
typedef struct rvs_epoch_chain {
  const rvs_grad_arm *arms;
  const rvs_point_arm *point;
  const double *basis_const;
  const double *pen_scale;
  void *fisher_work;
  double *chi, *grad, *fisher;
  const double *fixed, *vsini_fixed, *safe, *prior_mean, *prior_isig;
  double *theta, *vsini, *params, *extra, *velin, *vel;
  int32_t *star_id, *bad, *job_templ, *jstatus, *status;
  double min_vel, max_vel, max_vsini, badchi;
  int32_t narm, npoly, ntan, vsini_mode, m, ndim, vsini_col, cap_star, cap_epoch,
      reserved_;
  int32_t src[8];
} rvs_epoch_chain;
typedef struct rvs_alm_state {
  void *runs;
  double *state;
  const int32_t *eoff, *eoff_dev;
  const double *x0;
  double *x, *grad, *row, *fun, *mu, *F, *chi_trial, *chi_x;
  int32_t *nit, *nfev, *status, *nreq, *tab;
  double gtol, xtol, tau, mu_max;
  int32_t N, m, maxiter, reserved_;
} rvs_alm_state;
int64_t rvs_alm_run_bytes(void);
int rvs_alm_run(const rvs_alm_state *b, const rvs_epoch_chain *c, int64_t *stats,
                void *stream);

/* ------------------------------------------------------------------------
 * Template libraries from high-resolution models; replaces rvs_make_interpol's
 * per-model work: read_grid.make_rebinner (read_grid.py:360-466) without its sparse
 * matrix, apply_rebinner between the photon conversions of
 * make_interpol.extract_spectrum (make_interpol.py:152-154), and that function's
 * continuum, logarithm, finite check and cast (:156-172, :367-368).
 *
 * The band.  Output pixel i (centre lam[i], half steps as read_grid.py:409-416, LSF
 * sigma sigs[i] of :394-400) takes input pixels left[i] .. right[i] + 1: the segments
 * left[i] .. right[i] of :423-441, i.e. searchsorted(lam0, lam[i] -/+ 5 sigs[i])
 * (- 1 on the left) clamped to 0 and n0 - 2 -- found by the caller; the kernels clamp
 * again and never read outside lam0 [n0], hr [., n0] or W [npix, K].
 * W [npix, K] (row-major, K >= max_i right[i] - left[i] + 2): W[i, k] is the weight
 * of input pixel left[i] + k -- coeff1 of segment k plus coeff2 of segment k - 1 of
 * pix_integrator (:75-111), over leftstep + rightstep -- and 0 behind the window.
 * The weight is the integral over the output pixel of the Gaussian-convolved linear
 * interpolant; it is evaluated from the antiderivatives of Phi(u) and u Phi(u) with
 * erfc in the tails (csrc/rebin.hip), not from the reference's expression.
 * lam0 is the input grid AFTER the vacuum -> air conversion (:388-392, host work).
 * npix <= 65535. */
int rvs_rebin_weights(const double *lam0, int n0, const double *lam,
                      const double *sigs, const int32_t *left, const int32_t *right,
                      int npix, int K, double *W, void *stream);

/* photons != 0 (extract_spectrum: photons in, per wavelength out):
 *   out[t, i] = (1 / lam[i]) sum_k W[i, k] hr[t, left[i] + k] lam0[left[i] + k]
 * photons == 0 (apply_rebinner alone; lam0 and lam are not read):
 *   out[t, i] = sum_k W[i, k] hr[t, left[i] + k]
 * for T models: hr [T, n0] with row stride hr_stride >= n0 ELEMENTS, float32
 * (hr_f32 != 0; PHOENIX files) or float64; out float64 [T, npix]; sums in float64,
 * each in ascending input pixel whatever T is (the same bits for any split of the
 * models into calls).  T <= 32 * 65535 per call. */
int rvs_rebin_apply(const void *hr, int hr_f32, int64_t hr_stride, int T, int n0,
                    const double *lam0, const double *W, int K, const int32_t *left,
                    const int32_t *right, const double *lam, int npix, int photons,
                    double *out, void *stream);

/* rows float64 [T, npix] (rvs_rebin_apply's out) -> out [T, npix], float32
 * (float_bits 32) or float64 (64); one block per row.
 * mode RVS_NORM_LINEAR_CONTINUUM: get_line_continuum (make_interpol.py:47-75) divided
 *   out -- np.median of row[:npix // 2] and of row[npix // 2:], the straight line
 *   through (lam1, log) and (lam2, log) evaluated and extrapolated at every lam[i],
 *   exponentiated; lam1, lam2: the medians of the two halves of lam (host);
 * mode RVS_NORM_MEDIAN: divided by np.median(row), lognorms[t] = its log;
 * mode RVS_NORM_NONE.  lognorms [T] (nullable) is 0 in the other two modes.
 * Then log when log_spec != 0.  status[t] = RVS_ST_NONFINITE when a value of the row
 * is not finite (make_interpol.py:169-171 raises).  2 <= npix <= RVS_REBIN_MAX_NPIX,
 * which is RVS_CCF_MODEL_MAX_NTP: what this writes rvs_ccf_models_build accepts. */
#define RVS_REBIN_MAX_NPIX 9216
#define RVS_NORM_NONE 0
#define RVS_NORM_MEDIAN 1
#define RVS_NORM_LINEAR_CONTINUUM 2
int rvs_template_normalize(const double *rows, int T, int npix, const double *lam,
                           int mode, double lam1, double lam2, int log_spec,
                           int float_bits, void *out, double *lognorms,
                           int32_t *status, void *stream);

/* ------------------------------------------------------------------------
 * Filling the holes of a template grid; replaces the RBFInterpolator of
 * regularize_grid.converter (regularize_grid.py:118-140) and, for
 * kernel='multiquadric' (degree 0), scipy/interpolate/_rbfinterp.py:
 * _build_system + _build_and_solve_system (factor, solve) and _chunk_evaluator (eval).
 *
 *   K[i,j] = -sqrt(|eps y_i - eps y_j|^2 + 1),   (K + diag(smoothing)) c + 1 lam = d,
 *   1^T c = 0,   out[m,:] = sum_j -sqrt(|eps x_m - eps y_j|^2 + 1) c[j,:] + lam.
 *
 * y [N, ndim] nodes, d [N, S] values (float32 when d_f32 != 0, else float64; row
 * stride d_stride >= S ELEMENTS), x [M, ndim] points, out [M, S] (float32 / float64 by
 * float_bits; row stride out_stride >= S elements); smoothing [N] or NULL (zero).
 * All arithmetic is float64.  `work`: rvs_rbf_work_size(N, S) DOUBLES, the caller's.
 * rvs_rbf_factor fills its first part from the nodes alone; rvs_rbf_solve keeps the
 * coefficients of ONE set of S columns behind it and rvs_rbf_eval reads them -- the
 * columns are independent, so a caller short of memory factors once and walks d in
 * column chunks of S with solve + eval per chunk.
 * Route: blocked Cholesky of K + diag(smoothing) + a 1 1^T (a: the kernel of the nodes'
 * bounding box, >= max |K_ij|), c and lam from the extra right-hand side 1
 * (csrc/rbf.hip).  status (int32 [1], OR-ed into): RVS_ST_RBF_NOTPD when a pivot is
 * not finite and above 8 N DBL_EPSILON a (coincident nodes), RVS_ST_NONFINITE for non-finite nodes,
 * smoothing or values; the coefficients are then not to be used.
 * Limits (RVS_E_ARG beyond, before any launch): 1 <= N <= RVS_RBF_MAX_N (the factor is
 * N^2 doubles: 2 GiB there), 1 <= ndim <= 8, 1 <= S <= RVS_RBF_MAX_S,
 * 1 <= M <= RVS_RBF_MAX_M, 0 < eps < 1e300.  rvs_rbf_work_size returns RVS_E_ARG. */
#define RVS_RBF_MAX_N 16384
#define RVS_RBF_MAX_S 1048576
#define RVS_RBF_MAX_M 4194240
int64_t rvs_rbf_work_size(int N, int S);
int rvs_rbf_factor(const double *y, int N, int ndim, double eps,
                   const double *smoothing, double *work, int32_t *status,
                   void *stream);
int rvs_rbf_solve(const void *d, int d_f32, int64_t d_stride, int N, int S,
                  double *work, int32_t *status, void *stream);
int rvs_rbf_eval(const double *x, int M, const double *y, int N, int ndim, double eps,
                 const double *work, int S, int float_bits, void *out,
                 int64_t out_stride, void *stream);

/* ------------------------------------------------------------------------
 * Training of the MLP that rvs_template_nn evaluates; replaces the optimiser loop of
 * nn/train_interpolator.py:284-322 for NNInterpolator(withbn=False, SiLU)
 * (nn/NNInterpolator.py:14-91): per batch  R = model(x) SD_0 + D_0,
 * loss = mean|R - dat| / spread0, backward, torch.optim.Adam (betas 0.9 / 0.999,
 * eps 1e-8, no weight decay).  float32 throughout (f32-input MFMA, exact products);
 * every sum has a fixed order and no float atomics are used, so two runs from the same
 * state give the same bits (csrc/nn_train.hip).
 *
 *   dats [T, npix] float32: training rows; x [T, ndim] float32: the Mapper's output
 *   for them (nn/NNInterpolator.py:159-171); both stay where they are and are read by
 *   row index (indices are clamped to [0, T)).
 *   nlayer linear layers, dims int32 [nlayer + 1] (HOST; dims[0] = ndim, dims[nlayer] =
 *   npix): SiLU behind every layer but the last.  W, b, dW, db, mW, mb, vW, vb: HOST
 *   arrays of nlayer DEVICE pointers, W[l] [dims[l+1], dims[l]] row-major as
 *   rvs_template_nn, the others of the same shapes (m*, v*: Adam's moments).
 *   D0, SD0 float32 [npix] (train_interpolator.py:177-178), spread0 (:241).
 *   work: rvs_nn_train_work_size(T, B, nlayer, dims) BYTES of device memory, 256-byte
 *   aligned, the caller's (B: the largest batch it will be used with).
 * Limits (RVS_E_ARG beyond, before any launch): 1 <= ndim <= 8, 2 <= nlayer <= 8,
 * 1 <= hidden widths <= RVS_NN_TRAIN_MAX_WIDTH, 1 <= B <= RVS_NN_TRAIN_MAX_B,
 * 1 <= npix <= RVS_NN_TRAIN_MAX_NPIX (RVS_REBIN_MAX_NPIX), T >= 1, spread0 > 0;
 * rvs_nn_train_work_size returns RVS_E_ARG.
 *
 * rvs_nn_train_grad: forward and, when dW and db are not NULL, backward of ONE batch,
 * the rows[0 .. nrows) (device int32) of dats / x; updates nothing.  loss (device
 * double [1]) = mean|R - dat| / spread0; resid (nullable) float32 [nrows, npix] =
 * R - dat; dW[l], db[l] = the gradients of loss (what autograd gives).  With dW == db ==
 * NULL it is the evaluation loss of the rows (validation, train_interpolator.py:330-338).
 *
 * rvs_nn_adam_step: the update alone (torch/optim/adam.py: _single_tensor_adam) from
 * given gradients; step >= 1 is the count the bias correction uses.
 *
 * rvs_nn_train_epoch: the steps of one epoch (train_interpolator.py:315-322) on
 * `stream`, no host synchronisation: batch i is perm[i B .. min((i + 1) B, ntrain))
 * (device int32; the last one short as DataLoader(drop_last=False), its loss normalised
 * by its own size), step counts step0 + 1 ...  loss_accum (device double [1], ADDED
 * to) += sum_i loss_i rows_i npix (lossAccum, :322); step_loss (nullable, device
 * double [ceil(ntrain / B)]) = loss_i.  lr: the rate of this epoch. */
#define RVS_NN_TRAIN_MAX_B 1024
#define RVS_NN_TRAIN_MAX_WIDTH 1024
#define RVS_NN_TRAIN_MAX_NPIX 9216
int64_t rvs_nn_train_work_size(int T, int B, int nlayer, const int32_t *dims);
int rvs_nn_train_grad(const float *dats, const float *x, int T, const int32_t *rows,
                      int nrows, int nlayer, const int32_t *dims, const float *const *W,
                      const float *const *b, const float *D0, const float *SD0,
                      double spread0, float *const *dW, float *const *db, double *loss,
                      float *resid, void *work, void *stream);
int rvs_nn_adam_step(int nlayer, const int32_t *dims, float *const *W, float *const *b,
                     const float *const *dW, const float *const *db, float *const *mW,
                     float *const *mb, float *const *vW, float *const *vb, double lr,
                     int step, void *stream);
int rvs_nn_train_epoch(const float *dats, const float *x, int T, const int32_t *perm,
                       int ntrain, int B, int nlayer, const int32_t *dims, float *const *W,
                       float *const *b, float *const *mW, float *const *mb,
                       float *const *vW, float *const *vb, const float *D0,
                       const float *SD0, double spread0, double lr, int step0,
                       double *loss_accum, double *step_loss, void *work, void *stream);

#ifdef __cplusplus
}
#endif
#endif
