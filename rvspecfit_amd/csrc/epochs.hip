// epochs.hip -- the joint fit of a star's epochs (vel_fit.process_epochs): one set of
// stellar parameters (and one vsini) per star, one velocity per epoch.
//
// Epochs are rows of one SpecBatch sorted by star: star n owns the epochs
// eoff[n] .. eoff[n + 1] - 1.  Its optimiser vector is z = (theta [m], v [E]), theta in
// the columns of ParamMapper.get_fitted_params() without 'vel'.
//
//   rvs_epoch_map     theta [N, m], v [S] -> per star params, vsini, prior / vsini
//                     penalty (ONCE per star), bad; per epoch vel and the star's row
//                     (job_templ of rvs_chisq_point_fisher): rvs_proc_map's statements
//   rvs_epoch_finish  chi [S], grad [S, K], fisher [S, K, K] of the epochs, computed with
//                     job_templ = the star's row -> the star's arrow row
//                       f, g_theta [m], Htt packed [m (m + 1) / 2],
//                       then per epoch (g_e, h_e, c_e [m])
//                     behind a row-offset table: proc_finish_kernel<true>'s mapping per
//                     entry (bfgs_grad.hip), the sums over a star's epochs in epoch order
//
// Without FMA contraction: tests/epochs_truth.py states both in numpy and the kernels
// give its bits.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int EP_MAXM = 7;
constexpr int EP_SPW = 4;   // stars (waves) per block of the finish kernel

struct EpP {
  int m, ndim, ntan, vsini_col;
  int src[8];   // column of theta feeding library parameter i, or -1 = fixed
  int tan[8];   // column of theta -> its row of grad / fisher
  const double *prior_mean, *prior_isig;
  double max_vsini;
};

// the tables of both entry points from the host's src [ndim] (columns of THETA);
// false for what rvs_proc_finish_grad refuses
bool ep_tables(EpP &P, int m, int ndim, int ntan, const int32_t *src, int vsini_col,
               const double *prior_mean, const double *prior_isig, double max_vsini) {
  if (m < 1 || m > EP_MAXM || ndim < 1 || ndim > 6 || !src || vsini_col >= m ||
      (prior_mean && !prior_isig))
    return false;
  // (K K + K + 1 lanes of the finish kernel: K = 1 + ntan <= 7, as chain_ok has it)
  if (ntan != ndim + (vsini_col >= 0 ? 1 : 0) || ntan > 6) return false;
  P.m = m, P.ndim = ndim, P.ntan = ntan, P.vsini_col = vsini_col;
  int ncol = vsini_col >= 0 ? 1 : 0;
  bool seen[8] = {false, false, false, false, false, false, false, false};
  for (int i = 0; i < 8; i++) P.tan[i] = 0;
  for (int i = 0; i < 8; i++) {
    P.src[i] = (i < ndim) ? src[i] : -1;
    if (P.src[i] >= m || (P.src[i] >= 0 && P.src[i] == vsini_col)) return false;
    if (P.src[i] >= 0) {
      if (seen[P.src[i]]) return false;
      seen[P.src[i]] = true;
      ncol++;
      P.tan[P.src[i]] = 1 + i;
    }
  }
  if (ncol != m) return false;   // every column of theta has exactly one source
  if (vsini_col >= 0) P.tan[vsini_col] = ntan;
  P.prior_mean = prior_mean, P.prior_isig = prior_isig;
  P.max_vsini = max_vsini;
  return true;
}

// one thread per star: map_row_regs' statements (nm.hip) for the star's parameters, the
// velocity guard over its epochs
__global__ void __launch_bounds__(256)
    epoch_map_kernel(int N, EpP P, const double *__restrict__ theta,
                     const double *__restrict__ velin, const int32_t *__restrict__ eoff,
                     const int32_t *__restrict__ list, const double *__restrict__ fixed,
                     const double *__restrict__ vsini_fixed,
                     const double *__restrict__ safe, double min_vel, double max_vel,
                     int32_t *__restrict__ star_id, int32_t *__restrict__ job_templ,
                     double *__restrict__ vel, double *__restrict__ vsini,
                     double *__restrict__ params, double *__restrict__ extra,
                     int32_t *__restrict__ bad) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const int m = P.m, ndim = P.ndim;
  const int r = list[n];
  const int e0 = eoff[n], e1 = eoff[n + 1];
  const double *x = theta + (int64_t)n * m;
  double pen = 0;
  if (vsini) {
    double vs;
    if (P.vsini_col >= 0) {
      const double v0 = x[P.vsini_col];
      vs = fmin(fmax(v0, 0.0), P.max_vsini);  // np.clip
      if (v0 < 0 || v0 > P.max_vsini) pen += (vs - v0) * (vs - v0);
      if (v0 != v0) vs = v0;
    } else {
      vs = vsini_fixed[r];
    }
    vsini[n] = vs;
  }
  bool isbad = false;
  for (int e = e0; e < e1; e++) {
    const double v = velin[e];
    if ((v > max_vel) || (v < min_vel)) isbad = true;
  }
  double p[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    p[i] = 0;
    if (i >= ndim) continue;
    p[i] = (P.src[i] >= 0) ? x[P.src[i]] : fixed[(int64_t)r * ndim + i];
    if (!(fabs(p[i]) <= 1.79e308)) isbad = true;
  }
  if (isbad) {
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (i < ndim) p[i] = safe[(int64_t)r * ndim + i];
  }
  if (P.prior_mean) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      if (i >= ndim) continue;
      const double d = (P.prior_mean[(int64_t)r * ndim + i] - p[i]) *
                       P.prior_isig[(int64_t)r * ndim + i];
      pen += d * d;
    }
  }
  star_id[n] = r;
#pragma unroll
  for (int i = 0; i < 8; i++)
    if (i < ndim) params[(int64_t)n * ndim + i] = p[i];
  extra[n] = pen;
  bad[n] = isbad ? 1 : 0;
  for (int e = e0; e < e1; e++) {
    vel[e] = isbad ? 0.0 : velin[e];
    if (job_templ) job_templ[e] = n;
  }
}

// one wave per star.  Lane q < K K owns entry q of the K x K sum of the Fisher matrices,
// the next K lanes the sum of the gradients, one more the sum of chi: each walks the
// star's epochs in index order (a wave reads fisher[e] contiguously), additions only.  The
// sums meet in LDS; the lanes then write the head of the row (f, g_theta, Htt: at most
// 1 + 7 + 28 = 36 entries) and stride over the per-epoch records.
__global__ void __launch_bounds__(64 * EP_SPW)
    epoch_finish_kernel(int N, const int32_t *__restrict__ counts, int cidx, EpP P,
                        const int32_t *__restrict__ eoff,
                        const int64_t *__restrict__ rowoff,
                        const double *__restrict__ chi, const double *__restrict__ grad,
                        const double *__restrict__ fisher,
                        const double *__restrict__ theta,
                        const double *__restrict__ params,
                        const double *__restrict__ extra,
                        const int32_t *__restrict__ bad,
                        const int32_t *__restrict__ star_id,
                        const int32_t *__restrict__ job_status, double *__restrict__ F,
                        int32_t *__restrict__ star_status) {
  __shared__ double sm[EP_SPW][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.x * EP_SPW + wave;
  const bool act = n < N;
  const int m = P.m, K = 1 + P.ntan, KK = K * K;
  const int e0 = act ? eoff[n] : 0, E = act ? eoff[n + 1] - e0 : 0;
  const int isbad = act ? bad[n] : 1;
  double s = 0.0;
  if (!isbad && E > 0) {
    const double *base = nullptr;
    int stride = 0;
    if (lane < KK) {
      base = fisher + (int64_t)e0 * KK + lane, stride = KK;
    } else if (lane < KK + K) {
      base = grad + (int64_t)e0 * K + (lane - KK), stride = K;
    } else if (lane == KK + K) {
      base = chi + e0, stride = 1;
    }
    if (base) {
      s = base[0];
      for (int e = 1; e < E; e++) s += base[(int64_t)e * stride];
    }
  }
  sm[wave][lane] = s;
  __syncthreads();
  if (!act) return;
  const int head = 1 + m + m * (m + 1) / 2, w = 2 + m;
  double *f = F + rowoff[n];
  if (isbad) {
    const int64_t width = head + (int64_t)E * w;
    for (int64_t q = lane; q < width; q += 64) f[q] = (q == 0) ? 1e30 : 0.0;
    return;
  }
  const double *sum = sm[wave];
  const int r = star_id[n];
  bool inside = true, beyond = false;
  double x = 0, cl = 0;
  if (P.vsini_col >= 0) {
    x = theta[(int64_t)n * m + P.vsini_col];
    cl = fmin(fmax(x, 0.0), P.max_vsini);
    inside = (0 < x) && (x < P.max_vsini);
    beyond = (x < 0) || (x > P.max_vsini);
  }
  if (lane == 0) {
    f[0] = sum[KK + K] + extra[n];
  } else if (lane <= m) {
    const int i = lane - 1, t = P.tan[i];
    double v = sum[KK + t];
    if (i == P.vsini_col) {
      v = (inside ? v : 0.0) + 2.0 * (x - cl);
    } else if (P.prior_mean) {
      const double is = P.prior_isig[(int64_t)r * P.ndim + (t - 1)];
      if (is != 0)
        v += 2.0 * (params[(int64_t)n * P.ndim + (t - 1)] -
                    P.prior_mean[(int64_t)r * P.ndim + (t - 1)]) * is * is;
    }
    f[lane] = v;
  } else if (lane < head) {
    const int q = lane - 1 - m;
    int a = 0;
    while ((a + 1) * (a + 2) / 2 <= q) a++;
    const int b = q - a * (a + 1) / 2;
    double v = 2.0 * sum[P.tan[a] * K + P.tan[b]];
    if ((a == P.vsini_col || b == P.vsini_col) && !inside) v = 0.0;
    if (a == b) {
      if (a == P.vsini_col) {
        if (beyond) v += 2.0;
      } else if (P.prior_mean) {
        const double is = P.prior_isig[(int64_t)r * P.ndim + (P.tan[a] - 1)];
        if (is != 0) v += 2.0 * (is * is);
      }
    }
    f[lane] = v;
  }
  // the epochs' records: (g_e, h_e, c_e [m]) = d/dv, 2 F_vv, 2 F_(theta_i, v)
  for (int t = lane; t < E * w; t += 64) {
    const int e = t / w, k = t - e * w;
    const double *fm = fisher + (int64_t)(e0 + e) * KK;
    double v;
    if (k == 0) {
      v = grad[(int64_t)(e0 + e) * K];
    } else if (k == 1) {
      v = 2.0 * fm[0];
    } else {
      v = 2.0 * fm[P.tan[k - 2] * K];
      if (k - 2 == P.vsini_col && !inside) v = 0.0;
    }
    f[head + t] = v;
  }
  int st = 0;
  for (int e = lane; e < E; e += 64) st |= job_status[e0 + e];
  const int live = counts ? counts[cidx] : N;
  if (n < live && st) atomicOr(&star_status[r], st);
}

}  // namespace

extern "C" int rvs_epoch_map(int N, int S, int m, int ndim, const double *theta,
                             const double *velin, const int32_t *eoff,
                             const int32_t *list, const int32_t *src, int vsini_col,
                             const double *fixed, const double *vsini_fixed,
                             const double *safe, const double *prior_mean,
                             const double *prior_isig, double min_vel, double max_vel,
                             double max_vsini, int32_t *star_id, int32_t *job_templ,
                             double *vel, double *vsini, double *params, double *extra,
                             int32_t *bad, void *stream) {
  EpP P;
  if (N < 1 || S < N || !theta || !velin || !eoff || !list || !fixed || !safe ||
      !star_id || !vel || !params || !extra || !bad ||
      (vsini && vsini_col < 0 && !vsini_fixed) || (!vsini && vsini_col >= 0) ||
      !ep_tables(P, m, ndim, ndim + (vsini_col >= 0 ? 1 : 0), src, vsini_col,
                 prior_mean, prior_isig, max_vsini))
    return RVS_E_ARG;
  hipLaunchKernelGGL(epoch_map_kernel, dim3((N + 255) / 256), dim3(256), 0,
                     rvs_stream(stream), N, P, theta, velin, eoff, list, fixed,
                     vsini_fixed, safe, min_vel, max_vel, star_id, job_templ, vel, vsini,
                     params, extra, bad);
  RVS_LAUNCH_CHECK();
  return 0;
}

extern "C" int rvs_epoch_finish(int N, int m, int ndim, int ntan, const int32_t *counts,
                                int cidx, const int32_t *eoff, const int64_t *rowoff,
                                const double *chi, const double *grad,
                                const double *fisher, const double *theta,
                                const double *params, const double *extra,
                                const int32_t *bad, const int32_t *star_id,
                                const int32_t *job_status, const int32_t *src,
                                int vsini_col, const double *prior_mean,
                                const double *prior_isig, double max_vsini, double *F,
                                int32_t *star_status, void *stream) {
  EpP P;
  if (N < 1 || !eoff || !rowoff || !chi || !grad || !fisher || !theta || !params ||
      !extra || !bad || !star_id || !job_status || !F || !star_status ||
      !ep_tables(P, m, ndim, ntan, src, vsini_col, prior_mean, prior_isig, max_vsini))
    return RVS_E_ARG;
  hipLaunchKernelGGL(epoch_finish_kernel, dim3((N + EP_SPW - 1) / EP_SPW),
                     dim3(64 * EP_SPW), 0, rvs_stream(stream), N, counts, cidx, P, eoff,
                     rowoff, chi, grad, fisher, theta, params, extra, bad, star_id,
                     job_status, F, star_status);
  RVS_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------
// rvs_alm_run: the rounds of the joint fit inside the library.  N runs of alm_machine.h
// -- the machine alm_host.cpp drives -- live in HBM, one thread per star advances its
// run; the host reads nreq [N] once per round, lays the pending stars out in chunks of
// whole stars and launches, per chunk, the joint chain from C.
// ---------------------------------------------------------------------------
#include <vector>

#include "alm_machine.h"

#ifndef ALM_NT
#define ALM_NT 16   // runs per block, as LM_NT (lm_dev.hip): each run's path is its own
#endif

namespace {

using rvs_alm::Run;

struct AlmDev {
  Run *runs;
  double *state;
  const int32_t *eoff;
  const double *x0;
  double *F;
  int32_t *nreq;
  double *chi_trial, *chi_x;   // per epoch: chi of the last request / at x (nullable)
  double gtol, xtol, tau, mu_max;
  int N, m, maxiter;
};

__device__ inline int64_t alm_xoff(const AlmDev &D, int s) {
  return (int64_t)s * D.m + D.eoff[s];
}
__device__ inline int64_t alm_roff(const AlmDev &D, int s) {
  return (int64_t)s * (1 + D.m + D.m * (D.m + 1) / 2) + (int64_t)D.eoff[s] * (2 + D.m);
}

__global__ void __launch_bounds__(ALM_NT) alm_advance_kernel(AlmDev D, int first) {
  const int s = blockIdx.x * ALM_NT + threadIdx.x;
  if (s >= D.N) return;
  Run &r = D.runs[s];
  if (first) {
    const int E = D.eoff[s + 1] - D.eoff[s];
    // (a run's state: 5 (m + E) + E + row_size doubles, one behind the other)
    double *buf = D.state + 5 * alm_xoff(D, s) + D.eoff[s] + alm_roff(D, s);
    rvs_alm::init(r, D.m, E, buf, D.x0 + alm_xoff(D, s), D.gtol, D.xtol, D.tau,
                  D.mu_max, D.maxiter);
    rvs_alm::advance(r, nullptr);
  } else {
    if (!D.nreq[s]) return;
    const int phase = r.phase, nit = r.nit;
    rvs_alm::advance(r, D.F + alm_roff(D, s));
    // the request became the current point (the first row taken, or a trial accepted):
    // its epochs' chi are those at x
    if (D.chi_x && ((phase == 1 && r.phase == 2) || r.nit > nit))
      for (int e = D.eoff[s]; e < D.eoff[s + 1]; e++) D.chi_x[e] = D.chi_trial[e];
  }
  D.nreq[s] = (!r.done && r.pending) ? 1 : 0;
}

// the vectors the chunk's stars ask for -> theta [n, m], velin (the chunk's epochs)
__global__ void __launch_bounds__(256)
    alm_emit_kernel(int n, int m, const Run *__restrict__ runs,
                    const int32_t *__restrict__ list, const int32_t *__restrict__ leoff,
                    double *__restrict__ theta, double *__restrict__ velin) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const Run &r = runs[list[j]];
  for (int i = 0; i < m; i++) theta[(int64_t)j * m + i] = r.xt[i];
  const int e0 = leoff[j], E = leoff[j + 1] - e0;
  for (int e = 0; e < E; e++) velin[e0 + e] = r.xt[m + e];
}

// penalty of an epoch = outside[its star's row] * badchi of its spectrum
__global__ void __launch_bounds__(256)
    epoch_penalty_kernel(int S, const double *__restrict__ outside,
                         const int32_t *__restrict__ job_templ,
                         const double *__restrict__ pen_scale,
                         const int32_t *__restrict__ job_spec, double badchi,
                         double *__restrict__ pen) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= S) return;
  const double b = pen_scale ? pen_scale[job_spec[e]] * badchi : badchi;
  pen[e] = outside[job_templ[e]] * b;
}

// chi of a chunk's epochs -> their places among all epochs
__global__ void __launch_bounds__(256)
    epoch_scatter_kernel(int S, const double *__restrict__ chi,
                         const int32_t *__restrict__ job_spec, double *__restrict__ out) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e < S) out[job_spec[e]] = chi[e];
}

__global__ void __launch_bounds__(256)
    epoch_repeat_kernel(int J, int R, const double *__restrict__ vsini,
                        const double *__restrict__ outside, double *__restrict__ vs_rows,
                        double *__restrict__ out_rows) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= J * R) return;
  vs_rows[t] = vsini[t / R];
  out_rows[t] = outside[t / R];
}

__global__ void __launch_bounds__(ALM_NT)
    alm_result_kernel(AlmDev D, double *x, double *fun, double *grad, double *row,
                      double *mu, int32_t *nit, int32_t *nfev, int32_t *status) {
  const int s = blockIdx.x * ALM_NT + threadIdx.x;
  if (s >= D.N) return;
  const Run &r = D.runs[s];
  const int n = r.m + r.E;
  const int64_t xo = alm_xoff(D, s);
  for (int i = 0; i < n; i++) {
    x[xo + i] = r.x[i];
    grad[xo + i] = r.g[i];
  }
  if (row) {
    const int64_t ro = alm_roff(D, s), w = rvs_alm::row_size(r.m, r.E);
    for (int64_t q = 0; q < w; q++) row[ro + q] = r.row[q];
  }
  fun[s] = r.f;
  mu[s] = r.mu;
  nit[s] = r.nit;
  nfev[s] = r.nfev;
  status[s] = r.done ? r.status : -1;
}

int epoch_chain_ok(const rvs_epoch_chain *c) {
  if (!c || !c->arms || !c->point || !c->basis_const || !c->fisher_work || !c->chi ||
      !c->grad || !c->fisher || !c->fixed || !c->safe || !c->theta || !c->params ||
      !c->extra || !c->velin || !c->vel || !c->star_id || !c->bad || !c->job_templ ||
      !c->jstatus || !c->status || c->narm < 1 || c->narm > RVS_MAX_ARMS ||
      c->cap_star < 1 || c->cap_epoch < 1 || c->vsini_mode < 0 || c->vsini_mode > 2 ||
      c->ndim < 1 || c->ndim > 6 || c->m < 1 || c->m > 6 || c->ntan > 6 ||
      c->ntan != c->ndim + (c->vsini_mode == 2 ? 1 : 0) ||
      (c->vsini_mode == 2) != (c->vsini_col >= 0) ||
      (c->vsini_mode != 0) != (c->vsini != nullptr) ||
      (c->vsini_mode == 1 && !c->vsini_fixed))
    return 0;
  for (int a = 0; a < c->narm; a++) {
    const rvs_grad_arm &A = c->arms[a];
    if (!A.dats || !A.knots || !A.templ || !A.coef || !A.outside || !A.penalty ||
        A.ntp < 3 || A.ntp != c->point[a].ntp || !(A.lnstep > 0) ||
        c->point[a].coef != A.coef || c->point[a].penalty != A.penalty)
      return 0;
    if (A.tri == 2) {
      const rvs_nm_nn_arm *N = static_cast<const rvs_nm_nn_arm *>(A.dats);
      if (!N->M || !N->S || !N->W || !N->b || !N->dims || !N->act0 || !N->act1 ||
          N->nlayer < 3)
        return 0;
    } else if (A.tri ? (!A.transform || !A.extraflags || !A.simplices || !A.simplex ||
                        A.nsimplex < 1)
                     : (!A.idgrid || !A.uvecs || !A.vecs_s || !A.lens || !A.ptp ||
                        A.ngrid < 1))
      return 0;
    if (c->vsini_mode != 0 && !A.templ2) return 0;
    if (c->vsini_mode == 1 && (!A.vs_rows || !A.out_rows)) return 0;
  }
  return 1;
}

// the joint chain for one chunk: n stars (theta, velin emitted already), S epochs
int epoch_chain_eval(const rvs_epoch_chain *c, int n, int S, const int32_t *list,
                     const int32_t *leoff, const int64_t *rowoff,
                     const int32_t *job_spec, double *F, hipStream_t st) {
  const int ndim = c->ndim, ntan = c->ntan;
  int rc = rvs_epoch_map(n, S, c->m, ndim, c->theta, c->velin, leoff, list, c->src,
                         c->vsini_col, c->fixed, c->vsini_fixed, c->safe, c->prior_mean,
                         c->prior_isig, c->min_vel, c->max_vel, c->max_vsini, c->star_id,
                         c->job_templ, c->vel, c->vsini, c->params, c->extra, c->bad, st);
  if (rc) return rc;
  // the template, broadening and spline stage over the chunk's STARS: the arm loop of
  // rvs_bfgs_run_grad's chain (bfgs_grad.hip), the same entry points and arguments
  const int R = 1 + ndim;
  for (int a = 0; a < c->narm; a++) {
    const rvs_grad_arm &A = c->arms[a];
    if (A.tri == 2) {
      const rvs_nm_nn_arm *N = static_cast<const rvs_nm_nn_arm *>(A.dats);
      rc = rvs_template_nn_grad(c->params, n, ndim, N->log_mask, N->M, N->S, N->nlayer,
                                N->W, N->b, N->dims, N->act0, N->act1, A.templ, st);
      if (rc) return rc;
      rc = rvs_nn_outside(N->xeqs ? c->params : nullptr, n, ndim, N->log_mask, N->M,
                          N->S, N->xeqs ? 0 : 1, N->xeqs, N->nfx, N->yeqs, N->nfy,
                          A.outside, st);
    } else if (!A.tri)
      rc = rvs_template_polylinear_grad(
          static_cast<const float *>(A.dats), A.ngrid, A.ntp, A.idgrid, A.uvecs, A.lens,
          ndim, A.vecs_s, A.ptp, A.log_mask, A.exp_flag, c->params, n, A.templ,
          A.outside, nullptr, nullptr, st);
    else if (A.buckets.cell_start)
      rc = rvs_template_tri_buckets_grad(
          static_cast<const double *>(A.dats), A.ntp, A.simplices, A.transform,
          A.extraflags, A.nsimplex, ndim, A.log_mask, A.exp_flag, &A.buckets, c->params,
          n, A.templ, A.outside, A.simplex, nullptr, st);
    else
      rc = rvs_template_tri_grad(static_cast<const double *>(A.dats), A.ntp,
                                 A.simplices, A.transform, A.extraflags, A.nsimplex,
                                 ndim, A.log_mask, A.exp_flag, c->params, n, A.templ,
                                 A.outside, A.simplex, nullptr, st);
    if (rc) return rc;
    const double *rows = A.templ;
    if (c->vsini_mode == 2) {
      rc = rvs_vsini_convolve_grad(A.templ, c->vsini, A.outside, A.lnstep, 0.6, A.ntp, R,
                                   n, A.templ2, st);
      if (rc) return rc;
      rows = A.templ2;
    } else if (c->vsini_mode == 1) {
      hipLaunchKernelGGL(epoch_repeat_kernel, dim3((n * R + 255) / 256), dim3(256), 0, st,
                         n, R, c->vsini, A.outside, A.vs_rows, A.out_rows);
      RVS_LAUNCH_CHECK();
      rc = rvs_vsini_convolve(A.templ, A.vs_rows, A.out_rows, A.lnstep, 0.6, A.ntp,
                              n * R, A.templ2, st);
      if (rc) return rc;
      rows = A.templ2;
    }
    rc = rvs_spline_construct(A.knots, rows, A.ntp, n * (1 + ntan), A.spline_form,
                              A.factors, A.coef, st);
    if (rc) return rc;
    hipLaunchKernelGGL(epoch_penalty_kernel, dim3((S + 255) / 256), dim3(256), 0, st, S,
                       A.outside, c->job_templ, c->pen_scale, job_spec, c->badchi,
                       A.penalty);
    RVS_LAUNCH_CHECK();
  }
  if (hipMemsetAsync(c->jstatus, 0, sizeof(int32_t) * S, st) != hipSuccess)
    return RVS_E_LAUNCH;
  bool resol = false;
  for (int a = 0; a < c->narm; a++) resol = resol || c->point[a].taps;
  rc = (resol ? rvs_chisq_point_fisher_resol : rvs_chisq_point_fisher)(
      c->point, c->narm, c->npoly, ntan, job_spec, c->job_templ, S, c->vel, c->badchi,
      c->basis_const, c->fisher_work, c->chi, c->grad, c->fisher, c->jstatus, st);
  if (rc) return rc;
  return rvs_epoch_finish(n, c->m, ndim, ntan, nullptr, 0, leoff, rowoff, c->chi, c->grad,
                          c->fisher, c->theta, c->params, c->extra, c->bad, c->star_id,
                          c->jstatus, c->src, c->vsini_col, c->prior_mean, c->prior_isig,
                          c->max_vsini, F, c->status, st);
}

}  // namespace

extern "C" int64_t rvs_alm_run_bytes(void) { return (int64_t)sizeof(Run); }

extern "C" int rvs_alm_run(const rvs_alm_state *b, const rvs_epoch_chain *c,
                           int64_t *stats, void *stream) {
  if (!b || !c || b->N < 1 || b->m < 1 || b->m > 6 || b->m != c->m || !b->runs ||
      !b->state || !b->eoff || !b->eoff_dev || !b->x0 || !b->x || !b->grad || !b->fun ||
      !b->mu || !b->F || !b->nit || !b->nfev || !b->status || !b->nreq || !b->tab ||
      b->eoff[0] != 0 || (b->chi_x && !b->chi_trial) || !epoch_chain_ok(c))
    return RVS_E_ARG;
  const int N = b->N, m = b->m;
  for (int s = 0; s < N; s++) {
    const int E = b->eoff[s + 1] - b->eoff[s];
    if (E < 1 || E > c->cap_epoch) return RVS_E_ARG;
  }
  const int64_t S = b->eoff[N], head = 1 + m + m * (m + 1) / 2;
  const int64_t tab_len = 6 * (int64_t)N + S + 16;
  hipStream_t st = rvs_stream(stream);
  AlmDev D;
  D.runs = static_cast<Run *>(b->runs);
  D.state = b->state, D.eoff = b->eoff_dev, D.x0 = b->x0, D.F = b->F, D.nreq = b->nreq;
  D.chi_trial = b->chi_trial, D.chi_x = b->chi_x;
  D.gtol = b->gtol, D.xtol = b->xtol, D.tau = b->tau, D.mu_max = b->mu_max;
  D.N = N, D.m = m, D.maxiter = b->maxiter;
  const dim3 agrid((N + ALM_NT - 1) / ALM_NT);
  hipLaunchKernelGGL(alm_advance_kernel, agrid, dim3(ALM_NT), 0, st, D, 1);
  RVS_LAUNCH_CHECK();
  std::vector<int32_t> nreq(N);
  std::vector<std::vector<int32_t>> tabs;   // a round's tables stay until its look
  int64_t rounds = 0, calls = 0, rows = 0;
  while (true) {
    if (hipMemcpyAsync(nreq.data(), b->nreq, sizeof(int32_t) * N, hipMemcpyDeviceToHost,
                       st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return RVS_E_LAUNCH;
    tabs.clear();
    int64_t at = 0;   // int32 entries of b->tab used by this round's chunks (even)
    int s = 0;
    bool any = false;
    while (true) {
      // the next chunk: pending stars in order, whole stars, both capacities
      std::vector<int32_t> ids;
      int64_t ne = 0;
      for (; s < N; s++) {
        if (!nreq[s]) continue;
        const int E = b->eoff[s + 1] - b->eoff[s];
        if ((int)ids.size() >= c->cap_star || ne + E > c->cap_epoch) break;
        ids.push_back(s);
        ne += E;
      }
      if (ids.empty()) break;
      any = true;
      const int n = (int)ids.size();
      // [rowoff int64 [n] | leoff [n + 1] | list [n] | job_spec [ne] | pad]
      const int64_t len = 2 * (int64_t)n + (n + 1) + n + ne;
      const int64_t padded = len + (len & 1);
      if (at + padded > tab_len) return RVS_E_ARG;
      tabs.emplace_back((size_t)padded, 0);
      std::vector<int32_t> &T = tabs.back();
      int64_t *ro = reinterpret_cast<int64_t *>(T.data());
      int32_t *leoff = T.data() + 2 * n, *list = leoff + n + 1, *spec = list + n;
      leoff[0] = 0;
      for (int j = 0; j < n; j++) {
        const int q = ids[j], E = b->eoff[q + 1] - b->eoff[q];
        ro[j] = (int64_t)q * head + (int64_t)b->eoff[q] * (2 + m);
        list[j] = q;
        for (int e = 0; e < E; e++) spec[leoff[j] + e] = b->eoff[q] + e;
        leoff[j + 1] = leoff[j] + E;
      }
      int32_t *dT = b->tab + at;
      if (hipMemcpyAsync(dT, T.data(), sizeof(int32_t) * padded, hipMemcpyHostToDevice,
                         st) != hipSuccess)
        return RVS_E_LAUNCH;
      const int32_t *d_leoff = dT + 2 * n, *d_list = d_leoff + n + 1,
                    *d_spec = d_list + n;
      hipLaunchKernelGGL(alm_emit_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, m,
                         D.runs, d_list, d_leoff, c->theta, c->velin);
      RVS_LAUNCH_CHECK();
      int rc = epoch_chain_eval(c, n, (int)ne, d_list, d_leoff,
                                reinterpret_cast<const int64_t *>(dT), d_spec, b->F, st);
      if (rc) return rc;
      if (b->chi_x) {
        hipLaunchKernelGGL(epoch_scatter_kernel, dim3(((int)ne + 255) / 256), dim3(256), 0,
                           st, (int)ne, c->chi, d_spec, b->chi_trial);
        RVS_LAUNCH_CHECK();
      }
      at += padded;
      calls++;
      rows += n;
    }
    if (!any) break;
    hipLaunchKernelGGL(alm_advance_kernel, agrid, dim3(ALM_NT), 0, st, D, 0);
    RVS_LAUNCH_CHECK();
    rounds++;
  }
  hipLaunchKernelGGL(alm_result_kernel, agrid, dim3(ALM_NT), 0, st, D, b->x, b->fun,
                     b->grad, b->row, b->mu, b->nit, b->nfev, b->status);
  RVS_LAUNCH_CHECK();
  if (hipStreamSynchronize(st) != hipSuccess) return RVS_E_LAUNCH;
  if (stats) {
    stats[0] = rounds;
    stats[1] = calls;
    stats[2] = rows;
  }
  return 0;
}
