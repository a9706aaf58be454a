// lm_machine.h -- ONE run of the Levenberg-Marquardt polish of vel_fit.process
// (config['second_minimizer_lm']) as a resumable state machine, plain C++ for the host
// (lm_host.cpp: rvs_lm_begin / _pending / _feed) and for a kernel, one thread per
// spectrum (lm_dev.hip: rvs_lm_run) -- the form bfgs_machine.h has.
//
// A request is always ONE row, c.xt [n]; its reply is (f, g [n], H packed: the lower
// triangle row-major, n (n + 1) / 2 entries) = the row of rvs_proc_finish_fisher.
// advance(c, reply) runs until the next request (c.pending) or the end (c.done).
//
// The algorithm is Nielsen's damping with Marquardt's diagonal scaling, as stated in
// tests/refmachines/lm_restated.py with explicit loops in index order; this file follows
// it statement by statement, scalar arithmetic without FMA contraction, so that the two
// give the same bits:
//   1. request x0; a reply that is not finite or a bad row (f >= 1e30): status 2
//   2. max |g_i| <= gtol: status 0 (scipy BFGS's test)
//   3. d_i = 1 / sqrt(H_ii) where H_ii > 0, else 1; A = d H d + mu I; Cholesky; a
//      non-positive pivot counts as a rejected step
//   4. A y = -d g, delta = d y; |delta_i| <= xtol (|x_i| + xtol) for all i: the end,
//      status 0 after an accepted trial (or none), 2 after a rejected one
//   5. request x + delta; pred = 1/2 sum delta_i (mu delta_i / d_i^2 - g_i),
//      rho = (f - f_t) / pred
//   6. reply finite, pred > 0, rho > 0: accept, nit += 1,
//      mu *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; else mu *= nu, nu *= 2, and
//      mu > mu_max: status 2.  nit >= maxiter: status 1.
// nfev counts rows.  The state is 67 doubles and 7 ints, under 0.6 KB; the n <= 8 factor and
// the two work vectors are locals of advance() (52 doubles: in a kernel they are indexed
// by the run-time n and live in scratch memory -- DESIGN 4.17).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define LM_HD __host__ __device__
#else
#define LM_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rvs_lm {

constexpr int MAXN = 8;
constexpr int MAXT = MAXN * (MAXN + 1) / 2;
constexpr double TAU = 1e-3, XTOL = 1e-10, MU_MAX = 1e16;

struct Run {
  double x[MAXN], g[MAXN], xt[MAXN], H[MAXT];
  double f, mu, nu, pred;
  double gtol, xtol, mu_max;
  int n, phase, maxiter, nit, nfev, nrej, status;
  bool pending, rejected, done;
};

LM_HD inline int npack(int n) { return 1 + n + n * (n + 1) / 2; }

// gtol as for BFGS; xtol, tau, mu_max <= 0: the defaults; maxiter <= 0: 200 n
LM_HD inline void init(Run &c, int n, const double *x0, double gtol, double xtol,
                       double tau, double mu_max, int maxiter) {
  c.n = n;
  for (int i = 0; i < n; i++) c.x[i] = c.xt[i] = x0[i];
  for (int i = 0; i < n; i++) c.g[i] = 0;
  for (int q = 0; q < n * (n + 1) / 2; q++) c.H[q] = 0;
  c.f = 0;
  c.mu = tau > 0 ? tau : TAU;
  c.nu = 2.0;
  c.pred = 0;
  c.gtol = gtol;
  c.xtol = xtol > 0 ? xtol : XTOL;
  c.mu_max = mu_max > 0 ? mu_max : MU_MAX;
  c.maxiter = maxiter > 0 ? maxiter : 200 * n;
  c.nit = c.nfev = c.nrej = c.status = 0;
  c.phase = 0;
  c.pending = c.rejected = c.done = false;
}

LM_HD inline void end(Run &c, int status) {
  c.status = status;
  c.done = true;
  c.pending = false;
}

LM_HD inline bool finite_reply(const Run &c, const double *reply) {
  const int m = npack(c.n);
  for (int q = 0; q < m; q++)
    if (!std::isfinite(reply[q])) return false;
  return true;
}

LM_HD inline void take(Run &c, const double *reply) {
  const int n = c.n;
  c.f = reply[0];
  for (int i = 0; i < n; i++) c.g[i] = reply[1 + i];
  for (int q = 0; q < n * (n + 1) / 2; q++) c.H[q] = reply[1 + n + q];
}

// step 6, the reject branch; true where the run ended
LM_HD inline bool reject(Run &c) {
  c.nrej += 1;
  c.rejected = true;
  c.mu = c.mu * c.nu;
  c.nu = 2.0 * c.nu;
  if (c.mu > c.mu_max) {
    end(c, 2);
    return true;
  }
  if (c.nit >= c.maxiter) {
    end(c, 1);
    return true;
  }
  return false;
}

LM_HD inline void advance(Run &c, const double *reply) {
  const int n = c.n;
  if (c.phase == 0) {
    c.phase = 1;
    c.pending = true;
    return;
  }
  c.pending = false;
  c.nfev += 1;
  if (c.phase == 1) {
    c.f = reply[0];
    if (!finite_reply(c, reply) || reply[0] >= 1e30) {
      end(c, 2);
      return;
    }
    take(c, reply);
    c.phase = 2;
  } else {
    const double ft = reply[0];
    bool ok = finite_reply(c, reply) && c.pred > 0;
    double rho = 0.0;
    if (ok) {
      rho = (c.f - ft) / c.pred;
      ok = rho > 0;
    }
    if (ok) {
      for (int i = 0; i < n; i++) c.x[i] = c.xt[i];
      take(c, reply);
      c.nit += 1;
      double t = 2.0 * rho - 1.0;
      t = 1.0 - t * t * t;
      const double third = 1.0 / 3.0;
      c.mu = c.mu * (third > t ? third : t);
      c.nu = 2.0;
      c.rejected = false;
      if (c.nit >= c.maxiter) {
        end(c, 1);
        return;
      }
    } else if (reject(c)) {
      return;
    }
  }
  double d[MAXN], y[MAXN], L[MAXT];
  while (true) {
    // 2
    double gmax = 0.0;
    for (int i = 0; i < n; i++) {
      const double a = std::fabs(c.g[i]);
      if (a > gmax) gmax = a;
    }
    if (gmax <= c.gtol) {
      end(c, 0);
      return;
    }
    // 3
    for (int i = 0; i < n; i++) {
      const double hii = c.H[i * (i + 1) / 2 + i];
      d[i] = hii > 0 ? 1.0 / std::sqrt(hii) : 1.0;
    }
    bool posdef = true;
    for (int i = 0; i < n && posdef; i++) {
      for (int j = 0; j <= i; j++) {
        double s = (d[i] * c.H[i * (i + 1) / 2 + j]) * d[j];
        if (i == j) s = s + c.mu;
        for (int k = 0; k < j; k++)
          s = s - L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
        if (i == j) {
          if (!(s > 0)) {
            posdef = false;
            break;
          }
          L[i * (i + 1) / 2 + i] = std::sqrt(s);
        } else {
          L[i * (i + 1) / 2 + j] = s / L[j * (j + 1) / 2 + j];
        }
      }
    }
    if (!posdef) {
      if (reject(c)) return;
      continue;
    }
    // 4: L z = -d g, L^T y = z
    for (int i = 0; i < n; i++) {
      double s = -(d[i] * c.g[i]);
      for (int k = 0; k < i; k++) s = s - L[i * (i + 1) / 2 + k] * y[k];
      y[i] = s / L[i * (i + 1) / 2 + i];
    }
    for (int i = n - 1; i >= 0; i--) {
      double s = y[i];
      for (int k = i + 1; k < n; k++) s = s - L[k * (k + 1) / 2 + i] * y[k];
      y[i] = s / L[i * (i + 1) / 2 + i];
    }
    bool small = true;
    double pred = 0.0;
    for (int i = 0; i < n; i++) {
      const double delta = d[i] * y[i];
      if (!(std::fabs(delta) <= c.xtol * (std::fabs(c.x[i]) + c.xtol))) small = false;
      // 5 (mu delta_i / d_i^2 = mu y_i / d_i)
      pred = pred + delta * (c.mu * y[i] / d[i] - c.g[i]);
      c.xt[i] = c.x[i] + delta;
    }
    if (small) {
      end(c, c.rejected ? 2 : 0);
      return;
    }
    c.pred = 0.5 * pred;
    c.pending = true;
    return;
  }
}

// H at x as a full symmetric [n, n]
LM_HD inline void unpack_hess(const Run &c, double *out) {
  const int n = c.n;
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++)
      out[i * n + j] = out[j * n + i] = c.H[i * (i + 1) / 2 + j];
}

}  // namespace rvs_lm
