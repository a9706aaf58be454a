// alm_machine.h -- ONE run of the joint Levenberg-Marquardt fit of a star's epochs
// (vel_fit.process_epochs) as a resumable state machine, plain C++ for the host
// (alm_host.cpp: rvs_alm_begin / _pending / _feed) and for a kernel, one thread per star
// (epochs.hip: rvs_alm_run) -- the form lm_machine.h has, over an arrowhead
// Gauss-Newton matrix.
//
// A star has m <= 7 shared parameters theta (the device chain that makes the rows takes
// m <= 6) and E epochs with one velocity each; its
// vector is z = (theta [m], v [E]), n = m + E.  A request is always ONE vector, c.xt [n];
// its reply is the arrow row of rvs_epoch_finish:
//   f, g_theta [m], Htt packed (lower triangle row-major, m (m + 1) / 2),
//   then per epoch (g_e, h_e, c_e [m])
// of rvs_alm_row_size(m, E) = 1 + m + m (m + 1) / 2 + E (2 + m) doubles.
// advance(c, reply) runs until the next request (c.pending) or the end (c.done).
//
// The algorithm is lm_machine.h's, steps 1 - 6 of its header (Nielsen's damping,
// Marquardt's scaling, the same constants and status codes), over z, with the dense
// Cholesky of step 3 replaced by the elimination of the velocities, as stated in
// tests/refmachines/lm_arrow_restated.py with explicit loops in index order; this file
// follows it statement by statement, scalar arithmetic without FMA contraction, so that
// the two give the same bits:
//   3. d_i = 1 / sqrt(Htt_ii) where positive, else 1; d_e = 1 / sqrt(h_e) where positive,
//      else 1;  a_e = (d_e h_e) d_e + mu;  b_e[i] = (d_e c_e[i]) d_i;
//      S_ij = (d_i Htt_ij) d_j + mu delta_ij - sum_e b_e[i] b_e[j] / a_e;  Cholesky of S;
//      a_e <= 0 or a non-positive pivot counts as a rejected step
//   4. rhs_i = -d_i g_i + sum_e b_e[i] (d_e g_e) / a_e;  S y_theta = rhs;
//      y_e = (-d_e g_e - b_e . y_theta) / a_e;  delta = d y
// with the gradient test, the xtol test and pred over all m + E entries, theta first.
// The state is ragged: the caller owns x, g, xt, d, y [n], a [E] and row [row_size] and
// hands their addresses to init(); b_e[i] is recomputed where it is used (three
// multiplications of the same operands give the same bits each time), so the work per
// round is O(E m^2) without an E x m buffer.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define ALM_HD __host__ __device__
#else
#define ALM_HD
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace rvs_alm {

constexpr int MAXM = 7;
constexpr int MAXT = MAXM * (MAXM + 1) / 2;
constexpr double TAU = 1e-3, XTOL = 1e-10, MU_MAX = 1e16;

struct Run {
  double *x, *g, *xt, *d, *y;   // [n]
  double *a;                    // [E]
  double *row;                  // [row_size(m, E)]: the reply at x
  double f, mu, nu, pred;
  double gtol, xtol, mu_max;
  int m, E, phase, maxiter, nit, nfev, nrej, status;
  bool pending, rejected, done;
};

ALM_HD inline int64_t row_size(int m, int E) {
  return 1 + m + m * (m + 1) / 2 + (int64_t)E * (2 + m);
}
// doubles of one run's ragged state behind a Run: x, g, xt, d, y [n], a [E], the row
ALM_HD inline int64_t state_size(int m, int E) {
  return 5 * (int64_t)(m + E) + E + row_size(m, E);
}

// `buf`: state_size(m, E) doubles of the caller's.  gtol as for BFGS; xtol, tau,
// mu_max <= 0: the defaults; maxiter <= 0: 200 n
ALM_HD inline void init(Run &c, int m, int E, double *buf, const double *x0, double gtol,
                        double xtol, double tau, double mu_max, int maxiter) {
  const int n = m + E;
  c.m = m, c.E = E;
  c.x = buf, c.g = buf + n, c.xt = buf + 2 * n, c.d = buf + 3 * n, c.y = buf + 4 * n;
  c.a = buf + 5 * n;
  c.row = buf + 5 * n + E;
  for (int i = 0; i < n; i++) c.x[i] = c.xt[i] = x0[i];
  for (int i = 0; i < n; i++) c.g[i] = c.d[i] = c.y[i] = 0;
  for (int e = 0; e < E; e++) c.a[e] = 0;
  for (int64_t q = 0; q < row_size(m, E); q++) c.row[q] = 0;
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

ALM_HD inline void end(Run &c, int status) {
  c.status = status;
  c.done = true;
  c.pending = false;
}

ALM_HD inline bool finite_reply(const Run &c, const double *reply) {
  const int64_t w = row_size(c.m, c.E);
  for (int64_t q = 0; q < w; q++)
    if (!std::isfinite(reply[q])) return false;
  return true;
}

ALM_HD inline void take(Run &c, const double *reply) {
  const int m = c.m, E = c.E;
  const int64_t w = row_size(m, E);
  for (int64_t q = 0; q < w; q++) c.row[q] = reply[q];
  c.f = reply[0];
  for (int i = 0; i < m; i++) c.g[i] = reply[1 + i];
  const int E0 = 1 + m + m * (m + 1) / 2;
  for (int e = 0; e < E; e++) c.g[m + e] = reply[E0 + (int64_t)e * (2 + m)];
}

// step 6, the reject branch; true where the run ended
ALM_HD inline bool reject(Run &c) {
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

// steps 3 and 4 on c.row with c.mu: c.d, c.y; false where a_e <= 0 or a pivot of the
// Schur complement is not positive
ALM_HD inline bool arrow_step(Run &c) {
  const int m = c.m, E = c.E;
  const int H0 = 1 + m, E0 = H0 + m * (m + 1) / 2, w = 2 + m;
  const double *row = c.row;
  double *d = c.d, *y = c.y, *a = c.a;
  double L[MAXT];
  for (int i = 0; i < m; i++) {
    const double hii = row[H0 + i * (i + 1) / 2 + i];
    d[i] = hii > 0 ? 1.0 / std::sqrt(hii) : 1.0;
  }
  for (int e = 0; e < E; e++) {
    const double he = row[E0 + (int64_t)e * w + 1];
    d[m + e] = he > 0 ? 1.0 / std::sqrt(he) : 1.0;
    a[e] = (d[m + e] * he) * d[m + e] + c.mu;
    if (!(a[e] > 0)) return false;
  }
#define ALM_B(e, i) ((d[m + (e)] * row[E0 + (int64_t)(e) * w + 2 + (i)]) * d[(i)])
  for (int i = 0; i < m; i++) {
    for (int j = 0; j <= i; j++) {
      double s = (d[i] * row[H0 + i * (i + 1) / 2 + j]) * d[j];
      if (i == j) s = s + c.mu;
      for (int e = 0; e < E; e++) {
        const double bi = ALM_B(e, i), bj = ALM_B(e, j);
        s = s - bi * bj / a[e];
      }
      for (int k = 0; k < j; k++)
        s = s - L[i * (i + 1) / 2 + k] * L[j * (j + 1) / 2 + k];
      if (i == j) {
        if (!(s > 0)) return false;
        L[i * (i + 1) / 2 + i] = std::sqrt(s);
      } else {
        L[i * (i + 1) / 2 + j] = s / L[j * (j + 1) / 2 + j];
      }
    }
  }
  // 4: L z = rhs, L^T y_theta = z
  for (int i = 0; i < m; i++) {
    double s = -(d[i] * row[1 + i]);
    for (int e = 0; e < E; e++) {
      const double bi = ALM_B(e, i);
      const double dg = d[m + e] * row[E0 + (int64_t)e * w];
      s = s + bi * dg / a[e];
    }
    for (int k = 0; k < i; k++) s = s - L[i * (i + 1) / 2 + k] * y[k];
    y[i] = s / L[i * (i + 1) / 2 + i];
  }
  for (int i = m - 1; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < m; k++) s = s - L[k * (k + 1) / 2 + i] * y[k];
    y[i] = s / L[i * (i + 1) / 2 + i];
  }
  for (int e = 0; e < E; e++) {
    double s = -(d[m + e] * row[E0 + (int64_t)e * w]);
    for (int i = 0; i < m; i++) {
      const double bi = ALM_B(e, i);
      s = s - bi * y[i];
    }
    y[m + e] = s / a[e];
  }
#undef ALM_B
  return true;
}

ALM_HD inline void advance(Run &c, const double *reply) {
  const int n = c.m + c.E;
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
    // 3, 4
    if (!arrow_step(c)) {
      if (reject(c)) return;
      continue;
    }
    bool small = true;
    double pred = 0.0;
    for (int i = 0; i < n; i++) {
      const double delta = c.d[i] * c.y[i];
      if (!(std::fabs(delta) <= c.xtol * (std::fabs(c.x[i]) + c.xtol))) small = false;
      // 5 (mu delta_i / d_i^2 = mu y_i / d_i)
      pred = pred + delta * (c.mu * c.y[i] / c.d[i] - c.g[i]);
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

}  // namespace rvs_alm
