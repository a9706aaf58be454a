// lm_host.cpp -- host side of the Levenberg-Marquardt polish of vel_fit.process
// (config['second_minimizer_lm']): S runs of lm_machine.h advance in lock-step, the
// driver gathers the one pending row of every live run into ONE batch for the caller's
// objective and resumes the runs with the replies (f, g, packed H).  The shape of the
// rvs_bfgs_*_jac family (bfgs_host.cpp).  The same machine runs in a kernel
// (lm_dev.hip: rvs_lm_run); this driver serves a Python objective, is what the CPU
// suite holds against tests/refmachines/lm_restated.py, and is what rvs_lm_run is held
// against on the device.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rvsgpu.h"
#include "lm_machine.h"

namespace {

using rvs_lm::Run;

struct Driver {
  int S, n;
  std::vector<Run> runs;
  std::vector<int> order;  // runs with a pending request, ascending
  int64_t rounds = 0;
};

}  // namespace

extern "C" {

void *rvs_lm_begin(int S, int n, const double *x0, double gtol, double xtol,
                   double tau, double mu_max, int maxiter) {
  if (S < 1 || n < 1 || n > rvs_lm::MAXN || !x0) return nullptr;
  Driver *d = new Driver;
  d->S = S;
  d->n = n;
  d->runs.resize(S);
  for (int s = 0; s < S; s++) {
    Run &r = d->runs[s];
    rvs_lm::init(r, n, x0 + (int64_t)s * n, gtol, xtol, tau, mu_max, maxiter);
    rvs_lm::advance(r, nullptr);  // to the first request (x0)
  }
  return d;
}

int64_t rvs_lm_pending(void *h, int64_t *idx, double *X, int64_t cap_rows) {
  Driver *d = static_cast<Driver *>(h);
  if (!d || !idx || !X) return -1;
  d->order.clear();
  int64_t rows = 0;
  const int n = d->n;
  for (int s = 0; s < d->S; s++) {
    const Run &r = d->runs[s];
    if (r.done || !r.pending) continue;
    if (rows + 1 > cap_rows) return -2;
    idx[rows] = s;
    std::memcpy(X + rows * n, r.xt, sizeof(double) * n);
    rows += 1;
    d->order.push_back(s);
  }
  return rows;
}

int rvs_lm_feed(void *h, const double *F, int64_t nrows) {
  Driver *d = static_cast<Driver *>(h);
  if (!d || !F || nrows != (int64_t)d->order.size()) return RVS_E_ARG;
  const int m = rvs_lm::npack(d->n);
  int64_t at = 0;
  for (int s : d->order) {
    rvs_lm::advance(d->runs[s], F + at * m);
    at += 1;
  }
  d->rounds += 1;
  d->order.clear();
  return 0;
}

int rvs_lm_result(void *h, double *x, double *fun, double *grad, double *hess,
                  double *mu, int32_t *nit, int32_t *nfev, int32_t *status,
                  int64_t *rounds) {
  Driver *d = static_cast<Driver *>(h);
  if (!d || !x || !fun || !grad || !mu || !nit || !nfev || !status) return RVS_E_ARG;
  const int n = d->n;
  for (int s = 0; s < d->S; s++)
    if (!d->runs[s].done) return RVS_E_ARG;
  for (int s = 0; s < d->S; s++) {
    const Run &r = d->runs[s];
    std::memcpy(x + (int64_t)s * n, r.x, sizeof(double) * n);
    std::memcpy(grad + (int64_t)s * n, r.g, sizeof(double) * n);
    fun[s] = r.f;
    mu[s] = r.mu;
    nit[s] = r.nit;
    nfev[s] = r.nfev;
    status[s] = r.status;
    if (hess) rvs_lm::unpack_hess(r, hess + (int64_t)s * n * n);
  }
  if (rounds) *rounds = d->rounds;
  return 0;
}

void rvs_lm_end(void *h) {
  Driver *d = static_cast<Driver *>(h);
  if (!d) return;
  delete d;
}

}  // extern "C"
