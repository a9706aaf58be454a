// alm_host.cpp -- host side of the joint fit of a star's epochs (vel_fit.process_epochs):
// N runs of alm_machine.h advance in lock-step, the driver gathers the one pending vector
// of every live run into ONE ragged batch for the caller's objective (the arrow rows of
// optimizer.EpochChain.rows) and resumes the runs with the replies.  The shape of the
// rvs_lm_* family (lm_host.cpp), with ragged buffers: star s has E_s = eoff[s + 1] -
// eoff[s] epochs, its vector lies at s m + eoff[s] and has m + E_s entries, its row lies
// at s (1 + m + m (m + 1) / 2) + eoff[s] (2 + m).  This driver is what the CPU suite
// holds against tests/refmachines/lm_arrow_restated.py.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rvsgpu.h"
#include "alm_machine.h"

namespace {

using rvs_alm::Run;

struct Driver {
  int N, m;
  std::vector<int32_t> eoff;
  std::vector<Run> runs;
  std::vector<std::vector<double>> bufs;
  std::vector<int> order;  // runs with a pending request, ascending
  int64_t rounds = 0;
  int64_t xoff(int s) const { return (int64_t)s * m + eoff[s]; }
  int64_t roff(int s) const {
    return (int64_t)s * (1 + m + m * (m + 1) / 2) + (int64_t)eoff[s] * (2 + m);
  }
};

}  // namespace

extern "C" {

int64_t rvs_alm_row_size(int m, int E) {
  if (m < 1 || m > rvs_alm::MAXM || E < 1) return 0;
  return rvs_alm::row_size(m, E);
}

void *rvs_alm_begin(int N, int m, const int32_t *eoff, const double *x0, double gtol,
                    double xtol, double tau, double mu_max, int maxiter) {
  if (N < 1 || m < 1 || m > rvs_alm::MAXM || !eoff || !x0 || eoff[0] != 0)
    return nullptr;
  for (int s = 0; s < N; s++)
    if (eoff[s + 1] <= eoff[s]) return nullptr;   // a star without epochs
  Driver *d = new Driver;
  d->N = N;
  d->m = m;
  d->eoff.assign(eoff, eoff + N + 1);
  d->runs.resize(N);
  d->bufs.resize(N);
  for (int s = 0; s < N; s++) {
    const int E = eoff[s + 1] - eoff[s];
    d->bufs[s].assign(rvs_alm::state_size(m, E), 0.0);
    Run &r = d->runs[s];
    rvs_alm::init(r, m, E, d->bufs[s].data(), x0 + d->xoff(s), gtol, xtol, tau, mu_max,
                  maxiter);
    rvs_alm::advance(r, nullptr);  // to the first request (x0)
  }
  return d;
}

int64_t rvs_alm_pending(void *h, int64_t *idx, double *X, int64_t cap_values) {
  Driver *d = static_cast<Driver *>(h);
  if (!d || !idx || !X) return -1;
  d->order.clear();
  int64_t at = 0;
  for (int s = 0; s < d->N; s++) {
    const Run &r = d->runs[s];
    if (r.done || !r.pending) continue;
    const int n = r.m + r.E;
    if (at + n > cap_values) {
      d->order.clear();
      return -2;
    }
    idx[d->order.size()] = s;
    std::memcpy(X + at, r.xt, sizeof(double) * n);
    at += n;
    d->order.push_back(s);
  }
  return (int64_t)d->order.size();
}

int rvs_alm_feed(void *h, const double *F, int64_t nstars) {
  Driver *d = static_cast<Driver *>(h);
  if (!d || !F || nstars != (int64_t)d->order.size()) return RVS_E_ARG;
  int64_t at = 0;
  for (int s : d->order) {
    Run &r = d->runs[s];
    rvs_alm::advance(r, F + at);
    at += rvs_alm::row_size(r.m, r.E);
  }
  d->rounds += 1;
  d->order.clear();
  return 0;
}

int rvs_alm_result(void *h, double *x, double *fun, double *grad, double *row,
                   double *mu, int32_t *nit, int32_t *nfev, int32_t *status,
                   int64_t *rounds) {
  Driver *d = static_cast<Driver *>(h);
  if (!d || !x || !fun || !grad || !mu || !nit || !nfev || !status) return RVS_E_ARG;
  for (int s = 0; s < d->N; s++)
    if (!d->runs[s].done) return RVS_E_ARG;
  for (int s = 0; s < d->N; s++) {
    const Run &r = d->runs[s];
    const int n = r.m + r.E;
    std::memcpy(x + d->xoff(s), r.x, sizeof(double) * n);
    std::memcpy(grad + d->xoff(s), r.g, sizeof(double) * n);
    fun[s] = r.f;
    mu[s] = r.mu;
    nit[s] = r.nit;
    nfev[s] = r.nfev;
    status[s] = r.status;
    if (row)
      std::memcpy(row + d->roff(s), r.row, sizeof(double) * rvs_alm::row_size(r.m, r.E));
  }
  if (rounds) *rounds = d->rounds;
  return 0;
}

void rvs_alm_end(void *h) {
  Driver *d = static_cast<Driver *>(h);
  if (!d) return;
  delete d;
}

}  // extern "C"
