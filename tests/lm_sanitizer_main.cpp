// Drives rvs_lm_begin ... rvs_lm_end (csrc/lm_host.cpp) on the Rosenbrock residuals
// (case (a) of tests/test_lm_cpu.py, n = 2 and the chained n = 6) and on the log barrier
// with an underestimated curvature (case (c): the first trial lands outside, value
// +inf); built for the host with -fsanitize=address,undefined by tests/test_lm_cpu.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>
extern "C" {
void *rvs_lm_begin(int S, int n, const double *x0, double gtol, double xtol, double tau, double mu_max, int maxiter);
int64_t rvs_lm_pending(void *h, int64_t *idx, double *X, int64_t cap_rows);
int rvs_lm_feed(void *h, const double *F, int64_t nrows);
int rvs_lm_result(void *h, double *x, double *fun, double *grad, double *hess, double *mu, int32_t *nit, int32_t *nfev, int32_t *status, int64_t *rounds);
void rvs_lm_end(void *h);
}

// f = |r|^2, g = 2 J^T r, H = 2 J^T J of r = (10 (x_{i+1} - x_i^2), 1 - x_i)
static void rosen_row(int n, const double *x, double *F) {
  const int m = 2 * (n - 1);
  std::vector<double> r(m), J(m * n, 0.0);
  for (int i = 0; i < n - 1; i++) {
    r[2 * i] = 10 * (x[i + 1] - x[i] * x[i]);
    J[2 * i * n + i + 1] = 10;
    J[2 * i * n + i] = -20 * x[i];
    r[2 * i + 1] = 1 - x[i];
    J[(2 * i + 1) * n + i] = -1;
  }
  double f = 0;
  for (int k = 0; k < m; k++) f += r[k] * r[k];
  F[0] = f;
  for (int a = 0; a < n; a++) {
    double g = 0;
    for (int k = 0; k < m; k++) g += J[k * n + a] * r[k];
    F[1 + a] = 2 * g;
    for (int b = 0; b <= a; b++) {
      double h = 0;
      for (int k = 0; k < m; k++) h += J[k * n + a] * J[k * n + b];
      F[1 + n + a * (a + 1) / 2 + b] = 2 * h;
    }
  }
}

static void barrier_row(int n, const double *x, double *F) {
  const int w = 1 + n + n * (n + 1) / 2;
  for (int q = 0; q < w; q++) F[q] = 0;
  for (int i = 0; i < n; i++)
    if (x[i] >= 1) {
      F[0] = std::numeric_limits<double>::infinity();
      return;
    }
  for (int i = 0; i < n; i++) {
    F[0] += 0.5 * (x[i] + 2) * (x[i] + 2) - std::log(1 - x[i]);
    F[1 + i] = (x[i] + 2) + 1 / (1 - x[i]);
    F[1 + n + i * (i + 1) / 2 + i] = 0.1 * (1 + 1 / ((1 - x[i]) * (1 - x[i])));
  }
}

static int drive(const char *name, int S, int n, void (*row)(int, const double *, double *),
                 const std::vector<double> &x0, double gtol, double want, double tol) {
  const int w = 1 + n + n * (n + 1) / 2;
  void *h = rvs_lm_begin(S, n, x0.data(), gtol, 0, 0, 0, 0);
  if (!h) return 1;
  std::vector<int64_t> idx(S);
  std::vector<double> X(S * n), F(S * w);
  int64_t rows;
  while ((rows = rvs_lm_pending(h, idx.data(), X.data(), S)) > 0) {
    for (int64_t r = 0; r < rows; r++) row(n, &X[r * n], &F[r * w]);
    if (rvs_lm_feed(h, F.data(), rows + 1) == 0) return 5;   // the wrong count is refused
    if (rvs_lm_feed(h, F.data(), rows)) return 2;
  }
  if (rows < 0) return 6;
  std::vector<double> x(S * n), fun(S), g(S * n), H(S * n * n), mu(S);
  std::vector<int32_t> nit(S), nfev(S), st(S);
  int64_t rounds;
  if (rvs_lm_result(h, x.data(), fun.data(), g.data(), H.data(), mu.data(), nit.data(), nfev.data(), st.data(), &rounds)) return 3;
  rvs_lm_end(h);
  int nmax = 0, nconv = 0;
  double dev = 0;
  for (int s = 0; s < S; s++) {
    if (nit[s] > nmax) nmax = nit[s];
    if (st[s] == 0) nconv++;
    for (int i = 0; i < n; i++) dev = std::fmax(dev, std::fabs(x[s * n + i] - want));
  }
  printf("%s n %d rounds %lld max nit %d converged %d of %d max |x - min| %.3g\n", name, n, (long long)rounds, nmax, nconv, S, dev);
  return (nconv == S && dev < tol) ? 0 : 7;
}

int main() {
  int rc;
  for (int n : {2, 6}) {
    const int S = 40;
    std::vector<double> x0(S * n);
    // (the chain has a second minimum near x_0 = -1: its starts stay beside (1, ..., 1))
    for (int i = 0; i < S * n; i++) x0[i] = n == 2 ? std::sin(0.37 * i) * 2 : 1 + 0.3 * std::sin(0.37 * i);
    if ((rc = drive("rosenbrock", S, n, rosen_row, x0, 1e-8, 1.0, 1e-6))) return rc;
  }
  {
    const int S = 40, n = 3;
    std::vector<double> x0(S * n);
    for (int s = 0; s < S; s++)
      for (int i = 0; i < n; i++) x0[s * n + i] = -3.0 - 0.05 * s;
    if ((rc = drive("barrier", S, n, barrier_row, x0, 1e-5, -0.5 * (1 + std::sqrt(13.0)), 1e-5))) return rc;
  }
  return 0;
}
