// Drives rvs_bfgs_begin_jac ... rvs_bfgs_end (csrc/bfgs_host.cpp) on 200 quadratics
// with their exact gradients; built for the host with -fsanitize=address,undefined by
// tests/test_bfgs_jac_cpu.py.  Every seventh run gets a gradient that is 1e-3 off, so
// that the precision-loss exit and the line_search_wolfe2 fall-back run too.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>
extern "C" {
void *rvs_bfgs_begin_jac(int S, int n, const double *x0, const double *hess_inv0, double gtol, double c1, double c2, double xrtol, int maxiter);
int64_t rvs_bfgs_pending(void *h, int64_t *idx, double *X, int64_t cap_rows);
int rvs_bfgs_feed(void *h, const double *F, int64_t nrows);
int rvs_bfgs_feed_jac(void *h, const double *F, int64_t nrows);
int rvs_bfgs_result_jac(void *h, double *x, double *fun, int32_t *nit, int32_t *nfev, int32_t *njev, int32_t *status, double *hess_inv, int64_t *rounds);
void rvs_bfgs_end(void *h);
}
int main() {
  const int S = 200, n = 6;
  std::vector<double> x0(S * n);
  for (int i = 0; i < S * n; i++) x0[i] = std::sin(0.37 * i) * 2;
  void *h = rvs_bfgs_begin_jac(S, n, x0.data(), nullptr, 1e-5, 1e-4, 0.9, 0, 0);
  if (!h) return 1;
  std::vector<int64_t> idx(S);
  std::vector<double> X(S * n), F(S * (n + 1));
  int64_t rows;
  while ((rows = rvs_bfgs_pending(h, idx.data(), X.data(), S)) > 0) {
    for (int64_t r = 0; r < rows; r++) {
      // f = sum_j w_j (x_j - c_j)^2 + 0.1 sum_j (x_j - c_j)^4, w_j = 1 .. 10^(n-1)/2
      double f = 0;
      for (int j = 0; j < n; j++) {
        const double w = std::pow(10.0, 0.5 * j), d = X[r * n + j] - 0.1 * j;
        f += w * d * d + 0.1 * d * d * d * d;
        double g = 2 * w * d + 0.4 * d * d * d;
        if (idx[r] % 7 == 0) g *= 1 + 1e-3 * std::sin(1e3 * X[r * n + j]);
        F[r * (n + 1) + 1 + j] = g;
      }
      F[r * (n + 1)] = f;
    }
    if (rvs_bfgs_feed(h, F.data(), rows) == 0) return 4;  // the wrong feed is refused
    if (rvs_bfgs_feed_jac(h, F.data(), rows + 1) == 0) return 5;
    if (rvs_bfgs_feed_jac(h, F.data(), rows)) return 2;
  }
  std::vector<double> x(S * n), fun(S), H(S * n * n);
  std::vector<int32_t> nit(S), nfev(S), njev(S), st(S);
  int64_t rounds;
  if (rvs_bfgs_result_jac(h, x.data(), fun.data(), nit.data(), nfev.data(), njev.data(), st.data(), H.data(), &rounds)) return 3;
  rvs_bfgs_end(h);
  double fm = 0;
  int nmax = 0, nconv = 0;
  for (int s = 0; s < S; s++) {
    fm += fun[s];
    if (nit[s] > nmax) nmax = nit[s];
    if (st[s] == 0) nconv++;
  }
  printf("rounds %lld mean f %.3g max nit %d converged %d\n", (long long)rounds, fm / S, nmax, nconv);
  return 0;
}
