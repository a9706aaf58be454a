"""Levenberg-Marquardt on (value, gradient, Gauss-Newton matrix) for S runs in
lock-step: the statement csrc/lm_machine.h follows line by line.

Nielsen's damping (H. B. Nielsen, "Damping parameter in Marquardt's method", IMM-REP
1999-05) with Marquardt's diagonal scaling.  One request of a run is ONE row x; its
reply is (f, g [n], H packed: the lower triangle row-major, n (n + 1) / 2 entries).
Everything is scalar arithmetic on Python floats with explicit loops in index order,
so that the C++ machine (no FMA contraction) can give the same bits.

  1. request x0; a reply that is not finite, or a bad row (f >= 1e30): status 2, x = x0
  2. max |g_i| <= gtol: status 0
  3. d_i = 1 / sqrt(H_ii) where H_ii > 0, else 1;  A = d H d + mu I;  Cholesky of A;
     a non-positive pivot counts as a rejected step (6)
  4. A y = -d g, delta = d y; |delta_i| <= xtol (|x_i| + xtol) for every i: the run
     ends, status 0 if the previous trial was accepted (or there was none), 2 after a
     rejection ("precision loss": no decrease can be found)
  5. request x + delta -> (f_t, g_t, H_t);
     pred = 1/2 sum delta_i (mu delta_i / d_i^2 - g_i), rho = (f - f_t) / pred
  6. the reply finite, pred > 0 and rho > 0: accept -- (x, f, g, H) <- trial, nit += 1,
     mu <- mu max(1/3, 1 - (2 rho - 1)^3), nu <- 2;
     else reject -- mu <- mu nu, nu <- 2 nu; mu > mu_max: status 2.
     nit >= maxiter: status 1.
(pred > 0 holds in exact arithmetic, A being positive definite; asking for it keeps a
rounded pred <= 0 from turning an increase into rho > 0.  "The reply finite" is asked
of g_t and H_t too: a point with a NaN derivative is never made the current one.)
nfev counts rows."""
import math

import numpy as np

TAU = 1e-3
XTOL = 1e-10
MU_MAX = 1e16
THIRD = 1.0 / 3.0


def npack(n):
    return 1 + n + n * (n + 1) // 2


class Run:
    def __init__(self, x0, gtol=1e-5, xtol=XTOL, tau=TAU, mu_max=MU_MAX,
                 maxiter=None):
        n = len(x0)
        self.n = n
        self.x = [float(v) for v in x0]
        self.xt = list(self.x)
        self.f = 0.0
        self.g = [0.0] * n
        self.H = [0.0] * (n * (n + 1) // 2)
        self.mu, self.nu, self.pred = float(tau), 2.0, 0.0
        self.gtol, self.xtol, self.mu_max = float(gtol), float(xtol), float(mu_max)
        self.maxiter = int(maxiter) if maxiter else 200 * n
        self.nit = self.nfev = self.status = 0
        self.nrej = 0          # rejections (diagnostic; the C++ machine counts them too)
        self.phase = 0
        self.pending = False   # a request (self.xt) waits for its reply
        self.rejected = False  # the previous trial was rejected
        self.done = False

    def _end(self, status):
        self.status = status
        self.done = True
        self.pending = False

    def _finite(self, reply):
        for q in range(npack(self.n)):
            if not math.isfinite(reply[q]):
                return False
        return True

    def _take(self, reply):
        n = self.n
        self.f = reply[0]
        for i in range(n):
            self.g[i] = reply[1 + i]
        for q in range(n * (n + 1) // 2):
            self.H[q] = reply[1 + n + q]

    def _reject(self):
        """step 6, the reject branch; True where the run ended"""
        self.nrej += 1
        self.rejected = True
        self.mu = self.mu * self.nu
        self.nu = 2.0 * self.nu
        if self.mu > self.mu_max:
            self._end(2)
            return True
        if self.nit >= self.maxiter:
            self._end(1)
            return True
        return False

    def advance(self, reply=None):
        """runs until the next request (self.pending, the row is self.xt) or the end
        (self.done); `reply` answers the request before"""
        n = self.n
        if self.phase == 0:
            self.phase = 1
            self.pending = True
            return
        self.pending = False
        self.nfev += 1
        if self.phase == 1:
            reply = [float(v) for v in reply]
            self.f = reply[0]
            if not self._finite(reply) or reply[0] >= 1e30:
                self._end(2)
                return
            self._take(reply)
            self.phase = 2
        else:
            reply = [float(v) for v in reply]
            ft = reply[0]
            ok = self._finite(reply) and self.pred > 0
            rho = 0.0
            if ok:
                rho = (self.f - ft) / self.pred
                ok = rho > 0
            if ok:
                for i in range(n):
                    self.x[i] = self.xt[i]
                self._take(reply)
                self.nit += 1
                t = 2.0 * rho - 1.0
                t = 1.0 - t * t * t
                self.mu = self.mu * (THIRD if THIRD > t else t)
                self.nu = 2.0
                self.rejected = False
                if self.nit >= self.maxiter:
                    self._end(1)
                    return
            elif self._reject():
                return
        d = [0.0] * n
        L = [0.0] * (n * (n + 1) // 2)
        y = [0.0] * n
        while True:
            # 2
            gmax = 0.0
            for i in range(n):
                a = abs(self.g[i])
                if a > gmax:
                    gmax = a
            if gmax <= self.gtol:
                self._end(0)
                return
            # 3
            for i in range(n):
                hii = self.H[i * (i + 1) // 2 + i]
                d[i] = 1.0 / math.sqrt(hii) if hii > 0 else 1.0
            posdef = True
            for i in range(n):
                for j in range(i + 1):
                    s = (d[i] * self.H[i * (i + 1) // 2 + j]) * d[j]
                    if i == j:
                        s = s + self.mu
                    for k in range(j):
                        s = s - L[i * (i + 1) // 2 + k] * L[j * (j + 1) // 2 + k]
                    if i == j:
                        if not s > 0:
                            posdef = False
                            break
                        L[i * (i + 1) // 2 + i] = math.sqrt(s)
                    else:
                        L[i * (i + 1) // 2 + j] = s / L[j * (j + 1) // 2 + j]
                if not posdef:
                    break
            if not posdef:
                if self._reject():
                    return
                continue
            # 4: L z = -d g, L^T y = z
            for i in range(n):
                s = -(d[i] * self.g[i])
                for k in range(i):
                    s = s - L[i * (i + 1) // 2 + k] * y[k]
                y[i] = s / L[i * (i + 1) // 2 + i]
            for i in range(n - 1, -1, -1):
                s = y[i]
                for k in range(i + 1, n):
                    s = s - L[k * (k + 1) // 2 + i] * y[k]
                y[i] = s / L[i * (i + 1) // 2 + i]
            small = True
            pred = 0.0
            for i in range(n):
                delta = d[i] * y[i]
                if not abs(delta) <= self.xtol * (abs(self.x[i]) + self.xtol):
                    small = False
                # 5 (mu delta_i / d_i^2 = mu y_i / d_i)
                pred = pred + delta * (self.mu * y[i] / d[i] - self.g[i])
                self.xt[i] = self.x[i] + delta
            if small:
                self._end(2 if self.rejected else 0)
                return
            self.pred = 0.5 * pred
            self.pending = True
            return

    def hess(self):
        n = self.n
        out = np.zeros((n, n))
        for i in range(n):
            for j in range(i + 1):
                out[i, j] = out[j, i] = self.H[i * (i + 1) // 2 + j]
        return out


def minimize_lockstep(func, x0, gtol=1e-5, xtol=XTOL, tau=TAU, mu_max=MU_MAX,
                      maxiter=None, max_rows=None):
    """func(idx [J], X [J, n]) -> [J, 1 + n + n (n + 1) / 2]; x0 [S, n].  A round
    gathers the pending rows of all runs in run order, asks func for them (in chunks
    of max_rows) and resumes the runs."""
    x0 = np.asarray(x0, dtype=np.float64)
    S, n = x0.shape
    runs = [Run(x0[s], gtol, xtol, tau, mu_max, maxiter) for s in range(S)]
    for r in runs:
        r.advance()
    rounds = 0
    while True:
        order = [s for s in range(S) if runs[s].pending]
        if not order:
            break
        idx = np.array(order, dtype=np.int64)
        X = np.array([runs[s].xt for s in order], dtype=np.float64)
        step = len(order) if max_rows is None else max_rows
        F = np.concatenate([np.asarray(func(idx[a:a + step], X[a:a + step]),
                                       dtype=np.float64)
                            for a in range(0, len(order), step)])
        assert F.shape == (len(order), npack(n)), F.shape
        for q, s in enumerate(order):
            runs[s].advance(F[q])
        rounds += 1
    return dict(x=np.array([r.x for r in runs]), fun=np.array([r.f for r in runs]),
                grad=np.array([r.g for r in runs]),
                hess=np.array([r.hess() for r in runs]),
                mu=np.array([r.mu for r in runs]),
                nit=np.array([r.nit for r in runs], dtype=np.int64),
                nfev=np.array([r.nfev for r in runs], dtype=np.int64),
                nrej=np.array([r.nrej for r in runs], dtype=np.int64),
                status=np.array([r.status for r in runs], dtype=np.int64),
                rounds=rounds)
