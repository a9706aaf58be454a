"""Levenberg-Marquardt on an arrowhead Gauss-Newton matrix, for N stars in lock-step: the
statement csrc/alm_machine.h follows line by line.

A star has m shared parameters theta and E epochs with one velocity each; its vector is
z = (theta [m], v [E]), n = m + E.  The objective is the sum over the epochs of terms that
depend on (theta, v_e) only, so the Gauss-Newton matrix is

    [ Htt   c_0  c_1 ... ]      Htt [m, m] dense, h_e the diagonal over the velocities,
    [ c_0^T h_0          ]      c_e [m] the border
    [ c_1^T      h_1     ]
    [ ...            ... ]

One request of a run is ONE vector z; its reply is the arrow row
    f, g_theta [m], Htt packed (lower triangle row-major, m (m + 1) / 2),
    then per epoch (g_e, h_e, c_e [m])
of width 1 + m + m (m + 1) / 2 + E (2 + m).

The algorithm is tests/refmachines/lm_restated.py's (steps 1 - 6 of its header: Nielsen's
damping, Marquardt's scaling, the same constants and status codes) over z, with the dense
Cholesky of step 3 replaced by the elimination of the velocities:

  3. d_i = 1 / sqrt(Htt_ii) where positive, else 1; d_e = 1 / sqrt(h_e) where positive,
     else 1;  a_e = (d_e h_e) d_e + mu;  b_e[i] = (d_e c_e[i]) d_i;
     S_ij = (d_i Htt_ij) d_j + mu delta_ij - sum_e b_e[i] b_e[j] / a_e;  Cholesky of S.
     a_e <= 0 or a non-positive pivot counts as a rejected step
  4. rhs_i = -d_i g_i + sum_e b_e[i] (d_e g_e) / a_e;  S y_theta = rhs;
     y_e = (-d_e g_e - b_e . y_theta) / a_e;  delta = d y
The gradient test, the xtol test and pred = 1/2 sum delta_i (mu y_i / d_i - g_i) run over
all m + E entries, theta first, then the epochs in order.  Everything is scalar arithmetic
on Python floats with explicit loops in index order (the sums over e ascending), so that
the C++ machine (no FMA contraction) can give the same bits.  nfev counts rows."""
import math

import numpy as np

TAU = 1e-3
XTOL = 1e-10
MU_MAX = 1e16
THIRD = 1.0 / 3.0
MAXM = 7


def row_size(m, E):
    return 1 + m + m * (m + 1) // 2 + E * (2 + m)


def arrow_step(row, m, E, mu):
    """steps 3 and 4 on one row: (ok, d [n], y [n]); ok False where a_e <= 0 or a pivot
    of the Schur complement is not positive"""
    n = m + E
    H0 = 1 + m                      # Htt packed
    E0 = H0 + m * (m + 1) // 2      # the epochs' records
    w = 2 + m
    d = [0.0] * n
    y = [0.0] * n
    a = [0.0] * E
    L = [0.0] * (m * (m + 1) // 2)
    for i in range(m):
        hii = row[H0 + i * (i + 1) // 2 + i]
        d[i] = 1.0 / math.sqrt(hii) if hii > 0 else 1.0
    for e in range(E):
        he = row[E0 + e * w + 1]
        d[m + e] = 1.0 / math.sqrt(he) if he > 0 else 1.0
        a[e] = (d[m + e] * he) * d[m + e] + mu
        if not a[e] > 0:
            return False, d, y

    def b(e, i):
        return (d[m + e] * row[E0 + e * w + 2 + i]) * d[i]

    for i in range(m):
        for j in range(i + 1):
            s = (d[i] * row[H0 + i * (i + 1) // 2 + j]) * d[j]
            if i == j:
                s = s + mu
            for e in range(E):
                s = s - b(e, i) * b(e, j) / a[e]
            for k in range(j):
                s = s - L[i * (i + 1) // 2 + k] * L[j * (j + 1) // 2 + k]
            if i == j:
                if not s > 0:
                    return False, d, y
                L[i * (i + 1) // 2 + i] = math.sqrt(s)
            else:
                L[i * (i + 1) // 2 + j] = s / L[j * (j + 1) // 2 + j]
    # 4: L z = rhs, L^T y_theta = z
    for i in range(m):
        s = -(d[i] * row[1 + i])
        for e in range(E):
            s = s + b(e, i) * (d[m + e] * row[E0 + e * w]) / a[e]
        for k in range(i):
            s = s - L[i * (i + 1) // 2 + k] * y[k]
        y[i] = s / L[i * (i + 1) // 2 + i]
    for i in range(m - 1, -1, -1):
        s = y[i]
        for k in range(i + 1, m):
            s = s - L[k * (k + 1) // 2 + i] * y[k]
        y[i] = s / L[i * (i + 1) // 2 + i]
    for e in range(E):
        s = -(d[m + e] * row[E0 + e * w])
        for i in range(m):
            s = s - b(e, i) * y[i]
        y[m + e] = s / a[e]
    return True, d, y


class Run:
    def __init__(self, m, x0, gtol=1e-5, xtol=XTOL, tau=TAU, mu_max=MU_MAX,
                 maxiter=None):
        n = len(x0)
        assert 1 <= m <= MAXM and n > m
        self.m, self.E, self.n = m, n - m, n
        self.x = [float(v) for v in x0]
        self.xt = list(self.x)
        self.f = 0.0
        self.g = [0.0] * n
        self.row = [0.0] * row_size(m, n - m)
        self.mu, self.nu, self.pred = float(tau), 2.0, 0.0
        self.gtol, self.xtol, self.mu_max = float(gtol), float(xtol), float(mu_max)
        self.maxiter = int(maxiter) if maxiter else 200 * n
        self.nit = self.nfev = self.status = 0
        self.nrej = 0
        self.phase = 0
        self.pending = False
        self.rejected = False
        self.done = False

    def _end(self, status):
        self.status = status
        self.done = True
        self.pending = False

    def _finite(self, reply):
        for q in range(row_size(self.m, self.E)):
            if not math.isfinite(reply[q]):
                return False
        return True

    def _take(self, reply):
        m, E = self.m, self.E
        for q in range(row_size(m, E)):
            self.row[q] = reply[q]
        self.f = reply[0]
        for i in range(m):
            self.g[i] = reply[1 + i]
        E0 = 1 + m + m * (m + 1) // 2
        for e in range(E):
            self.g[m + e] = reply[E0 + e * (2 + m)]

    def _reject(self):
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
        n = self.n
        if self.phase == 0:
            self.phase = 1
            self.pending = True
            return
        self.pending = False
        self.nfev += 1
        reply = [float(v) for v in reply]
        if self.phase == 1:
            self.f = reply[0]
            if not self._finite(reply) or reply[0] >= 1e30:
                self._end(2)
                return
            self._take(reply)
            self.phase = 2
        else:
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
            # 3, 4
            ok, d, y = arrow_step(self.row, self.m, self.E, self.mu)
            if not ok:
                if self._reject():
                    return
                continue
            small = True
            pred = 0.0
            for i in range(n):
                delta = d[i] * y[i]
                if not abs(delta) <= self.xtol * (abs(self.x[i]) + self.xtol):
                    small = False
                # 5
                pred = pred + delta * (self.mu * y[i] / d[i] - self.g[i])
                self.xt[i] = self.x[i] + delta
            if small:
                self._end(2 if self.rejected else 0)
                return
            self.pred = 0.5 * pred
            self.pending = True
            return


def offsets(m, eoff):
    """start of every star's vector and row in the ragged buffers (and their ends)"""
    eoff = np.asarray(eoff, dtype=np.int64)
    N = len(eoff) - 1
    k = np.arange(N + 1, dtype=np.int64)
    return k * m + eoff, k * (1 + m + m * (m + 1) // 2) + eoff * (2 + m)


def minimize_lockstep(func, m, eoff, x0, gtol=1e-5, xtol=XTOL, tau=TAU, mu_max=MU_MAX,
                      maxiter=None, max_stars=None):
    """func(idx [J], Z: list of J vectors) -> list of J rows; x0 ragged [N m + S]: per
    star theta [m] then v [E].  A round gathers the pending vectors of all runs in run
    order, asks func for them (in chunks of max_stars) and resumes the runs."""
    x0 = np.asarray(x0, dtype=np.float64)
    xo, ro = offsets(m, eoff)
    N = len(xo) - 1
    assert len(x0) == xo[-1]
    runs = [Run(m, x0[xo[s]:xo[s + 1]], gtol, xtol, tau, mu_max, maxiter)
            for s in range(N)]
    for r in runs:
        r.advance()
    rounds = 0
    while True:
        order = [s for s in range(N) if runs[s].pending]
        if not order:
            break
        step = len(order) if max_stars is None else max_stars
        rows = []
        for a in range(0, len(order), step):
            part = order[a:a + step]
            rows += list(func(np.array(part, dtype=np.int64),
                              [np.array(runs[s].xt) for s in part]))
        assert len(rows) == len(order)
        for q, s in enumerate(order):
            assert len(rows[q]) == row_size(m, runs[s].E)
            runs[s].advance(rows[q])
        rounds += 1
    return dict(x=np.concatenate([r.x for r in runs]),
                fun=np.array([r.f for r in runs]),
                grad=np.concatenate([r.g for r in runs]),
                row=np.concatenate([r.row for r in runs]),
                mu=np.array([r.mu for r in runs]),
                nit=np.array([r.nit for r in runs], dtype=np.int64),
                nfev=np.array([r.nfev for r in runs], dtype=np.int64),
                nrej=np.array([r.nrej for r in runs], dtype=np.int64),
                status=np.array([r.status for r in runs], dtype=np.int64),
                rounds=rounds)
