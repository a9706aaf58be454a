"""Lock-step BFGS on an objective that returns its gradient:
scipy.optimize.minimize(fun, x0, method='BFGS', jac=True, options=dict(hess_inv0=...))
restated as one Python generator per run, beside bfgs_scipy_restated.py (the
forward-difference form), whose line searches (_wolfe1, _wolfe2: MINPACK-2
dcsrch / dcstep, the zoom fall-back) it uses as they are -- they only ever ask
their `sf` for fun / grad / fun_grad.

What differs is where f and g come from (scipy 1.15):
  minimize()         wraps fun in MemoizeJac: fun = MemoizeJac(fun), jac =
                     fun.derivative.  MemoizeJac calls the user's function when x
                     differs from the x of its last call, and keeps both halves.
  ScalarFunction     fun(x) -> _update_fun -> MemoizeJac.__call__, nfev += 1;
                     grad(x) -> _update_grad -> MemoizeJac.derivative, ngev += 1
                     (a callable grad does not ask for f first).
MemoizeJac is only ever called at ScalarFunction's own x, so the user's function
runs once per distinct consecutive x, and a request of the generator is always
ONE point; it is sent (f, g).  Control flow and the order of every floating-point
operation follow scipy, so on equal function values the iterates are identical
(tests/test_bfgs_jac_cpu.py compares with scipy itself).
"""
import numpy as np

from refmachines.bfgs_scipy_restated import _Fail, _wolfe1, _wolfe2


class _SFJac:
    """ScalarFunction over MemoizeJac: f and g of the latest x, both from one call"""

    def __init__(self):
        self.x = None
        self.f = None
        self.g = None
        self.memo = None     # MemoizeJac's (value, jac) at self.x
        self.nfev = 0
        self.ngev = 0

    def _set_x(self, x):
        if self.x is None or not (x == self.x).all():
            self.x = np.array(x, dtype=float, copy=True)
            self.f = None
            self.g = None
            self.memo = None

    def _compute_if_needed(self):
        if self.memo is None:
            f, g = yield ('fg', self.x)
            self.memo = (float(f), np.atleast_1d(np.asarray(g, dtype=float)))

    def fun(self, x):
        self._set_x(x)
        if self.f is None:
            yield from self._compute_if_needed()
            self.f = self.memo[0]
            self.nfev += 1
        return self.f

    def grad(self, x):
        self._set_x(x)
        if self.g is None:
            yield from self._compute_if_needed()
            self.g = self.memo[1]
            self.ngev += 1
        return self.g

    def fun_grad(self, x):
        f = yield from self.fun(x)
        g = yield from self.grad(x)
        return f, g


def bfgs_generator_jac(x0, hess_inv0=None, gtol=1e-5, c1=1e-4, c2=0.9, xrtol=0,
                       maxiter=None):
    """_minimize_bfgs for one starting point as a request generator: yields
    ('fg', x [n]) and is sent (f, g [n]); its return value (StopIteration.value)
    is dict(x, fun, jac, hess_inv, nit, nfev, njev, status, success)."""
    sf = _SFJac()
    x0 = np.asarray(x0, dtype=float).flatten()
    N = len(x0)
    if maxiter is None:
        maxiter = N * 200
    old_fval, gfk = yield from sf.fun_grad(x0)
    k = 0
    I = np.eye(N, dtype=int)
    Hk = I if hess_inv0 is None else hess_inv0
    old_old_fval = old_fval + np.linalg.norm(gfk) / 2
    xk = x0
    warnflag = 0
    gnorm = np.amax(np.abs(gfk))
    while (gnorm > gtol) and (k < maxiter):
        pk = -np.dot(Hk, gfk)
        try:
            # _line_search_wolfe12(amin=1e-100, amax=1e100)
            stp, fval, ofv, gfkp1 = yield from _wolfe1(
                sf, xk, pk, gfk, old_fval, old_old_fval, c1, c2, 1e100, 1e-100)
            if stp is None:
                stp, fval, ofv, gfkp1 = yield from _wolfe2(
                    sf, xk, pk, gfk, old_fval, old_old_fval, c1, c2, 1e100)
            if stp is None:
                raise _Fail()
            alpha_k = stp
            old_fval, old_old_fval = fval, ofv
        except _Fail:
            warnflag = 2
            break
        sk = alpha_k * pk
        xkp1 = xk + sk
        xk = xkp1
        if gfkp1 is None:
            gfkp1 = yield from sf.grad(xkp1)
        yk = gfkp1 - gfk
        gfk = gfkp1
        k += 1
        gnorm = np.amax(np.abs(gfk))
        if gnorm <= gtol:
            break
        if alpha_k * np.sqrt(np.sum(pk**2)) <= xrtol * (
                xrtol + np.sqrt(np.sum(xk**2))):
            break
        if not np.isfinite(old_fval):
            warnflag = 2
            break
        rhok_inv = np.dot(yk, sk)
        if rhok_inv == 0.:
            rhok = 1000.0
        else:
            rhok = 1. / rhok_inv
        A1 = I - sk[:, np.newaxis] * yk[np.newaxis, :] * rhok
        A2 = I - yk[:, np.newaxis] * sk[np.newaxis, :] * rhok
        Hk = np.dot(A1, np.dot(Hk, A2)) + (rhok * sk[:, np.newaxis] *
                                            sk[np.newaxis, :])
    fval = old_fval
    if warnflag == 2:
        pass
    elif k >= maxiter:
        warnflag = 1
    elif np.isnan(gnorm) or np.isnan(fval) or np.isnan(xk).any():
        warnflag = 3
    return dict(x=xk, fun=fval, jac=gfk, hess_inv=Hk, nit=k, nfev=sf.nfev,
                njev=sf.ngev, status=warnflag, success=(warnflag == 0))


def minimize_lockstep_jac(func, x0, hess_inv0=None, max_rows=None, **kw):
    """BFGS from every row of x0 [S, n] (numpy).  func(idx int64 [J], X [J, n])
    -> [J, 1 + n] (value, gradient) is called with the requests of all runs that
    are waiting, at most max_rows rows at a time.
    Returns dict(x [S,n], fun, nit, nfev, njev, status [S], hess_inv, rounds)."""
    x0 = np.asarray(x0, dtype=float)
    S, n = x0.shape
    gens = [bfgs_generator_jac(x0[i], hess_inv0=hess_inv0, **kw) for i in range(S)]
    pending = {}
    results = [None] * S
    for i, g in enumerate(gens):
        pending[i] = next(g)     # the first request is (f, g)(x0)
    rounds = 0
    while pending:
        rounds += 1
        ids = sorted(pending)
        X = np.stack([pending[i][1] for i in ids])
        idx = np.asarray(ids, dtype=np.int64)
        step = len(ids) if max_rows is None else max_rows
        F = np.concatenate([
            np.asarray(func(idx[a:a + step], X[a:a + step]), dtype=float)
            for a in range(0, len(ids), step)])
        assert F.shape == (len(ids), n + 1)
        for r, i in enumerate(ids):
            try:
                pending[i] = gens[i].send((float(F[r, 0]), F[r, 1:].copy()))
            except StopIteration as e:
                results[i] = e.value
                del pending[i]
    return dict(x=np.stack([r['x'] for r in results]),
                fun=np.array([r['fun'] for r in results]),
                nit=np.array([r['nit'] for r in results]),
                nfev=np.array([r['nfev'] for r in results]),
                njev=np.array([r['njev'] for r in results]),
                status=np.array([r['status'] for r in results]),
                hess_inv=[np.asarray(r['hess_inv'], dtype=float) for r in results],
                rounds=rounds)
