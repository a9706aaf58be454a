"""config['second_minimizer_lm'] of vel_fit.process: Levenberg-Marquardt on the value,
the exact gradient and the Fisher (Gauss-Newton) matrix of the objective, for S spectra
in lock-step.  The per-spectrum state machine (csrc/lm_machine.h) is Nielsen's damping
with Marquardt's diagonal scaling; a run asks for ONE row per request and is answered
with (f, grad f, H packed: the lower triangle row-major).  Two drivers around the one
machine, as bfgs.py has:
  minimize_lockstep_device  the rounds on the GPU (rvs_lm_run: one thread per run, the
                            Fisher form of optimizer.GradChain's chain as the objective)
  minimize_lockstep_native  the machines on the host (rvs_lm_begin / _pending / _feed)
                            around any Python objective (GradChain.rows of either form)
The Python statement of the algorithm lives with the tests
(tests/refmachines/lm_restated.py); tests/test_lm_cpu.py holds the C++ machine against it.

status: 0 converged (max |g_i| <= gtol, or a step below xtol after an accepted one),
1 maxiter, 2 no decrease can be found (a step below xtol after a rejected one, mu beyond
mu_max) or a bad first row.  nfev counts rows.
"""
import numpy as np

TAU = 1e-3
XTOL = 1e-10
MU_MAX = 1e16


def npack(n):
    """length of a row: f, the gradient, the lower triangle of H"""
    return 1 + n + n * (n + 1) // 2


def unpack_rows(F, n):
    """rows [J, npack(n)] -> f [J], g [J, n], H [J, n, n] (full symmetric)"""
    F = np.asarray(F, dtype=np.float64)
    H = np.zeros((F.shape[0], n, n))
    il = np.tril_indices(n)
    H[:, il[0], il[1]] = F[:, 1 + n:]
    H[:, il[1], il[0]] = F[:, 1 + n:]
    return F[:, 0].copy(), F[:, 1:1 + n].copy(), H


def pack_row(f, g, H):
    """(f, g [n], H [n, n]) -> one row [npack(n)]"""
    g = np.asarray(g, dtype=np.float64)
    H = np.asarray(H, dtype=np.float64)
    return np.concatenate([[f], g, H[np.tril_indices(len(g))]])


def minimize_lockstep_native(func, x0, gtol=1e-5, xtol=XTOL, tau=TAU, mu_max=MU_MAX,
                             maxiter=None, max_rows=None):
    """func(idx [J], X [J, n]) -> [J, npack(n)]; x0 [S, n], n <= 8.  Returns x, fun,
    grad, hess [S, n, n] (H at x), mu, nit, nfev, status, rounds."""
    import ctypes
    from . import _lib
    L = _lib.lib()
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    S, n = x0.shape

    def p(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    h = L.rvs_lm_begin(S, n, p(x0), float(gtol), float(xtol), float(tau),
                       float(mu_max), int(maxiter or 0))
    if not h:
        raise ValueError('rvs_lm_begin: bad arguments (n <= 8)')
    h = ctypes.c_void_p(h)
    m = npack(n)
    try:
        idx = np.empty(S, dtype=np.int64)
        X = np.empty((S, n), dtype=np.float64)
        while True:
            rows = L.rvs_lm_pending(h, p(idx), p(X), S)
            if rows < 0:
                raise RuntimeError('rvs_lm_pending failed (%d)' % rows)
            if rows == 0:
                break
            step = rows if max_rows is None else max_rows
            F = np.concatenate([
                np.asarray(func(idx[a:min(rows, a + step)], X[a:min(rows, a + step)]),
                           dtype=np.float64) for a in range(0, rows, step)])
            F = np.ascontiguousarray(F)
            if F.shape != (rows, m):
                raise ValueError('the objective returns [rows, 1 + n + n (n + 1) / 2], '
                                 'not %s' % (F.shape, ))
            _lib.check(L.rvs_lm_feed(h, p(F), rows), 'rvs_lm_feed')
        x, grad = np.empty((S, n)), np.empty((S, n))
        fun, mu = np.empty(S), np.empty(S)
        hess = np.empty((S, n, n))
        nit, nfev, status = (np.empty(S, dtype=np.int32) for _ in range(3))
        rounds = ctypes.c_int64(0)
        _lib.check(L.rvs_lm_result(h, p(x), p(fun), p(grad), p(hess), p(mu), p(nit),
                                   p(nfev), p(status), ctypes.byref(rounds)),
                   'rvs_lm_result')
    finally:
        L.rvs_lm_end(h)
    return dict(x=x, fun=fun, grad=grad, hess=hess, mu=mu, nit=nit.astype(np.int64),
                nfev=nfev.astype(np.int64), status=status.astype(np.int64),
                rounds=int(rounds.value))


def minimize_lockstep_device(pobj, x0, gtol=1e-5, xtol=XTOL, tau=TAU, mu_max=MU_MAX,
                             maxiter=None, sync_every=4, chain=None, cap=None):
    """The runs on the device (csrc/lm_dev.hip, rvs_lm_run) around an
    optimizer.ProcessObjective: x0 [S, n] device tensor; `chain` an
    optimizer.GradChain(pobj, fisher=True), or one built here with `cap` rows per chunk;
    a GradChain(pobj, fused_fisher=True) takes rvs_lm_run_fused (one rvs_objective_fisher
    call per chunk in the place of the chain's stages).
    Returns device tensors x, grad [S, n], fun, mu [S], hess [S, n, n], nit, nfev,
    status [S] and the statistics of the run (rounds, objective calls, rows launched).
    Libraries and options the gradient does not cover raise ValueError."""
    import ctypes
    import torch
    from . import _lib
    L = _lib.lib()
    dev = x0.device
    S, n = x0.shape
    if n != pobj.n or S != pobj.S:
        raise ValueError('minimize_lockstep_device: x0 does not fit the objective')
    if chain is None:
        from . import optimizer
        chain = optimizer.GradChain(pobj, cap=cap, fisher=True)
    if not chain.fisher:
        raise ValueError('minimize_lockstep_device: the chain was built without '
                         'fisher=True')
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    keep = dict(
        runs=torch.empty(S * int(L.rvs_lm_run_bytes()) // 8 + 1, **f64),
        x0=x0.to(torch.float64).contiguous(), x=torch.empty((S, n), **f64),
        fun=torch.empty(S, **f64), grad=torch.empty((S, n), **f64),
        hess=torch.empty((S, n, n), **f64), mu=torch.empty(S, **f64),
        nit=torch.empty(S, **i32), nfev=torch.empty(S, **i32),
        status=torch.empty(S, **i32), nreq=torch.zeros(S, **i32),
        off=torch.zeros(S, **i32), list=torch.zeros(S, **i32),
        counts=torch.zeros(32, **i32), X=torch.zeros((S, n), **f64),
        F=torch.zeros((S, npack(n)), **f64))
    b = _lib.LmState()
    for k, t in keep.items():
        setattr(b, k, t.data_ptr())
    b.gtol, b.xtol, b.tau, b.mu_max = float(gtol), float(xtol), float(tau), \
        float(mu_max)
    b.S, b.n, b.maxiter = S, n, int(maxiter or 0)
    o = pobj.native_desc()
    g = chain.desc()
    st3 = (ctypes.c_int64 * 3)()
    if getattr(chain, 'fused_fisher', False):
        # optimizer.GradChain(fused_fisher=True): one rvs_objective_fisher call per chunk
        _lib.check(L.rvs_lm_run_fused(ctypes.addressof(b), ctypes.addressof(o),
                                      ctypes.addressof(g), ctypes.addressof(chain.garms),
                                      ctypes.addressof(chain.bconst),
                                      chain.fwork.data_ptr(), int(chain.nbytes),
                                      int(sync_every), st3, _lib.stream()),
                   'rvs_lm_run_fused')
    else:
        fc = chain.fisher_desc()
        _lib.check(L.rvs_lm_run(ctypes.addressof(b), ctypes.addressof(o),
                                ctypes.addressof(g), ctypes.addressof(fc),
                                int(sync_every), st3, _lib.stream()), 'rvs_lm_run')
    pobj.calls += int(st3[1])
    pobj.slots += int(st3[2])
    pobj.jobs += int(st3[2])
    return dict(x=keep['x'], fun=keep['fun'], grad=keep['grad'], hess=keep['hess'],
                mu=keep['mu'], nit=keep['nit'].long(), nfev=keep['nfev'].long(),
                status=keep['status'].long(), rounds=int(st3[0]), calls=int(st3[1]),
                rows_launched=int(st3[2]))
