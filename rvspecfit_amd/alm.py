"""vel_fit.process_epochs: Levenberg-Marquardt for N stars in lock-step, each with m shared
parameters theta and one velocity per epoch, on the arrowhead Gauss-Newton matrix of the
joint objective.  The per-star state machine (csrc/alm_machine.h) is lm.py's -- Nielsen's
damping, Marquardt's scaling, the same constants and status codes -- with the dense
Cholesky replaced by the elimination of the velocities.  A run asks for ONE vector
z = (theta [m], v [E]) per request and is answered with the arrow row
    f, g_theta [m], Htt packed (lower triangle row-major), then per epoch (g_e, h_e, c_e [m])
(optimizer.EpochChain.rows, rvs_epoch_finish).  Buffers are ragged: star s with E_s =
eoff[s + 1] - eoff[s] epochs has its vector at s m + eoff[s] and its row at
s (1 + m + m (m + 1) / 2) + eoff[s] (2 + m).

  minimize_lockstep_device  the rounds on the GPU (rvs_alm_run: one thread per star, the
                            joint chain of optimizer.EpochChain launched from C)
  minimize_lockstep_native  the machines on the host (rvs_alm_begin / _pending / _feed)
                            around any Python objective
The Python statement of the algorithm lives with the tests
(tests/refmachines/lm_arrow_restated.py); tests/test_epochs_cpu.py holds the C++ machine
against it bit for bit.  status and nfev as lm.py's.
"""
import numpy as np

TAU = 1e-3
XTOL = 1e-10
MU_MAX = 1e16
MAXM = 7


def row_size(m, E):
    """length of a star's row"""
    return 1 + m + m * (m + 1) // 2 + E * (2 + m)


def offsets(m, eoff):
    """(xoff [N + 1], rowoff [N + 1]): where every star's vector and row start in the
    ragged buffers, and where the buffers end"""
    eoff = np.asarray(eoff, dtype=np.int64)
    k = np.arange(len(eoff), dtype=np.int64)
    return k * m + eoff, k * (1 + m + m * (m + 1) // 2) + eoff * (2 + m)


def unpack_row(row, m, E):
    """one row -> f, g_theta [m], Htt [m, m] (full symmetric), g_v [E], h [E], c [E, m]"""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape == (row_size(m, E), )
    H = np.zeros((m, m))
    il = np.tril_indices(m)
    H[il] = row[1 + m:1 + m + len(il[0])]
    H[il[1], il[0]] = H[il]
    rec = row[1 + m + len(il[0]):].reshape(E, 2 + m)
    return row[0], row[1:1 + m].copy(), H, rec[:, 0].copy(), rec[:, 1].copy(), \
        rec[:, 2:].copy()


def dense(row, m, E):
    """the row's gradient [m + E] and its full arrow matrix [m + E, m + E]"""
    f, gt, H, gv, h, c = unpack_row(row, m, E)
    A = np.zeros((m + E, m + E))
    A[:m, :m] = H
    A[:m, m:] = c.T
    A[m:, :m] = c
    A[np.arange(m, m + E), np.arange(m, m + E)] = h
    return np.concatenate([gt, gv]), A


def minimize_lockstep_native(func, m, eoff, x0, gtol=1e-5, xtol=XTOL, tau=TAU,
                             mu_max=MU_MAX, maxiter=None, max_stars=None):
    """func(idx [J], X ragged, xoff [J + 1]) -> the J rows one behind the other; eoff
    [N + 1] (eoff[0] = 0, every star at least one epoch); x0 ragged [N m + S].  Returns x,
    grad (ragged), row (ragged: the row at x), fun, mu, nit, nfev, status [N], rounds."""
    import ctypes
    from . import _lib
    L = _lib.lib()
    eoff = np.ascontiguousarray(eoff, dtype=np.int32)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    N = len(eoff) - 1
    if m > MAXM or m < 1:
        raise ValueError('the joint fit takes 1 <= m <= %d shared parameters, not %d'
                         % (MAXM, m))
    if N < 1 or eoff[0] != 0 or (np.diff(eoff) < 1).any():
        raise ValueError('eoff: every star needs at least one epoch')
    xo, ro = offsets(m, eoff)
    if x0.shape != (xo[-1], ):
        raise ValueError('x0 has %s entries, the stars need %d' % (x0.shape, xo[-1]))
    nE = np.diff(eoff).astype(np.int64)

    def p(a):
        return None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    h = L.rvs_alm_begin(N, m, p(eoff), p(x0), float(gtol), float(xtol), float(tau),
                        float(mu_max), int(maxiter or 0))
    if not h:
        raise ValueError('rvs_alm_begin: bad arguments')
    h = ctypes.c_void_p(h)
    try:
        idx = np.empty(N, dtype=np.int64)
        X = np.empty(xo[-1], dtype=np.float64)
        while True:
            J = L.rvs_alm_pending(h, p(idx), p(X), X.size)
            if J < 0:
                raise RuntimeError('rvs_alm_pending failed (%d)' % J)
            if J == 0:
                break
            ids = idx[:J]
            lx = np.concatenate([[0], np.cumsum(m + nE[ids])])
            lr = np.concatenate([[0], np.cumsum(row_size(m, nE[ids]))])
            step = J if max_stars is None else max_stars
            F = np.concatenate([
                np.asarray(func(ids[a:a + step], X[lx[a]:lx[min(J, a + step)]],
                                lx[a:a + step + 1] - lx[a]),
                           dtype=np.float64).reshape(-1) for a in range(0, J, step)])
            F = np.ascontiguousarray(F)
            if F.shape != (lr[-1], ):
                raise ValueError('the objective returns %s values, the rows of the %d '
                                 'stars have %d' % (F.shape, J, lr[-1]))
            _lib.check(L.rvs_alm_feed(h, p(F), J), 'rvs_alm_feed')
        x, grad = np.empty(xo[-1]), np.empty(xo[-1])
        row = np.empty(ro[-1])
        fun, mu = np.empty(N), np.empty(N)
        nit, nfev, status = (np.empty(N, dtype=np.int32) for _ in range(3))
        rounds = ctypes.c_int64(0)
        _lib.check(L.rvs_alm_result(h, p(x), p(fun), p(grad), p(row), p(mu), p(nit),
                                    p(nfev), p(status), ctypes.byref(rounds)),
                   'rvs_alm_result')
    finally:
        L.rvs_alm_end(h)
    return dict(x=x, fun=fun, grad=grad, row=row, mu=mu, nit=nit.astype(np.int64),
                nfev=nfev.astype(np.int64), status=status.astype(np.int64),
                rounds=int(rounds.value), xoff=xo, rowoff=ro)


def minimize_lockstep_device(chain, x0, gtol=1e-5, xtol=XTOL, tau=TAU, mu_max=MU_MAX,
                             maxiter=None):
    """The runs on the device (csrc/epochs.hip, rvs_alm_run) around an
    optimizer.EpochChain: one thread per star advances its machine, the joint chain of a
    round is launched from C.  x0 ragged numpy [N m + S] as for
    minimize_lockstep_native, whose keys and bits the result has (numpy arrays; `calls`:
    chunks evaluated, `star_rows`: template-stage rows, `chi_x` [S]: the chi of every
    epoch at its star's x, nan for a star whose first row is bad)."""
    import ctypes
    import torch
    from . import _lib
    L = _lib.lib()
    m, dev = chain.m, chain.dev
    eoff = np.ascontiguousarray(chain.eoff, dtype=np.int32)
    N, S = len(eoff) - 1, int(eoff[-1])
    xo, ro = offsets(m, eoff)
    x0 = np.ascontiguousarray(x0, dtype=np.float64)
    if x0.shape != (xo[-1], ):
        raise ValueError('x0 has %s entries, the stars need %d' % (x0.shape, xo[-1]))
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    keep = dict(
        runs=torch.empty(N * int(L.rvs_alm_run_bytes()) // 8 + 1, **f64),
        state=torch.empty(5 * int(xo[-1]) + S + int(ro[-1]), **f64),
        eoff_dev=torch.as_tensor(eoff).to(dev), x0=torch.as_tensor(x0).to(dev),
        x=torch.empty(int(xo[-1]), **f64), grad=torch.empty(int(xo[-1]), **f64),
        row=torch.empty(int(ro[-1]), **f64), fun=torch.empty(N, **f64),
        mu=torch.empty(N, **f64), F=torch.zeros(int(ro[-1]), **f64),
        chi_trial=torch.zeros(S, **f64), chi_x=torch.full((S, ), np.nan, **f64),
        nit=torch.empty(N, **i32), nfev=torch.empty(N, **i32),
        status=torch.empty(N, **i32), nreq=torch.zeros(N, **i32),
        tab=torch.zeros(6 * N + S + 16, **i32))
    b = _lib.AlmState()
    for k, t in keep.items():
        setattr(b, k, t.data_ptr())
    b.eoff = eoff.ctypes.data
    b.gtol, b.xtol, b.tau, b.mu_max = float(gtol), float(xtol), float(tau), \
        float(mu_max)
    b.N, b.m, b.maxiter = N, m, int(maxiter or 0)
    c = chain.native_desc()
    st3 = (ctypes.c_int64 * 3)()
    _lib.check(L.rvs_alm_run(ctypes.addressof(b), ctypes.addressof(c), st3,
                             _lib.stream()), 'rvs_alm_run')
    chain.calls += int(st3[1])
    chain.star_rows += int(st3[2])
    out = {k: keep[k].cpu().numpy() for k in ('x', 'fun', 'grad', 'row', 'mu', 'chi_x')}
    for k in ('nit', 'nfev', 'status'):
        out[k] = keep[k].cpu().numpy().astype(np.int64)
    chain.epoch_jobs += int((out['nfev'] * np.diff(eoff)).sum())
    out.update(rounds=int(st3[0]), calls=int(st3[1]), star_rows=int(st3[2]), xoff=xo,
               rowoff=ro)
    return out
