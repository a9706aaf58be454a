"""Numpy restatement of the adjoint method of csrc/objective_grad.hip:
value and gradient of the continuum-marginalised chi^2 of one arm with ONE adjoint row
carried from the pixels back to the knots.  Notation of DESIGN 4.12: t the gathered
template [ntp], y = w (*) t the broadened row, z the natural spline's second
derivatives, m_k the spline value at pixel k in knot interval pos, offset dl, width h.

  1  value and pixel adjoint   mbar_k = 2 (m_k/e_k^2) q_k - 2 r_k s_k/e_k,
                               q = |L^-1 phi|^2, s = c.phi, r = D/e - s m/e
                               d/dvel = sum_k mbar_k S'(x_k) lam_k df/dvel
  2  resampling, transposed    ybar[pos] += mbar (1 - dl/h), ybar[pos+1] += mbar dl/h,
                               zbar[pos] += mbar (-dl h/3 + dl^2/2 - dl^3/(6h)),
                               zbar[pos+1] += mbar (-dl h/6 + dl^3/(6h)); the boundary
                               entries of zbar are dropped (natural ends)
  3  spline, transposed        M u = zbar (Thomas), sl_j = 6 (u_{j-1} - u_j),
                               ybar_{j+1} += sl_j/h_j, ybar_j -= sl_j/h_j
  4  FIR, transposed           tbar = w (*) ybar, vbar = (dw/dvsini) (*) ybar
  5  contraction at the knots  d/dp_d = sum_n tbar_n t_n g_dn, d/dvsini = sum_n vbar_n t_n

The intermediates mbar, ybar, zbar, u, tbar are returned, so that a wrong stage of the
kernel can be located.  The template, its tangents and the taps are formed as
tests/chisq_grad_truth.py and tests/vsini_grad_truth.py form them."""
import numpy as np


import chisq_grad_truth as truth
import vsini_grad_truth as vtruth

C_KMS = truth.C_KMS


def thomas(h, rhs):
    """solve M x = rhs, M the symmetric tridiagonal matrix of the natural spline on
    the interior knots: rows (h_u, 2 (h_u + h_{u+1}), h_{u+1})"""
    n = len(rhs)
    cp, dp = np.zeros(n), np.zeros(n)
    c = d = 0.0
    for u in range(n):
        den = 2 * (h[u] + h[u + 1]) - h[u] * c
        c = h[u + 1] / den
        d = (rhs[u] - h[u] * d) / den
        cp[u], dp[u] = c, d
    x = np.zeros(n)
    nxt = 0.0
    for u in range(n - 1, -1, -1):
        nxt = dp[u] - (cp[u] * nxt if u < n - 1 else 0.0)
        x[u] = nxt
    return x


def template_and_tangents(lib, params):
    """(t [ntp], tangents dt/dp [ndim, ntp] per physical unit, outside); the tangents
    are zero in the nearest-neighbour modes"""
    p = np.asarray(params, dtype=np.float64)
    outside = float(lib.outside_flag(p))
    if outside != 0:
        t = np.asarray(lib.eval(p), dtype=np.float64)
        return t, np.zeros((lib.ndim, len(t))), outside
    mp = lib.map_params(p)
    pos = lib.cell(mp)
    ids = lib.idgrid[tuple((pos[None, :] + lib.edges).T)]
    rows = lib.dats[ids, :].astype(np.float64)
    x, dx = [], []
    for d in range(lib.ndim):
        u = lib.uvecs[d]
        wd = u[pos[d] + 1] - u[pos[d]]
        x.append((mp[d] - u[pos[d]]) / wd)
        dx.append((1.0 / (p[d] * np.log(10.0)) if d in lib.log_ids else 1.0) / wd)
    e = lib.edges.astype(np.float64)
    fac = [e[:, d] * x[d] + (1 - e[:, d]) * (1 - x[d]) for d in range(lib.ndim)]
    w = np.prod(fac, axis=0)
    t = np.exp(w @ rows)
    tan = []
    for d in range(lib.ndim):
        dw = (2 * e[:, d] - 1) * dx[d]
        for o in range(lib.ndim):
            if o != d:
                dw = dw * fac[o]
        tan.append(t * (dw @ rows))     # formed per knot, as the chain forms it
    return t, np.array(tan), outside


def arm(sd, lib, vel, params, vsini, npoly, rbf=True, vsini_grad=False):
    """one arm: dict(value, grad [1 + ndim (+ 1)], outside, mbar, ybar, zbar, u, tbar);
    value None for a template with a non-finite outside flag"""
    nd = lib.ndim
    K = 1 + nd + (1 if vsini_grad else 0)
    t, tan, outside = template_and_tangents(lib, params)
    if not np.isfinite(outside):
        return dict(value=None, grad=np.zeros(K), outside=outside)
    lam_t = np.asarray(lib.lam, dtype=np.float64)
    N = len(lam_t)
    h = np.diff(lam_t)
    # broadening
    w = dw = None
    if vsini is not None and vsini > 0:
        R = (vsini / C_KMS) / vtruth.lnstep(lib)
        if R >= 1e-9:
            w, dwdR = vtruth.taps(R)
            dw = dwdR / (C_KMS * vtruth.lnstep(lib))
    y = t if w is None else np.convolve(t, w, 'same')
    # spline
    sl = np.diff(y) / h
    z = np.concatenate([[0.0], thomas(h, 6.0 * np.diff(sl)), [0.0]])
    # resampling
    beta = vel / C_KMS
    f = np.sqrt((1 - beta) / (1 + beta))
    lam = np.asarray(sd.lam, dtype=np.float64)
    x = lam * f
    pos = np.clip(np.searchsorted(lam_t, x, 'right') - 1, 0, N - 2)
    dl, hh = x - lam_t[pos], h[pos]
    b = sl[pos] - hh * (2 * z[pos] + z[pos + 1]) / 6.0
    c2 = z[pos] / 2.0
    c3 = (z[pos + 1] - z[pos]) / (6.0 * hh)
    m = y[pos] + dl * (b + dl * (c2 + dl * c3))
    dm = b + dl * (2 * c2 + 3 * c3 * dl)
    # 1: value and pixel adjoint
    Q, const = truth.ortho_basis(sd.lam, npoly, rbf)
    Q = Q.numpy()
    e = np.asarray(sd.espec, dtype=np.float64)
    D = np.asarray(sd.spec, dtype=np.float64)
    ST = Q * (m / e)[None, :]
    A, v = ST @ ST.T, ST @ (D / e)
    L = np.linalg.cholesky(A)
    c = np.linalg.solve(L.T, np.linalg.solve(L, v))
    s = c @ Q
    r = D / e - s * m / e
    value = 2 * np.log(np.diag(L)).sum() + const + 2 * np.log(e).sum() + r @ r
    q = (np.linalg.solve(L, Q) ** 2).sum(0)
    mbar = 2 * (m / e**2) * q - 2 * r * s / e
    dfdv = -f / (C_KMS * (1 - beta * beta))
    grad = np.zeros(K)
    grad[0] = np.sum(mbar * dm * lam * dfdv)
    # 2: resampling, transposed
    ybar, zbar = np.zeros(N), np.zeros(N)
    np.add.at(ybar, pos, mbar * (1 - dl / hh))
    np.add.at(ybar, pos + 1, mbar * dl / hh)
    np.add.at(zbar, pos, mbar * (-dl * hh / 3 + dl**2 / 2 - dl**3 / (6 * hh)))
    np.add.at(zbar, pos + 1, mbar * (-dl * hh / 6 + dl**3 / (6 * hh)))
    zbar = zbar[1:-1]
    ybar_resampled = ybar.copy()
    # 3: spline, transposed
    u = thomas(h, zbar)
    up = np.concatenate([[0.0], u, [0.0]])      # up[j] = u_{j-1}
    slb = 6 * (up[:-1] - up[1:])                # sl_j, j = 0 .. N-2
    ybar[1:] += slb / h
    ybar[:-1] -= slb / h
    # 4: FIR, transposed (symmetric taps, zero-padded ends: the same FIR)
    tbar = ybar if w is None else np.convolve(ybar, w, 'same')
    # 5: contraction at the knots
    grad[1:1 + nd] = tan @ tbar
    if vsini_grad and dw is not None:
        grad[1 + nd] = np.convolve(ybar, dw, 'same') @ t
    return dict(value=value, grad=grad, outside=outside, mbar=mbar,
                ybar_resampled=ybar_resampled, ybar=ybar, zbar=zbar, u=u, tbar=tbar,
                t=t, y=y, z=z, m=m)


def chisq_and_grad(sds, libs, vel, params, vsini=None, npoly=5, rbf=True,
                   vsini_grad=False, details=False):
    """get_chisq of the arms `sds` (oracle SpecData) and its gradient by (vel, *params
    [, vsini]); the penalties as tests/chisq_grad_truth.py adds them"""
    badchi = 10 * sum(len(sd.lam) for sd in sds)
    tot, pen, grad, arms = 0.0, 0.0, 0.0, []
    for sd in sds:
        a = arm(sd, libs[sd.name], vel, params, vsini, npoly, rbf, vsini_grad)
        arms.append(a)
        if a['value'] is None:
            pen += 1000.0 * badchi
            continue
        pen += a['outside'] * badchi
        tot += a['value']
        grad = grad + a['grad']
    grad = np.zeros(1 + len(params) + (1 if vsini_grad else 0)) + grad
    return (tot + pen, grad, arms) if details else (tot + pen, grad)
