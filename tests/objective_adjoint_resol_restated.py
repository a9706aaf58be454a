"""Numpy restatement of the adjoint method of csrc/objective_grad.hip under banded
resolution matrices: tests/objective_adjoint_restated.py with the band
between the resampling and the pixels, and its transpose between the pixel adjoint and
the transposed resampling.  With raw_k the spline value at pixel k and R the arm's matrix
(scipy.sparse, or None: no matrix),

  model            m = R raw
  1  value and pixel adjoint    as there, on m: mbar_k = 2 (m_k/e_k^2) q_k - 2 r_k s_k/e_k
  1b band, transposed           rawbar = R^T mbar
                                d/dvel = sum_j rawbar_j S'(x_j) lam_j df/dvel
  2 .. 5                        as there, with rawbar in the place of mbar

The intermediates are returned (mbar, rawbar, ybar, zbar, u, tbar), so that a wrong stage
of the kernel can be located.  The pieces (template, taps, Thomas solve) are those of
objective_adjoint_restated."""
import numpy as np

import chisq_grad_truth as truth
import vsini_grad_truth as vtruth
import objective_adjoint_restated as adj

C_KMS = truth.C_KMS


def band(R, nd=None):
    """taps [npix, nd] of the matrix R as the kernel reads them: taps[k, d] =
    R[k, k - (nd - 1) / 2 + d], 0 outside the matrix; nd: the smallest odd number of
    diagonals that holds R unless given"""
    R = R.tocoo()
    keep = R.data != 0
    hb = int(np.abs(R.col[keep] - R.row[keep]).max())
    if nd is not None:
        assert nd % 2 == 1 and (nd - 1) // 2 >= hb
        hb = (nd - 1) // 2
    taps = np.zeros((R.shape[0], 2 * hb + 1))
    taps[R.row[keep], R.col[keep] - R.row[keep] + hb] = R.data[keep]
    return taps


def band_apply(taps, raw):
    """m_k = sum_d taps[k, d] raw[k - hb + d], d ascending, between loaded zeros"""
    npix, nd = taps.shape
    hb = (nd - 1) // 2
    pad = np.concatenate([np.zeros(hb), raw, np.zeros(hb)])
    m = np.zeros(npix)
    for d in range(nd):
        m = m + taps[:, d] * pad[d:d + npix]
    return m


def band_transposed(taps, mbar):
    """rawbar_j = sum_d taps[j + hb - d, d] mbar[j + hb - d], d ascending; a row outside
    [0, npix) meets a loaded zero"""
    npix, nd = taps.shape
    hb = (nd - 1) // 2
    pad = np.concatenate([np.zeros(hb), mbar, np.zeros(hb)])
    j = np.arange(npix)
    out = np.zeros(npix)
    for d in range(nd):
        row = np.clip(j + hb - d, 0, npix - 1)
        out = out + taps[row, d] * pad[j + 2 * hb - d]
    return out


def arm(sd, lib, R, vel, params, vsini, npoly, rbf=True, vsini_grad=False, t_row=None,
        x_ulps=0.0):
    """one arm under the matrix R (None: none): dict(value, grad [1 + ndim (+ 1)],
    outside, mbar, rawbar, ybar, zbar, u, tbar, raw, m); value None for a template with
    a non-finite outside flag.  t_row: the unbroadened template itself (the
    from-template form: no parameter components).  x_ulps: the pixels' template
    coordinates x = lam f moved by that many units in their last place -- what another
    float64 statement of the same product (a fused multiply-add, another rounding of f)
    may differ by; the rows' change under it is their conditioning, not an error"""
    nd = lib.ndim if t_row is None else 0
    K = 1 + nd + (1 if vsini_grad else 0)
    if t_row is None:
        t, tan, outside = adj.template_and_tangents(lib, params)
    else:
        t, tan, outside = np.asarray(t_row, dtype=np.float64), np.zeros((0, len(t_row))), 0.0
    if not np.isfinite(outside):
        return dict(value=None, grad=np.zeros(K), outside=outside)
    lam_t = np.asarray(lib.lam, dtype=np.float64)
    N = len(lam_t)
    h = np.diff(lam_t)
    w = dw = None
    if vsini is not None and vsini > 0:
        Rv = (vsini / C_KMS) / vtruth.lnstep(lib)
        if Rv >= 1e-9:
            w, dwdR = vtruth.taps(Rv)
            dw = dwdR / (C_KMS * vtruth.lnstep(lib))
    y = t if w is None else np.convolve(t, w, 'same')
    sl = np.diff(y) / h
    z = np.concatenate([[0.0], adj.thomas(h, 6.0 * np.diff(sl)), [0.0]])
    beta = vel / C_KMS
    f = np.sqrt((1 - beta) / (1 + beta))
    lam = np.asarray(sd.lam, dtype=np.float64)
    x = lam * f
    x = x + x_ulps * np.spacing(x)
    pos = np.clip(np.searchsorted(lam_t, x, 'right') - 1, 0, N - 2)
    dl, hh = x - lam_t[pos], h[pos]
    b = sl[pos] - hh * (2 * z[pos] + z[pos + 1]) / 6.0
    c2 = z[pos] / 2.0
    c3 = (z[pos + 1] - z[pos]) / (6.0 * hh)
    raw = y[pos] + dl * (b + dl * (c2 + dl * c3))
    draw = b + dl * (2 * c2 + 3 * c3 * dl)
    # the band
    taps = None if R is None else band(R)
    m = raw if taps is None else band_apply(taps, raw)
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
    # 1b: the band, transposed; the velocity component behind it
    rawbar = mbar if taps is None else band_transposed(taps, mbar)
    dfdv = -f / (C_KMS * (1 - beta * beta))
    grad = np.zeros(K)
    grad[0] = np.sum(rawbar * draw * lam * dfdv)
    # 2: resampling, transposed
    ybar, zbar = np.zeros(N), np.zeros(N)
    np.add.at(ybar, pos, rawbar * (1 - dl / hh))
    np.add.at(ybar, pos + 1, rawbar * dl / hh)
    np.add.at(zbar, pos, rawbar * (-dl * hh / 3 + dl**2 / 2 - dl**3 / (6 * hh)))
    np.add.at(zbar, pos + 1, rawbar * (-dl * hh / 6 + dl**3 / (6 * hh)))
    zbar = zbar[1:-1]
    # 3: spline, transposed
    u = adj.thomas(h, zbar)
    up = np.concatenate([[0.0], u, [0.0]])
    slb = 6 * (up[:-1] - up[1:])
    ybar[1:] += slb / h
    ybar[:-1] -= slb / h
    # 4: FIR, transposed
    tbar = ybar if w is None else np.convolve(ybar, w, 'same')
    # 5: contraction at the knots
    grad[1:1 + nd] = tan @ tbar
    if vsini_grad and dw is not None:
        grad[1 + nd] = np.convolve(ybar, dw, 'same') @ t
    return dict(value=value, grad=grad, outside=outside, mbar=mbar, rawbar=rawbar,
                ybar=ybar, zbar=zbar, u=u, tbar=tbar, t=t, y=y, z=z, raw=raw, m=m)


def chisq_and_grad(sds, libs, mats, vel, params, vsini=None, npoly=5, rbf=True,
                   vsini_grad=False, details=False):
    """get_chisq of the arms `sds` (oracle SpecData) under `mats` (one matrix or None per
    arm) and its gradient by (vel, *params[, vsini]); the penalties as
    tests/chisq_grad_resol_truth.py adds them"""
    badchi = 10 * sum(len(sd.lam) for sd in sds)
    tot, pen, grad, arms = 0.0, 0.0, 0.0, []
    for sd, R in zip(sds, mats):
        a = arm(sd, libs[sd.name], R, vel, params, vsini, npoly, rbf, vsini_grad)
        arms.append(a)
        if a['value'] is None:
            pen += 1000.0 * badchi
            continue
        pen += a['outside'] * badchi
        tot += a['value']
        grad = grad + a['grad']
    grad = np.zeros(1 + len(params) + (1 if vsini_grad else 0)) + grad
    return (tot + pen, grad, arms) if details else (tot + pen, grad)
