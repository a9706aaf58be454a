"""Numpy restatement of the forward-mode method of csrc/objective_fisher.hip (DESIGN
4.23): value, gradient and Fisher matrix of the continuum-marginalised fit of one arm
with the K = 1 + ndim (+ 1) tangent rows taken, one at a time, through the value's own
linear path.  Notation of DESIGN 4.12 / 4.15 and of tests/objective_adjoint_restated.py
(whose template, tangents at the knots and Thomas solve are used here):

  value          t -> y = w (*) t -> z (natural spline) -> m_k; ST = phi m / e,
                 A = ST ST^T = L L^T, c = A^-1 ST D/e, s = c.phi, r = D/e - s m/e
  pixel adjoint  mbar_k = 2 (m_k/e_k^2) q_k - 2 r_k s_k/e_k, q = |L^-1 phi|^2; te = m/e
  tangents       knots:  t'_0 = -, t'_d = t sum_v (dw_v/dp_d) L_v, t'_vsini = t
                 FIR:    y'_d = w (*) t'_d,  y'_vsini = (dw/dvsini) (*) t
                 spline: z'_i of y'_i
                 pixels: m'_k0 = S'(x_k) lam_k df/dvel, m'_ki = the spline of y'_i at x_k
  moments        J_ki = s_k m'_ki / e_k;  B'_pi = sum_k phi_pk te_k J_ki;
                 B = L^-1 B' (= sum_k y_p(k) te_k J_ki, y = L^-1 phi, by linearity)
  sums           G = J^T J,  F = G - B^T B,  g_i = sum_k mbar_k m'_ki

The intermediates are returned, so that a wrong stage of the kernel can be located.  Also
here: the truth of tests/chisq_fisher_truth.py with vsini as one more, last, parameter
(autograd Jacobian, QR projection), which that module has no form for.  No tests here."""
import numpy as np
import torch

import chisq_grad_truth as truth
import chisq_fisher_truth as ftruth
import objective_adjoint_restated as adj
import vsini_grad_truth as vtruth

C_KMS = truth.C_KMS


def _spline_at(lam_t, h, y, pos, dl):
    """(value, derivative) at the pixels of the natural spline through y"""
    sl = np.diff(y) / h
    z = np.concatenate([[0.0], adj.thomas(h, 6.0 * np.diff(sl)), [0.0]])
    hh = h[pos]
    b = sl[pos] - hh * (2 * z[pos] + z[pos + 1]) / 6.0
    c2 = z[pos] / 2.0
    c3 = (z[pos + 1] - z[pos]) / (6.0 * hh)
    return y[pos] + dl * (b + dl * (c2 + dl * c3)), b + dl * (2 * c2 + 3 * c3 * dl), z


def arm(sd, lib, vel, params, vsini, npoly, rbf=True, vsini_grad=False):
    """one arm: dict(value, grad [K], fisher, gram [K, K], outside and the intermediates
    tknots, yknots, zknots [K, ntp] (row 0 unused), mdot [npix, K], J, Bp, B [P, K]);
    value None for a template with a non-finite outside flag"""
    nd = lib.ndim
    K = 1 + nd + (1 if vsini_grad else 0)
    t, tan, outside = adj.template_and_tangents(lib, params)
    if not np.isfinite(outside):
        return dict(value=None, grad=np.zeros(K), fisher=np.zeros((K, K)),
                    gram=np.zeros((K, K)), outside=outside)
    lam_t = np.asarray(lib.lam, dtype=np.float64)
    N = len(lam_t)
    h = np.diff(lam_t)
    w = dw = None
    if vsini is not None and vsini > 0:
        R = (vsini / C_KMS) / vtruth.lnstep(lib)
        if R >= 1e-9:
            w, dwdR = vtruth.taps(R)
            dw = dwdR / (C_KMS * vtruth.lnstep(lib))
    fir = (lambda row: row) if w is None else (lambda row: np.convolve(row, w, 'same'))
    beta = vel / C_KMS
    f = np.sqrt((1 - beta) / (1 + beta))
    dfdv = -f / (C_KMS * (1 - beta * beta))
    lam = np.asarray(sd.lam, dtype=np.float64)
    x = lam * f
    pos = np.clip(np.searchsorted(lam_t, x, 'right') - 1, 0, N - 2)
    dl = x - lam_t[pos]
    # value
    y = fir(t)
    m, dm, z = _spline_at(lam_t, h, y, pos, dl)
    Q, const = truth.ortho_basis(sd.lam, npoly, rbf)
    Q = Q.numpy()
    e = np.asarray(sd.espec, dtype=np.float64)
    D = np.asarray(sd.spec, dtype=np.float64)
    te = m / e
    ST = Q * te[None, :]
    A, v = ST @ ST.T, ST @ (D / e)
    L = np.linalg.cholesky(A)
    c = np.linalg.solve(L.T, np.linalg.solve(L, v))
    s = c @ Q
    r = D / e - s * te
    value = 2 * np.log(np.diag(L)).sum() + const + 2 * np.log(e).sum() + r @ r
    q = (np.linalg.solve(L, Q) ** 2).sum(0)
    mbar = 2 * (m / e**2) * q - 2 * r * s / e
    # tangents: knots, FIR, spline, pixels
    tk, yk, zk = np.zeros((K, N)), np.zeros((K, N)), np.zeros((K, N))
    mdot = np.zeros((len(lam), K))
    mdot[:, 0] = dm * lam * dfdv
    for d in range(nd):
        tk[1 + d] = tan[d]
        yk[1 + d] = fir(tan[d])
    if vsini_grad and dw is not None:
        tk[1 + nd] = t
        yk[1 + nd] = np.convolve(t, dw, 'same')
    for i in range(1, K):
        mdot[:, i], _, zk[i] = _spline_at(lam_t, h, yk[i], pos, dl)
    # moments and sums
    J = mdot * (s / e)[:, None]
    Bp = (Q * te[None, :]) @ J                      # [P, K]
    B = np.linalg.solve(L, Bp)
    G = J.T @ J
    F = G - B.T @ B
    F = 0.5 * (F + F.T)
    return dict(value=value, grad=mbar @ mdot, fisher=F, gram=G, outside=outside,
                tknots=tk, yknots=yk, zknots=zk, mdot=mdot, J=J, Bp=Bp, B=B, mbar=mbar,
                te=te, m=m, y=y, z=z, t=t)


def value_grad_fisher(sds, libs, vel, params, vsini=None, npoly=5, rbf=True,
                      vsini_grad=False, details=False):
    """(value, grad [K], F [K, K], G [K, K]) of the arms `sds` (oracle SpecData); the
    penalties as tests/chisq_grad_truth.py adds them, on the value only"""
    K = 1 + len(params) + (1 if vsini_grad else 0)
    badchi = 10 * sum(len(sd.lam) for sd in sds)
    tot, pen, arms = 0.0, 0.0, []
    grad, F, G = np.zeros(K), np.zeros((K, K)), np.zeros((K, K))
    for sd in sds:
        a = arm(sd, libs[sd.name], vel, params, vsini, npoly, rbf, vsini_grad)
        arms.append(a)
        if a['value'] is None:
            pen += 1000.0 * badchi
            continue
        pen += a['outside'] * badchi
        tot += a['value']
        grad += a['grad']
        F += a['fisher']
        G += a['gram']
    return (tot + pen, grad, F, G, arms) if details else (tot + pen, grad, F, G)


# ---- the truth with the vsini column ----------------------------------------------------
def _model_row_vsini(sd, lib, theta):
    """m [npix] as a torch function of theta = (vel, *params, vsini)"""
    t, outside = truth.template(lib, theta[1:-1])
    if not np.isfinite(outside):
        return None
    t = vtruth.broadened(lib, t, theta[-1])
    beta = theta[0] / C_KMS
    x = torch.as_tensor(sd.lam) * torch.sqrt((1 - beta) / (1 + beta))
    return truth.spline_eval(lib.lam, t, x)


_jac_cache = {}


def _project(sd, m, Jm, npoly, rbf):
    """(F, G, cond(A)) of one arm from its model row and the row's Jacobian, as
    chisq_fisher_truth.arm_fisher forms them"""
    Q = truth.ortho_basis(sd.lam, npoly, rbf)[0].numpy()
    e = np.asarray(sd.espec, dtype=np.float64)
    STt = (Q * (m / e)[None, :]).T
    U, R = np.linalg.qr(STt)
    c = np.linalg.solve(R, U.T @ (np.asarray(sd.spec, dtype=np.float64) / e))
    Jw = Jm * ((c @ Q) / e)[:, None]
    Jp = Jw - U @ (U.T @ Jw)
    sv = np.linalg.svd(STt, compute_uv=False)
    return Jp.T @ Jp, Jw.T @ Jw, float((sv[0] / sv[-1])**2)


def fisher_truth(sds, libs, vel, params, vsini=None, npoly=5, rbf=True,
                 vsini_grad=False):
    """(F, G, largest cond(A)) by tests/chisq_fisher_truth.py's definition (autograd
    Jacobian of the model row, QR projection); with vsini_grad theta = (vel, *params,
    vsini), the vsini column per km/s (zero where the broadening is not applied)"""
    if not vsini_grad:
        return ftruth.fisher(sds, libs, vel, params, vsini, npoly=npoly, rbf=rbf)
    theta = torch.tensor([float(vel)] + [float(_) for _ in params] +
                         [float(vsini or 0.0)], dtype=torch.float64)
    K = len(theta)
    F, G, cond = np.zeros((K, K)), np.zeros((K, K)), 0.0
    for sd in sds:
        lib = libs[sd.name]
        key = (sd.name, np.asarray(sd.lam).tobytes(), len(lib.lam), float(lib.lam[0]),
               float(lib.lam[-1]), tuple(theta.tolist()))
        if key not in _jac_cache:
            m = _model_row_vsini(sd, lib, theta)
            _jac_cache[key] = None if m is None else (
                m.numpy(), torch.autograd.functional.jacobian(
                    lambda th: _model_row_vsini(sd, lib, th), theta).numpy())
        if _jac_cache[key] is None:
            continue
        a = _project(sd, *_jac_cache[key], npoly, rbf)
        F += a[0]
        G += a[1]
        cond = max(cond, a[2])
    return F, G, cond


_col_cache = {}


def model_columns(sd, lib, vel, params, vsini, vsini_grad):
    """(m [npix], dm/dtheta [npix, K], outside) of one arm WITHOUT a Jacobian of npix
    backward passes, for the shapes of tests/objective_grad_shapes.py (thousands of
    pixels on thousands of knots): the path from the template row to the model row is
    linear, so a column is the truth's own path applied to the template's tangent --
    autograd's dt/dp_d (chisq_grad_truth.template_jacobian) through the same fixed
    broadening and truth.spline_eval; the velocity column is autograd's dm/dx (one
    backward pass: m_k depends on x_k alone) times lam df/dvel; the vsini column is the
    spline of (dw/dvsini) (*) t with the taps' derivative of vsini_grad_truth.taps.
    test_objective_fisher_cpu.py pins this to the autograd Jacobian on the golden jobs."""
    key = (sd.name, np.asarray(sd.lam).tobytes(), len(lib.lam), float(lib.lam[0]),
           float(lib.lam[-1]), float(vel), tuple(float(_) for _ in params), vsini,
           vsini_grad, truth.BANDED_ABOVE)
    if key in _col_cache:
        return _col_cache[key]
    p = torch.tensor([float(_) for _ in params], dtype=torch.float64)
    t, outside = truth.template(lib, p)
    if not np.isfinite(outside):
        _col_cache[key] = (None, None, outside)
        return _col_cache[key]
    nd = len(p)
    K = 1 + nd + (1 if vsini_grad else 0)
    tan = truth.template_jacobian(lib, params)[1] if outside == 0 else \
        np.zeros((nd, len(lib.lam)))
    w = dw = None
    if vsini is not None and vsini > 0:
        R = (vsini / C_KMS) / vtruth.lnstep(lib)
        if R >= 1e-9:
            w, dwdR = vtruth.taps(R)
            dw = dwdR / (C_KMS * vtruth.lnstep(lib))
    fir = (lambda row: row) if w is None else (lambda row: np.convolve(row, w, 'same'))
    beta = vel / C_KMS
    f = np.sqrt((1 - beta) / (1 + beta))
    dfdv = -f / (C_KMS * (1 - beta * beta))
    lam = np.asarray(sd.lam, dtype=np.float64)
    x = torch.tensor(lam * f, requires_grad=True)
    tn = t.detach().numpy()
    m = truth.spline_eval(lib.lam, torch.as_tensor(fir(tn)), x)
    m.sum().backward()
    Jm = np.zeros((len(lam), K))
    Jm[:, 0] = x.grad.numpy() * lam * dfdv
    xc = x.detach()
    for d in range(nd):
        Jm[:, 1 + d] = truth.spline_eval(lib.lam, torch.as_tensor(fir(tan[d])),
                                         xc).numpy()
    if vsini_grad and dw is not None:
        Jm[:, 1 + nd] = truth.spline_eval(
            lib.lam, torch.as_tensor(np.convolve(tn, dw, 'same')), xc).numpy()
    _col_cache[key] = (m.detach().numpy(), Jm, outside)
    return _col_cache[key]


def fisher_truth_columns(sds, libs, vel, params, vsini=None, npoly=5, rbf=True,
                         vsini_grad=False):
    """(F, G, largest cond(A)) as fisher_truth forms them (QR projection, never the
    normal equations), the Jacobian of the model row from model_columns"""
    K = 1 + len(params) + (1 if vsini_grad else 0)
    F, G, cond = np.zeros((K, K)), np.zeros((K, K)), 0.0
    for sd in sds:
        m, Jm, outside = model_columns(sd, libs[sd.name], vel, params, vsini, vsini_grad)
        if m is None:
            continue
        a = _project(sd, m, Jm, npoly, rbf)
        F += a[0]
        G += a[1]
        cond = max(cond, a[2])
    return F, G, cond


def rel_fisher(F, Ft, G):
    """the project's measure for these sums: |F - Ft|_il / sqrt(G_ii G_ll); an entry of a
    row that is exactly zero in G counts where it differs at all"""
    g = np.sqrt(np.diag(G))
    den = g[:, None] * g[None, :]
    d = np.abs(np.asarray(F) - Ft)
    return np.where(den > 0, d / np.where(den > 0, den, 1.0), np.where(d > 0, np.inf, 0.0))
