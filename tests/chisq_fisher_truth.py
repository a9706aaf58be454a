"""Float64 CPU statement of the Fisher matrix of the continuum-marginalised fit, for the
tests of rvs_chisq_point_fisher.  Written from the definition, on the pieces of
tests/chisq_grad_truth.py (template, spline, orthonormal basis), not from the device code:

  per arm   m(theta)  the model row, theta = (vel, *params): template -> [broadening]
                      -> natural spline at lam * sqrt((1 - b) / (1 + b)), b = vel / c
            Jm        = dm/dtheta [npix, K] from torch.autograd.functional.jacobian
            ST        = phi m / e, c the least-squares continuum coefficients of D / e on
                      ST^T, s = c . phi the fitted continuum
            J         = Jm * (s / e)[:, None], the Jacobian of the whitened model
            projection by a QR of ST^T (never the normal equations):
            Jp        = J - U (U^T J), ST^T = U R;   F = Jp^T Jp,   G = J^T J
  summed over the arms whose outside flag is finite.

F is the expected information of the Gaussian likelihood marginalised over the continuum
coefficients (the Schur complement of the joint Fisher matrix), in the convention of
0.5 * (-2 log L): profiled_half_hessian() checks that against autograd's Hessian of the
profiled chi^2 with the data replaced by the fitted model, where the two are equal.
"""
import numpy as np
import torch

import chisq_grad_truth as truth

C_KMS = truth.C_KMS


def regular_template(lib, p, vsini):
    return truth.template(lib, p, vsini)


def tri_template(lib, p, vsini):
    """tri_grad_truth.template with the fixed broadening of chisq_grad_truth.template"""
    import tri_grad_truth as ttruth
    from oracle import rvs_oracle as orc
    t, outside = ttruth.template(lib, p)
    if t is not None and vsini is not None and vsini > 0:
        R = (vsini / C_KMS) / np.log(lib.lam[1] / lib.lam[0])
        if R >= 1e-9:
            ker = torch.as_tensor(orc.compute_vsini_kernel(R))
            k = (len(ker) - 1) // 2
            t = torch.nn.functional.conv1d(t[None, None, :], ker[None, None, :],
                                           padding=k)[0, 0]
    return t, outside


_rows = {}


def model_row(sd, lib, theta, vsini, template_fn):
    """(m [npix] as a torch function of theta = (vel, *params), outside flag)"""
    t, outside = template_fn(lib, theta[1:], vsini)
    if not np.isfinite(outside):
        return None, outside
    beta = theta[0] / C_KMS
    x = torch.as_tensor(sd.lam) * torch.sqrt((1 - beta) / (1 + beta))
    return truth.spline_eval(lib.lam, t, x), outside


def arm_fisher(sd, lib, vel, params, vsini, npoly, rbf=True,
               template_fn=regular_template):
    """dict(F, G [K, K], condA, s, m) of one arm, or None where the arm is skipped"""
    theta = torch.tensor([float(vel)] + [float(_) for _ in params], dtype=torch.float64)
    # (the model row and its Jacobian do not depend on the basis: once per job and arm)
    key = (template_fn.__name__, sd.name, np.asarray(sd.lam).tobytes(), float(vel),
           tuple(float(_) for _ in params), vsini)
    if key not in _rows:
        m, outside = model_row(sd, lib, theta, vsini, template_fn)
        if m is None:
            _rows[key] = None
        else:
            f = lambda th: model_row(sd, lib, th, vsini, template_fn)[0]  # noqa: E731
            _rows[key] = (m.numpy(),
                          torch.autograd.functional.jacobian(f, theta).numpy())
    if _rows[key] is None:
        return None
    m, Jm = _rows[key]                                              # [npix], [npix, K]
    Q, _ = truth.ortho_basis(sd.lam, npoly, rbf)
    Q = Q.numpy()
    e = np.asarray(sd.espec, dtype=np.float64)
    STt = (Q * (m / e)[None, :]).T                                  # [npix, P]
    U, R = np.linalg.qr(STt)
    c = np.linalg.solve(R, U.T @ (np.asarray(sd.spec, dtype=np.float64) / e))
    s = c @ Q
    J = Jm * (s / e)[:, None]
    Jp = J - U @ (U.T @ J)
    sv = np.linalg.svd(STt, compute_uv=False)
    return dict(F=Jp.T @ Jp, G=J.T @ J, condA=float((sv[0] / sv[-1])**2), s=s, m=m)


def fisher(sds, libs, vel, params, vsini=None, npoly=5, rbf=True,
           template_fn=regular_template):
    """(F, G, largest cond(A) of the arms that count) summed over the arms `sds`"""
    K = 1 + len(params)
    F, G, cond = np.zeros((K, K)), np.zeros((K, K)), 0.0
    for sd in sds:
        a = arm_fisher(sd, libs[sd.name], vel, params, vsini, npoly, rbf, template_fn)
        if a is None:
            continue
        F += a['F']
        G += a['G']
        cond = max(cond, a['condA'])
    return F, G, cond


def profiled_half_hessian(sds, libs, vel, params, vsini=None, npoly=5, rbf=True,
                          template_fn=regular_template):
    """0.5 * autograd's Hessian in theta of sum_arms (D.D - v.c), the profiled chi^2
    (chisq_grad_truth.marginal_chisq without its log-determinant terms), with the data
    of every arm replaced by its fitted model at (vel, params): D := s * m"""
    theta0 = torch.tensor([float(vel)] + [float(_) for _ in params],
                          dtype=torch.float64)
    arms = []
    for sd in sds:
        a = arm_fisher(sd, libs[sd.name], vel, params, vsini, npoly, rbf, template_fn)
        if a is None:
            continue
        Q, _ = truth.ortho_basis(sd.lam, npoly, rbf)
        e = torch.as_tensor(np.asarray(sd.espec, dtype=np.float64))
        arms.append((sd, Q, e, torch.as_tensor(a['s'] * a['m']) / e))

    def profiled(th):
        tot = 0.0 * th.sum()
        for sd, Q, e, Dn in arms:
            m = model_row(sd, libs[sd.name], th, vsini, template_fn)[0]
            ST = Q * (m / e)[None, :]
            v = ST @ Dn
            L = torch.linalg.cholesky(ST @ ST.T)
            tot = tot + Dn @ Dn - v @ torch.cholesky_solve(v[:, None], L)[:, 0]
        return tot
    return 0.5 * torch.autograd.functional.hessian(profiled, theta0).numpy()


_cache = {}


def truth_jobs(cases, libs, npoly, jobs=None, template_fn=regular_template, key='grid'):
    """[(F, G, condA)] of `jobs` (chisq_grad_truth.JOBS) at `npoly`, computed once"""
    jobs = truth.JOBS if jobs is None else jobs
    k = (key, npoly)
    if k not in _cache:
        from oracle import rvs_oracle as orc
        sp = truth.spectra(cases, orc.SpecData)
        _cache[k] = [fisher(sp[s], libs, v, p, vs, npoly=npoly, template_fn=template_fn)
                     for s, v, p, vs in jobs]
    return _cache[k]
