"""Float64 CPU statement of the continuum-marginalised chi^2, its gradient and the Fisher
matrix of the fit under banded resolution matrices, for the tests of
rvs_chisq_point_grad_resol / rvs_chisq_point_fisher_resol.  Built from the pieces of
tests/chisq_grad_truth.py, tests/vsini_grad_truth.py and tests/chisq_fisher_truth.py
(template, broadening, spline, orthonormal basis, marginal chi^2, QR projection), not
from the device code.  With R the matrix of an arm (None: no matrix),

  model row    m = R @ spline_eval(template, lam * sqrt((1 - b) / (1 + b)))
  gradient     torch.autograd's of marginal_chisq(m, ...)
  Fisher       Jm = R @ d(spline row)/dtheta, then chisq_fisher_truth's projection

R is a dense float64 matrix here (the arms have 401 and 301 pixels).
"""
import numpy as np
import torch

from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import vsini_grad_truth as vtruth

C_KMS = truth.C_KMS


def width(job, arm):
    """Gaussian sigma (Angstrom) of the matrix of `job` on arm number `arm`: 9 ... 25
    diagonals on the golden arms, so that the band crosses pixel 256"""
    return 0.5 + 0.3 * job + 0.2 * arm


def matrices(sds, job, cls=orc):
    """the arms' matrices of `job` (cls.construct_resol_mat: scipy.sparse from the
    oracle, ResolMatrix from the package)"""
    return [cls.construct_resol_mat(sd.lam, width=width(job, ia))
            for ia, sd in enumerate(sds)]


def dense(R):
    return None if R is None else torch.as_tensor(np.asarray(R.todense(),
                                                             dtype=np.float64))


def ndiag(R):
    """the number of diagonals engine.resol_taps gives the matrix"""
    R = R.tocoo()
    keep = R.data != 0
    return 2 * int(np.abs(R.col[keep] - R.row[keep]).max()) + 1


def model_row(sd, lib, theta, vsini, R, vsini_fit=False):
    """(m [npix] as a torch function of theta = (vel, *params[, vsini]), outside flag);
    vsini_fit: vsini is theta's last entry (vsini_grad_truth.broadened)"""
    if vsini_fit:
        t, outside = truth.template(lib, theta[1:-1])
        if np.isfinite(outside):
            t = vtruth.broadened(lib, t, theta[-1])
    else:
        t, outside = truth.template(lib, theta[1:], vsini)
    if not np.isfinite(outside):
        return None, outside
    beta = theta[0] / C_KMS
    x = torch.as_tensor(sd.lam) * torch.sqrt((1 - beta) / (1 + beta))
    m = truth.spline_eval(lib.lam, t, x)
    return (m if R is None else R @ m), outside


def _theta(vel, params, vsini, vsini_fit):
    return [float(vel)] + [float(_) for _ in params] + \
        ([float(vsini)] if vsini_fit else [])


def chisq_and_grad(sds, libs, mats, vel, params, vsini=None, npoly=5, rbf=True,
                   outside_penalty=True, vsini_fit=False):
    """get_chisq of the arms `sds` under `mats` and its gradient with respect to
    (vel, *params[, vsini]): (float, ndarray).  Penalties as get_chisq adds them; they
    are not differentiated."""
    theta = torch.tensor(_theta(vel, params, vsini, vsini_fit), dtype=torch.float64,
                         requires_grad=True)
    badchi = 10 * sum(len(sd.lam) for sd in sds)
    tot = 0.0 * theta.sum()
    pen = 0.0
    for sd, R in zip(sds, mats):
        m, outside = model_row(sd, libs[sd.name], theta, vsini, dense(R), vsini_fit)
        if m is None:
            pen += 1000.0 * badchi
            continue
        if outside_penalty:
            pen += outside * badchi
        Q, const = truth.ortho_basis(sd.lam, npoly, rbf)
        tot = tot + truth.marginal_chisq(m, Q, const, torch.as_tensor(sd.spec),
                                         torch.as_tensor(sd.espec))
    tot.backward()
    return float(tot.item()) + pen, theta.grad.numpy().copy()


_rows = {}


def fisher(sds, libs, mats, vel, params, vsini=None, npoly=5, rbf=True,
           vsini_fit=False, key=None):
    """(F, G, largest cond(A)) summed over the arms, as chisq_fisher_truth.fisher;
    `key` (hashable) names (sds, mats) so that the model rows and their Jacobians, which
    do not depend on the basis, are computed once"""
    th = _theta(vel, params, vsini, vsini_fit)
    K = len(th)
    F, G, cond = np.zeros((K, K)), np.zeros((K, K)), 0.0
    for ia, (sd, R) in enumerate(zip(sds, mats)):
        lib = libs[sd.name]
        k = None if key is None else (key, ia, tuple(th), vsini, vsini_fit)
        if k is None or k not in _rows:
            theta = torch.tensor(th, dtype=torch.float64)
            Rd = dense(R)
            m, outside = model_row(sd, lib, theta, vsini, Rd, vsini_fit)
            row = None
            if m is not None:
                f = lambda q: model_row(sd, lib, q, vsini, Rd, vsini_fit)[0]  # noqa
                row = (m.numpy(), torch.autograd.functional.jacobian(f, theta).numpy())
            if k is None:
                rowk = row
            else:
                _rows[k] = rowk = row
        else:
            rowk = _rows[k]
        if rowk is None:
            continue
        m, Jm = rowk
        Q = truth.ortho_basis(sd.lam, npoly, rbf)[0].numpy()
        e = np.asarray(sd.espec, dtype=np.float64)
        STt = (Q * (m / e)[None, :]).T
        U, Rq = np.linalg.qr(STt)
        c = np.linalg.solve(Rq, U.T @ (np.asarray(sd.spec, dtype=np.float64) / e))
        s = c @ Q
        J = Jm * (s / e)[:, None]
        Jp = J - U @ (U.T @ J)
        sv = np.linalg.svd(STt, compute_uv=False)
        F += Jp.T @ Jp
        G += J.T @ J
        cond = max(cond, float((sv[0] / sv[-1])**2))
    return F, G, cond
