"""Float64 CPU statement, in torch, of the template of a Delaunay library as a
differentiable function of the stellar parameters, and with it of the
continuum-marginalised chi^2 of tests/chisq_grad_truth.py on such libraries, for the
tests of the analytic gradient.  Written from the formulas, not from the device code:

  template   inside the simplex that holds the mapped query q (log10 of the library's
             log_ids parameters) the barycentric coordinates are b = T (q - r) for the
             first ndim vertices and b_ndim = 1 - sum_i b_i for the last, T and r the
             simplex's rows of scipy's Delaunay.transform; t(p) = exp(b @ rows), rows
             the log-flux rows of the simplex's ndim + 1 vertices (b @ rows itself
             for a library whose rows are not logarithms)
  outside    the same blend of the vertices' extraflags (a number, not differentiated);
             no simplex (outside the hull, a non-finite mapped parameter): NaN
  the rest   broadening, spline, marginal chi^2: chisq_grad_truth / vsini_grad_truth

The gradient is torch.autograd's.  The simplex index is piecewise constant and is taken
outside the graph, from the oracle's exhaustive search.
"""
import os

import numpy as np
import torch

from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import vsini_grad_truth as vtruth
from chisq_grad_truth import marginal_chisq, ortho_basis, spline_eval

C_KMS = truth.C_KMS
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def tri_lib_dict(n):
    """converted artefact of a golden Delaunay setup (ndim 4, 270 nodes, 5718
    simplices; ntp 977 for gold_b, 781 for gold_r)"""
    return dict(np.load(os.path.join(GOLD, 'lib_tri_%s.npz' % n)))


def oracle_libs():
    return {n: orc.TriLibrary(tri_lib_dict(n)) for n in ('gold_b', 'gold_r')}


def barycentric(lib, p):
    """(simplex id or -1, b [ndim + 1] as a torch function of p)"""
    xid = lib.find_simplex(lib.map_params(p.detach().numpy()))
    if xid == -1:
        return -1, None
    nd = lib.ndim
    q = torch.stack([torch.log10(p[d]) if d in lib.log_ids else p[d]
                     for d in range(nd)])
    T = torch.as_tensor(lib.transform[xid, :nd, :])
    r = torch.as_tensor(lib.transform[xid, nd, :])
    b = T @ (q - r)
    return xid, torch.cat([b, (1.0 - b.sum())[None]])


def template(lib, p):
    """(unbroadened template [ntp] as a torch function of the float64 tensor p [ndim],
    outside flag); (None, nan) where no simplex holds the point"""
    xid, b = barycentric(lib, p)
    if xid == -1:
        return None, float('nan')
    ids = lib.simplices[xid]
    t = b @ torch.as_tensor(lib.dats[ids, :])
    if lib.exp:
        t = torch.exp(t)
    outside = float(b.detach().numpy() @ lib.extraflags[ids])
    return t, outside


def template_jacobian(lib, params):
    """(t [ntp], dt/dp [ndim, ntp]) of the unbroadened template"""
    p = torch.tensor([float(_) for _ in params], dtype=torch.float64)
    f = lambda q: template(lib, q)[0]
    jac = [torch.autograd.functional.jvp(f, p, e)[1].numpy()
           for e in torch.eye(len(p), dtype=torch.float64)]
    return f(p).numpy(), np.array(jac)


def chisq_and_grad(sds, libs, vel, params, vsini=None, npoly=5, rbf=True,
                   outside_penalty=True, vsini_grad=False):
    """get_chisq of the arms `sds` (oracle SpecData) on the Delaunay libraries `libs`
    and its gradient with respect to (vel, *params), or (vel, *params, vsini) with
    vsini_grad: (float, ndarray).  Penalties as get_chisq adds them
    (spec_fit.py:888-896); they are not differentiated."""
    x = [float(vel)] + [float(_) for _ in params]
    if vsini_grad:
        x.append(float(vsini))
    theta = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    nd = len(params)
    badchi = 10 * sum(len(sd.lam) for sd in sds)
    tot = 0.0 * theta.sum()
    pen = 0.0
    for sd in sds:
        lib = libs[sd.name]
        t, outside = template(lib, theta[1:1 + nd])
        if not np.isfinite(outside):
            pen += 1000.0 * badchi
            continue
        if outside_penalty:
            pen += outside * badchi
        if vsini_grad:
            t = vtruth.broadened(lib, t, theta[-1])
        elif vsini is not None and vsini > 0:
            R = (vsini / C_KMS) / np.log(lib.lam[1] / lib.lam[0])
            if R >= 1e-9:
                ker = torch.as_tensor(orc.compute_vsini_kernel(R))
                k = (len(ker) - 1) // 2
                t = torch.nn.functional.conv1d(t[None, None, :], ker[None, None, :],
                                               padding=k)[0, 0]
        beta = theta[0] / C_KMS
        xs = torch.as_tensor(sd.lam) * torch.sqrt((1 - beta) / (1 + beta))
        m = spline_eval(lib.lam, t, xs)
        Q, const = ortho_basis(sd.lam, npoly, rbf)
        tot = tot + marginal_chisq(m, Q, const, torch.as_tensor(sd.spec),
                                   torch.as_tensor(sd.espec))
    tot.backward()
    return float(tot.item()) + pen, theta.grad.numpy().copy()


# ---- the shared cases of the gradient tests -----------------------------------
# (spectrum of chisq_grad_truth.SPECTRA, vel, (teff, logg, feh, alpha), vsini).  The two
# golden arms share one triangulation, so a query has the same simplex and the same
# barycentric coordinates on both.  Jobs 0-5 lie inside a simplex with every coordinate
# >= MIN_BARY (the smallest: 0.112, 0.074, 0.061, 0.029, 0.050, 0.028); job 3 is
# broadened; job 6 lies outside the hull (no simplex); job 7 has a non-finite mapped
# parameter (log10 of a negative teff)
MIN_BARY = 0.01
JOBS = [
    (0, -212.7, (6000.0, 2.5, -0.4, 0.1), None),
    (1, 5.5, (6900.0, 1.5, -0.2, 0.05), None),
    (2, 37.3, (5000.0, 2.2, -1.0, 0.2), None),
    (0, -209.49, (6123.0, 2.5, -0.4, 0.1), 30.0),
    (1, 8.71, (6500.0, 3.6, -0.3, 0.12), None),
    (2, 20.0, (6200.0, 2.9, -0.9, 0.22), None),
    (2, 100.0, (8000.0, 5.0, 0.5, 0.6), None),
    (0, 12.5, (-100.0, 2.0, -1.0, 0.2), None),
]
INSIDE = [0, 1, 2, 3, 4, 5]
BROADENED = 3
NO_SIMPLEX = 6
NONFINITE = 7

spectra = truth.spectra

_truth_cache = {}


def truth_jobs(cases, libs, npoly):
    """[(value, grad [1 + ndim])] of JOBS at `npoly` (rbf basis), once per npoly"""
    if npoly not in _truth_cache:
        sp = spectra(cases, orc.SpecData)
        _truth_cache[npoly] = [chisq_and_grad(sp[s], libs, v, p, vs, npoly=npoly)
                               for s, v, p, vs in JOBS]
    return _truth_cache[npoly]
