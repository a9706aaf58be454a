"""Float64 CPU statement, in torch, of the continuum-marginalised chi^2 of one arm as
a differentiable function of (velocity, stellar parameters), for the tests of the
analytic gradient.  Written from the formulas, not from the device code:

  template   t(p) = exp(sum_S w_S(p) L_S), polylinear weights of the mapped
             parameters (log10 for the library's log_ids) inside the query's cell;
             outside the grid / on a cell with a missing vertex the evaluator's
             nearest-neighbour row, which does not depend on p
  broadening 'same' convolution with the oracle's rotational kernel (vsini fixed)
  spline     natural cubic spline through the knots by a DENSE solve for the second
             derivatives, evaluated at lam * sqrt((1 - b) / (1 + b)), b = vel / c
  chi^2      ST = phi m / e, A = ST ST^T, v = ST D, c = A^-1 v (torch.linalg.cholesky),
             chi^2 = log det A + 2 sum log e + D.D - v.c, phi the orthonormalised
             continuum basis (phi^T = Q of a QR; the constant 2 log|det R| is added)

The gradient is torch.autograd's.  The pixel -> knot-interval index and the grid cell
are piecewise constant and are taken outside the graph.
"""
import numpy as np
import torch

from oracle import rvs_oracle as orc

C_KMS = orc.SPEED_OF_LIGHT
_spline_inv = {}


def _spline_matrix_inverse(lam):
    """inverse of the (N-2) x (N-2) tridiagonal system of the natural spline's interior
    second derivatives; a constant of the knots"""
    key = (len(lam), lam[:2].tobytes(), lam[-1:].tobytes())
    if key not in _spline_inv:
        h = np.diff(lam)
        n = len(lam) - 2
        M = np.zeros((n, n))
        i = np.arange(n)
        M[i, i] = 2 * (h[:-1] + h[1:])
        M[i[:-1], i[:-1] + 1] = h[1:-1]
        M[i[1:], i[1:] - 1] = h[1:-1]
        _spline_inv[key] = torch.as_tensor(np.linalg.inv(M))
    return _spline_inv[key]


# knot sets longer than this take the banded solve below; None: always the dense
# inverse (what every caller gets that does not ask: see banded_spline)
BANDED_ABOVE = None


class banded_spline:
    """with banded_spline(n): spline_eval solves knot sets of more than n knots by
    scipy.linalg.solveh_banded instead of the dense inverse (2-7 s and 340 MB per set of
    ~6000 knots).  The same symmetric system, the same second derivatives to rounding
    (tests/test_objective_grad_shapes_cpu.py pins one to the other at 977 knots)."""

    def __init__(self, above=2000):
        self.above = above

    def __enter__(self):
        global BANDED_ABOVE
        self.keep, BANDED_ABOVE = BANDED_ABOVE, self.above

    def __exit__(self, *exc):
        global BANDED_ABOVE
        BANDED_ABOVE = self.keep


class _BandedSolve(torch.autograd.Function):
    """x = M^-1 rhs, M the symmetric positive definite tridiagonal matrix of
    _spline_matrix_inverse in upper banded storage `ab` [2, n] (a constant); M is
    symmetric, so the backward pass is the same solve"""

    @staticmethod
    def forward(ctx, ab, rhs):
        from scipy.linalg import solveh_banded
        ctx.ab = ab
        return torch.as_tensor(solveh_banded(ab, rhs.detach().numpy()))

    @staticmethod
    def backward(ctx, g):
        from scipy.linalg import solveh_banded
        return None, torch.as_tensor(solveh_banded(ctx.ab, g.detach().numpy()))


def _spline_banded(lam):
    h = np.diff(lam)
    ab = np.zeros((2, len(lam) - 2))
    ab[1] = 2 * (h[:-1] + h[1:])
    ab[0, 1:] = h[1:-1]
    return ab


def template(lib, p, vsini=None):
    """(template [ntp] as a torch function of the float64 tensor p [ndim], outside)"""
    pn = p.detach().numpy()
    outside = float(lib.outside_flag(pn))
    if outside != 0:
        t = torch.as_tensor(lib.eval(pn)) + 0.0 * p.sum()
        if not np.isfinite(outside):
            return t, outside
    else:
        mp = lib.map_params(pn)
        pos = lib.cell(mp)
        ids = lib.idgrid[tuple((pos[None, :] + lib.edges).T)]
        rows = torch.as_tensor(lib.dats[ids, :].astype(np.float64))
        x = []
        for d in range(lib.ndim):
            u = lib.uvecs[d]
            q = torch.log10(p[d]) if d in lib.log_ids else p[d]
            x.append((q - u[pos[d]]) / (u[pos[d] + 1] - u[pos[d]]))
        w = torch.ones(len(ids), dtype=torch.float64)
        edges = lib.edges
        for d in range(lib.ndim):
            e = torch.as_tensor(edges[:, d].astype(np.float64))
            w = w * (e * x[d] + (1 - e) * (1 - x[d]))
        t = torch.exp(w @ rows)
    if vsini is not None and vsini > 0:
        R = (vsini / C_KMS) / np.log(lib.lam[1] / lib.lam[0])
        if R >= 1e-9:
            ker = torch.as_tensor(orc.compute_vsini_kernel(R))
            k = (len(ker) - 1) // 2
            t = torch.nn.functional.conv1d(t[None, None, :], ker[None, None, :],
                                           padding=k)[0, 0]
    return t, outside


def spline_eval(lam, t, x):
    """natural cubic spline through (lam, t) at the torch points x (inside the knots)"""
    lam_t = torch.as_tensor(lam)
    h = lam_t[1:] - lam_t[:-1]
    sl = (t[1:] - t[:-1]) / h
    rhs = 6.0 * (sl[1:] - sl[:-1])
    if BANDED_ABOVE is not None and len(lam) > BANDED_ABOVE:
        zi = _BandedSolve.apply(_spline_banded(np.asarray(lam, dtype=np.float64)), rhs)
    else:
        zi = _spline_matrix_inverse(lam) @ rhs
    z = torch.cat([torch.zeros(1, dtype=torch.float64), zi,
                   torch.zeros(1, dtype=torch.float64)])
    pos = np.clip(np.searchsorted(lam, x.detach().numpy(), 'right') - 1, 0,
                  len(lam) - 2)
    pos = torch.as_tensor(pos)
    dl = x - lam_t[pos]
    hh = h[pos]
    b = sl[pos] - hh * (2 * z[pos] + z[pos + 1]) / 6.0
    c = z[pos] / 2.0
    d = (z[pos + 1] - z[pos]) / (6.0 * hh)
    return t[pos] + dl * (b + dl * (c + dl * d))


def marginal_chisq(m, basis_q, const, D, e):
    """chi^2 of the model row m (torch) against D with errors e, orthonormal basis
    rows basis_q [P, npix] and the constant of the basis change"""
    ST = basis_q * (m / e)[None, :]
    Dn = D / e
    A = ST @ ST.T
    v = ST @ Dn
    L = torch.linalg.cholesky(A)
    c = torch.cholesky_solve(v[:, None], L)[:, 0]
    logdet = 2.0 * torch.log(torch.diagonal(L)).sum()
    return logdet + const + 2.0 * torch.log(e).sum() + Dn @ Dn - v @ c


def ortho_basis(lam, npoly, rbf):
    P = orc.get_poly_basis(lam, npoly, rbf)
    Q, R = np.linalg.qr(P.T)
    return torch.as_tensor(np.ascontiguousarray(Q.T)), \
        2.0 * float(np.sum(np.log(np.abs(np.diag(R)))))


def arm_chisq(sd, lib, vel, p, vsini, npoly, rbf):
    """one arm's chi^2 (torch scalar, no penalty) and the template's outside flag"""
    t, outside = template(lib, p, vsini)
    if not np.isfinite(outside):
        return None, outside
    beta = vel / C_KMS
    x = torch.as_tensor(sd.lam) * torch.sqrt((1 - beta) / (1 + beta))
    m = spline_eval(lib.lam, t, x)
    Q, const = ortho_basis(sd.lam, npoly, rbf)
    return marginal_chisq(m, Q, const, torch.as_tensor(sd.spec),
                          torch.as_tensor(sd.espec)), outside


def chisq_and_grad(sds, libs, vel, params, vsini=None, npoly=5, rbf=True,
                   outside_penalty=True):
    """get_chisq of the arms `sds` (oracle SpecData) and its gradient with respect to
    (vel, *params): (float, ndarray [1 + ndim]).  Penalties as get_chisq adds them
    (spec_fit.py:888-896); they are not differentiated."""
    theta = torch.tensor([float(vel)] + [float(_) for _ in params],
                         dtype=torch.float64, requires_grad=True)
    badchi = 10 * sum(len(sd.lam) for sd in sds)
    tot = 0.0 * theta.sum()
    pen = 0.0
    for sd in sds:
        val, outside = arm_chisq(sd, libs[sd.name], theta[0], theta[1:], vsini,
                                 npoly, rbf)
        if val is None:
            pen += 1000.0 * badchi
            continue
        if outside_penalty:
            pen += outside * badchi
        tot = tot + val
    tot.backward()
    return float(tot.item()) + pen, theta.grad.numpy().copy()


def template_jacobian(lib, params):
    """(t [ntp], dt/dp [ndim, ntp]) of the unbroadened template"""
    p = torch.tensor([float(_) for _ in params], dtype=torch.float64)
    f = lambda q: template(lib, q)[0]
    jac = [torch.autograd.functional.jvp(f, p, e)[1].numpy()
           for e in torch.eye(len(p), dtype=torch.float64)]
    return f(p).numpy(), np.array(jac)


# ---- the shared cases of the gradient tests -----------------------------------
# three spectra on the two golden arms: c1, c3, and c0's blue arm with c2's red arm
# (S/N 30, 10 and 100 / 1000)
SPECTRA = [('c1', 'c1'), ('c3', 'c3'), ('c0', 'c2')]
# (spectrum, vel, (teff, logg, feh, alpha), vsini): every query of the first five is
# strictly inside its grid cell, at least 1 % of the cell width away from each face
# (teff is the log-mapped parameter); job 3 is broadened; job 5 lies outside the grid
# (teff below the first node), job 6 has a non-finite mapped parameter
JOBS = [
    (0, -212.7, (6000.0, 2.5, -0.4, 0.1), None),
    (1, 5.5, (6900.0, 1.5, -0.2, 0.05), None),
    (2, 37.3, (5000.0, 2.2, -1.0, 0.2), None),
    (0, -209.49, (6123.0, 2.5, -0.4, 0.1), 30.0),
    (1, 8.71, (4200.0, 3.5, -1.7, 0.3), None),
    (2, 100.0, (3400.0, 2.0, -1.0, 0.2), None),
    (0, 12.5, (-100.0, 2.0, -1.0, 0.2), None),
]
INSIDE = [0, 1, 2, 3, 4]
# a query on a cell with a missing vertex (idgrid[0, 2, 1, 1] = -1)
HOLE_PARAM = (4000.0, 3.5, -1.0, 0.2)


def spectra(cases, cls):
    """the three spectra as lists of `cls` SpecData (gold_b, gold_r)"""
    out = []
    for tb, tr in SPECTRA:
        out.append([cls(n, cases['%s/%s/lam' % (t, n)], cases['%s/%s/spec' % (t, n)],
                        cases['%s/%s/espec' % (t, n)],
                        badmask=cases['%s/%s/badmask' % (t, n)])
                    for t, n in ((tb, 'gold_b'), (tr, 'gold_r'))])
    return out


_truth_cache = {}


def truth_jobs(cases, libs, npoly):
    """[(value, grad)] of JOBS at `npoly` (rbf basis), computed once per npoly"""
    if npoly not in _truth_cache:
        sp = spectra(cases, orc.SpecData)
        _truth_cache[npoly] = [chisq_and_grad(sp[s], libs, v, p, vs, npoly=npoly)
                               for s, v, p, vs in JOBS]
    return _truth_cache[npoly]
