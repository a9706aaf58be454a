"""Yardsticks of rvs_template_tri_vjp, the contraction of one adjoint row
with the tangent rows of a Delaunay library's template, written from the formulas:

  truth        sum_n tbar_n dt_n/dp_k with dt/dp = tri_grad_truth.template_jacobian
               (float64 autograd), the products and the sum over n in long double
  per_element  the method of the kernel in float64 numpy: per knot the ndim sums
               sum_i (db_i/dp_k) L_i[n], times tbar_n (t_n tbar_n for a library of
               log-flux rows), then the sum over n
  vertex_dot   the other order -- the ndim + 1 dot products sum_n u_n L_i[n] first,
               combined with db afterwards -- which cancels: the db_ik sum to zero over
               i and the rows L_i share a large common part

metric(got, want, scale) = |got - want| / sum_n |tbar_n dt_n/dp_k|.  vjp_rel_cpu() is the
largest figure of per_element on the golden libraries at tri_grad_truth.JOBS[0..5] with
seeded adjoint rows of random sign over 12 decades; the device is held to ten times it
(the project's margin for a different summation order).
"""
import numpy as np

import tri_grad_truth as ttruth

SEED = 20260
_cache = {}


def adjoint_row(rng, ntp):
    """random signs, magnitudes 1e-6 .. 1e6"""
    return rng.choice([-1.0, 1.0], size=ntp) * 10.0**rng.uniform(-6.0, 6.0, size=ntp)


def truth(lib, params, tbar):
    """(t [ntp], sum_n tbar_n dt_n/dp_k [ndim] in long double, the metric's scale
    sum_n |tbar_n dt_n/dp_k| [ndim])"""
    t, jac = ttruth.template_jacobian(lib, params)
    prod = tbar.astype(np.longdouble)[None, :] * jac.astype(np.longdouble)
    return t, prod.sum(axis=1), np.abs(prod).sum(axis=1).astype(np.float64)


def _simplex(lib, params):
    p = np.asarray(params, dtype=np.float64)
    with np.errstate(all='ignore'):
        xid = lib.find_simplex(lib.map_params(p))
    if xid < 0:
        return p, xid, None, None
    nd = lib.ndim
    T = lib.transform[xid, :nd, :]
    s = np.array([1.0 / (p[k] * np.log(10.0)) if k in lib.log_ids else 1.0
                  for k in range(nd)])
    db = np.vstack([T * s[None, :], -(T * s[None, :]).sum(axis=0)[None, :]])
    return p, xid, db, lib.dats[lib.simplices[xid], :]


def per_element(lib, params, t, tbar):
    p, xid, db, L = _simplex(lib, params)
    if xid < 0:
        return np.zeros(lib.ndim)
    g = np.zeros((lib.ndim, L.shape[1]))
    for i in range(lib.ndim + 1):
        g += db[i][:, None] * L[i][None, :]
    u = tbar * t if lib.exp else tbar
    return (u[None, :] * g).sum(axis=1)


def vertex_dot(lib, params, t, tbar):
    p, xid, db, L = _simplex(lib, params)
    if xid < 0:
        return np.zeros(lib.ndim)
    u = tbar * t if lib.exp else tbar
    return db.T @ (L @ u)


def metric(got, want, scale):
    return np.abs((np.asarray(got).astype(np.longdouble) - want).astype(np.float64)) / scale


def golden_cases():
    """[(library name, job, params, t, tbar, want, scale)] on the golden libraries at the
    in-simplex jobs; once"""
    if 'cases' not in _cache:
        olibs = ttruth.oracle_libs()
        rng = np.random.default_rng(SEED)
        out = []
        for name in ('gold_b', 'gold_r'):
            lib = olibs[name]
            for j in ttruth.INSIDE:
                p = ttruth.JOBS[j][2]
                tbar = adjoint_row(rng, lib.dats.shape[1])
                t, want, scale = truth(lib, p, tbar)
                out.append((name, j, p, t, tbar, want, scale))
        _cache['olibs'], _cache['cases'] = olibs, out
    return _cache['olibs'], _cache['cases']


def golden_figures(method):
    olibs, cs = golden_cases()
    return np.array([metric(method(olibs[n], p, t, tb), w, s)
                     for n, j, p, t, tb, w, s in cs])


def vjp_rel_cpu():
    if 'rel' not in _cache:
        _cache['rel'] = float(golden_figures(per_element).max())
    return _cache['rel']


def vjp_rel_bound():
    return 10.0 * vjp_rel_cpu()
