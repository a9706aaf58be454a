"""chi^2-grid callers -- API mirror of the grid-driven parts of
py/rvspecfit/vel_fit.py: firstguess (:13-94), _minimum_sampler (:358-439),
_find_best_vel_iterate (:315-355) and the first step of process (:571-602).

`process` (vel_fit.py:505-737) runs its Nelder-Mead stage as S lock-step
simplices (optimizer.py over csrc/nm.hip) over batched objective evaluations (SURVEY 8(f)
rank 1); see its docstring for what differs from the reference.
"""
import contextlib
import itertools
import logging
import math
import os
import threading
import time
import types

import numpy as np
import torch

from . import engine
from . import numdiff
from . import optimizer
from . import spec_fit
from . import spec_inter
from .engine import SpecBatch
from .spec_fit import as_batch


def firstguess(specdata, options=None, config=None, resolParams=None,
               vsinigrid=(None, 10, 100), paramsgrid=None):
    """vel_fit.firstguess (vel_fit.py:13-94).  One spectrum -> dict of best
    parameters; SpecBatch -> dict of [S] tensors."""
    options = options or {}
    if paramsgrid is None:
        paramsgrid = {'logg': [1, 2, 3, 4, 5], 'teff': [3000, 5000, 8000, 10000],
                      'feh': [-2, -1, 0], 'alpha': [0]}
    batch, is_batch = as_batch(specdata)
    names = spec_inter.getSpecParams(batch.names[0], config)
    params = []
    for x in itertools.product(*paramsgrid.values()):
        d = dict(zip(paramsgrid.keys(), x))
        params.append([d[_] for _ in names])
    vg = np.arange(config['min_vel'], config['max_vel'], config['vel_step0'])
    S, dev = batch.S, batch.device
    best_chi = torch.full((S, ), float('inf'), dtype=torch.float64, device=dev)
    best_par = torch.zeros((S, len(names)), dtype=torch.float64, device=dev)
    best_vs = torch.full((S, ), float('nan'), dtype=torch.float64, device=dev)
    for vs in vsinigrid:
        rot = None if vs is None else (vs, )
        r = spec_fit.find_best(batch, vg, params, rot_params=rot,
                               resol_params=resolParams, config=config,
                               options=options)
        better = r['best_chi'] < best_chi
        best_chi = torch.where(better, r['best_chi'], best_chi)
        best_par = torch.where(better[:, None], r['best_param'], best_par)
        if vs is not None:
            best_vs = torch.where(better, torch.full_like(best_vs, float(vs)),
                                  best_vs)
        else:
            best_vs = torch.where(better, torch.full_like(best_vs, float('nan')),
                                  best_vs)
    if is_batch:
        out = {k: best_par[:, i] for i, k in enumerate(names)}
        out['vsini'] = best_vs
        return out
    bp = best_par[0].cpu().numpy()
    out = {}
    for i, k in enumerate(names):
        v = float(bp[i])
        out[k] = int(v) if v == int(v) else v
    v = float(best_vs[0].item())
    if not np.isnan(v):
        out['vsini'] = int(v) if v == int(v) else v
    return out


def _minimum_sampler_batch(batch, best_vel, best_param, vsini, config, options,
                           crit_ratio=5, goal_width=10, grid_budget=1 << 24,
                           resolParams=None, keep_grids=False, templates=None,
                           templ_rows=None):
    """Batched _minimum_sampler (vel_fit.py:358-439): every spectrum carries
    its own (min_vel, max_vel, step) state; per round all spectra that are not
    converged are evaluated on their own velocity grids in one launch set.
    Grid construction follows the reference formula exactly:
        arange(ceil((min_vel-best_vel)/step)*step, max_vel-best_vel, step)+best_vel
    (host float64, per spectrum).  Returns per-spectrum numpy arrays.
    The templates (spline records of every spectrum's parameters, all arms) are
    built once -- or handed over by the caller as `templates` = (coefs, outs) of
    engine.build_templates, with `templ_rows` (int32 [S]) naming the row of each
    spectrum when spectra share templates -- and every round's grids are evaluated against
    them: the reference's get_chisq finds them in its template cache the same way
    (spec_fit.py:902-910)."""
    S, dev = batch.S, batch.device
    opts = options or {}
    npoly = opts.get('npoly') or 5
    rbf = opts.get('rbf_continuum', True)
    libs = spec_inter.get_libs(batch.names, config)
    # The per-spectrum state (window, step, current minimum) lives on the device
    # and every formula below is the reference's, evaluated element-wise in
    # float64 by separate (un-fused) operations -- the same roundings as numpy's:
    #     arange(ceil((min_vel-best_vel)/step)*step, max_vel-best_vel, step)+best_vel
    # The host looks at two numbers per round (how many spectra are still
    # active, the longest grid); no grid ever crosses PCIe.
    f64 = dict(dtype=torch.float64, device=dev)
    min_vel = torch.full((S, ), float(config['min_vel']), **f64)
    max_vel = torch.full((S, ), float(config['max_vel']), **f64)
    step = torch.full((S, ), float(config['vel_step0']), **f64)
    min_vel_step = config['min_vel_step']
    bv0 = best_vel if isinstance(best_vel, torch.Tensor) else \
        torch.as_tensor(np.asarray(best_vel, dtype=np.float64))
    bv = torch.minimum(torch.maximum(bv0.to(**f64).reshape(-1), min_vel),
                       max_vel).clone()
    err = torch.zeros(S, **f64)
    skw = torch.zeros(S, **f64)
    kur = torch.zeros(S, **f64)
    active = torch.ones(S, dtype=torch.bool, device=dev)
    ngrids = torch.zeros(S, dtype=torch.int64, device=dev)
    ngrid_pts = torch.zeros(S, dtype=torch.int64, device=dev)
    params = best_param if isinstance(best_param, torch.Tensor) else \
        torch.as_tensor(np.asarray(best_param, dtype=np.float64)).to(dev)
    if params.dim() == 1:
        params = params[None].expand(S, -1)
    all_grids = [[] for _ in range(S)] if keep_grids else None
    if templates is None:
        coefs, outs = [], []
        for arm in batch.arms:
            c, o = engine.build_templates(libs[arm.name], params.contiguous(),
                                          vsini)
            coefs.append(c)
            outs.append(o)
    else:
        coefs, outs = templates
    resols = spec_fit._resols(batch, resolParams)
    nanv = torch.full((1, ), float('nan'), **f64)
    # (a tensor divisor: torch turns `x / python_scalar` into a multiplication by
    # the reciprocal on the GPU, one ulp away from numpy's division)
    crit = torch.full((1, ), float(crit_ratio), **f64)
    for it in range(10):
        idx = torch.nonzero(active).reshape(-1)
        n = int(idx.numel())
        if n == 0:
            break
        st_, bv_ = step[idx], bv[idx]
        start = torch.ceil((min_vel[idx] - bv_) / st_) * st_
        stop = max_vel[idx] - bv_
        nv = torch.clamp(torch.ceil((stop - start) / st_), min=0).to(torch.int64)
        nvmax = int(nv.max().item())
        # the reference accepts any grid length ((max_vel - min_vel) / vel_step0
        # is the user's choice): long grids are evaluated for fewer spectra at a
        # time, so that a launch set holds at most grid_budget velocities
        r = torch.empty((n, 8), **f64)
        rows = max(1, int(grid_budget // max(nvmax, 1)))
        for a in range(0, n, rows):
            sl = slice(a, a + rows)
            nvc = nv[sl]
            nmax = max(nvmax if rows >= n else int(nvc.max().item()), 1)
            ii = torch.arange(nmax, **f64)
            vg = (start[sl, None] + ii[None, :] * st_[sl, None]) + bv_[sl, None]
            last = vg.gather(1, torch.clamp(nvc - 1, min=0)[:, None])
            vg = torch.where(ii[None, :] < nvc[:, None], vg, last).contiguous()
            if keep_grids:
                vh, nh = vg.cpu().numpy(), nvc.cpu().numpy()
                for k, i in enumerate(idx[sl].cpu().numpy()):
                    all_grids[i].append(vh[k, :nh[k]].copy())
            idt = None if (rows >= n and n == S) else \
                idx[sl].to(torch.int32).contiguous()
            jt = idt
            if templ_rows is not None:
                jt = templ_rows if idt is None else \
                    templ_rows[idx[sl]].contiguous()
            chisq, status = engine.chisq_grid(
                batch, libs, coefs, outs, vg, npoly=npoly, rbf=rbf,
                job_spec=idt, job_templ=jt, resols=resols)
            res, _, _ = engine.grid_moments(
                chisq.reshape(nvc.shape[0], -1), vg, Np=1,
                nvel=nvc.to(torch.int32).contiguous())
            r[sl] = res
        # a spectrum whose grid has no finite minimum (every chi^2 non finite,
        # an empty grid) leaves the loop with NaN results instead of steering
        # the next grid of the whole batch with them
        lost = ~(torch.isfinite(r[:, 1]) & torch.isfinite(r[:, 2])) | (nv < 1)
        keep = ~lost
        bv[idx] = torch.where(lost, nanv, r[:, 1])
        err[idx] = torch.where(lost, nanv, r[:, 2])
        kur[idx] = torch.where(lost, nanv, r[:, 3])
        skw[idx] = torch.where(lost, nanv, r[:, 4])
        ngrids[idx] += keep.to(torch.int64)
        ngrid_pts[idx] += torch.where(keep, nv, torch.zeros_like(nv))
        e_ = err[idx]
        done = (st_ < e_ / crit) | (st_ < min_vel_step)
        coarse = st_ > e_
        new_step = torch.where(coarse, st_ / crit, e_ / crit * 0.8)
        width = torch.where(coarse, st_ * goal_width, e_ * goal_width)
        go = keep & ~done
        active[idx] = go
        bvn = bv[idx]
        min_vel[idx] = torch.where(go, torch.maximum(bvn - width, min_vel[idx]),
                                   min_vel[idx])
        max_vel[idx] = torch.where(go, torch.minimum(bvn + width, max_vel[idx]),
                                   max_vel[idx])
        step[idx] = torch.where(go, new_step, st_)
    bv, err, skw, kur = (_.cpu().numpy() for _ in (bv, err, skw, kur))
    ngrids, ngrid_pts = ngrids.cpu().numpy(), ngrid_pts.cpu().numpy()
    return dict(best_vel=bv, vel_err=err, skewness=skw, kurtosis=kur,
                ngrids=ngrids, npoints=ngrid_pts, grids=all_grids)


_sub_cache = {}


def _sub_batch(batch, idx):
    """view of a subset of spectra as a SpecBatch (full batch -> itself)"""
    if len(idx) == batch.S:
        return batch
    return batch.subset(torch.as_tensor(idx).to(batch.device))


def _find_best_vel_iterate(best_vel, min_vel, max_vel, vel_step0, specdata=None,
                           best_param=None, resolParams=None, config=None,
                           options=None, min_vel_step=None):
    """vel_fit._find_best_vel_iterate (vel_fit.py:315-355) for one spectrum."""
    if best_vel > max_vel or best_vel < min_vel:
        logging.warning('Velocity too large...')
    batch, _ = as_batch(specdata)
    rot = best_param['rot_params']
    vs = None
    if rot is not None:
        vs = torch.as_tensor(np.asarray(rot, dtype=np.float64)).to(batch.device)
    cfg = dict(config)
    cfg.update(min_vel=min_vel, max_vel=max_vel, vel_step0=vel_step0,
               min_vel_step=min_vel_step)
    r = _minimum_sampler_batch(batch, [best_vel], best_param['params'], vs, cfg,
                               options, resolParams=resolParams)
    return (float(r['best_vel'][0]), float(r['vel_err'][0]),
            float(r['skewness'][0]), float(r['kurtosis'][0]))


class VSiniMapper:
    """vel_fit.VSiniMapper (vel_fit.py:95-116) on tensors"""

    def __init__(self, max_vsini):
        self.max_vsini = max_vsini

    def to_internal(self, vsini):
        if not isinstance(vsini, torch.Tensor):   # (one spectrum: the reference's form)
            return np.clip(vsini, 0, self.max_vsini)
        return torch.clamp(vsini, 0, self.max_vsini)

    def to_vsini(self, x):
        if not isinstance(x, torch.Tensor):
            vsini = np.clip(x, 0, self.max_vsini)
            penalty = int(x < 0) * (vsini - x)**2 + int(x > self.max_vsini) * \
                (vsini - x)**2
            return vsini, penalty
        vsini = torch.clamp(x, 0, self.max_vsini)
        out = (x < 0) | (x > self.max_vsini)
        penalty = torch.where(out, (vsini - x)**2, torch.zeros_like(x))
        return vsini, penalty


class ParamMapper:
    """vel_fit.ParamMapper (vel_fit.py:119-202) for a batch: parameter vectors
    [J, n] ordered (vel, [vsini], free stellar parameters in specParams order)
    <-> vel [J], vsini [J] | None, params [J, ndim], penalty [J].
    paramDict0 values are [S] tensors; `idx` selects the spectra of the J rows."""

    def __init__(self, specParams, paramDict0, fixParam, vsiniMapper,
                 fitVsini=True):
        self.specParams = specParams
        self.paramDict0 = paramDict0
        self.fixParam = fixParam
        self.vsiniMapper = vsiniMapper
        self.fitVsini = fitVsini

    def forward(self, p0, idx=None):
        if idx is None and not isinstance(p0, torch.Tensor):
            return self._forward_one(p0)
        ret = {}
        k = 0
        ret['vel'] = p0[:, k]
        k += 1
        penalty = torch.zeros_like(ret['vel'])
        if self.fitVsini:
            vsini, pen = self.vsiniMapper.to_vsini(p0[:, k])
            k += 1
            penalty = penalty + pen
            ret['vsini'] = vsini
        elif 'vsini' in self.fixParam:
            ret['vsini'] = self.paramDict0['vsini'][idx]
        else:
            ret['vsini'] = None
        cols = []
        for x in self.specParams:
            if x in self.fixParam:
                cols.append(self.paramDict0[x][idx])
            else:
                cols.append(p0[:, k])
                k += 1
        assert k == p0.shape[1]
        ret['params'] = torch.stack(cols, dim=1)
        ret['penalty'] = penalty
        return ret

    def _forward_one(self, p0):
        """the reference's own form (vel_fit.py:156-202): ONE parameter vector ->
        dict(vel, vsini, rot_params, params [list], penalty) of plain numbers;
        paramDict0 holds numbers"""
        ret = {}
        p0rev = list(p0)[::-1]
        penalty = 0
        ret['vel'] = p0rev.pop()
        if self.fitVsini:
            vsini, penalty_vsini = self.vsiniMapper.to_vsini(p0rev.pop())
            penalty += penalty_vsini
            ret['vsini'] = vsini
        elif 'vsini' in self.fixParam:
            ret['vsini'] = self.paramDict0['vsini']
        else:
            ret['vsini'] = None
        ret['rot_params'] = None if ret['vsini'] is None else (ret['vsini'], )
        ret['params'] = []
        for x in self.specParams:
            if x in self.fixParam:
                ret['params'].append(self.paramDict0[x])
            else:
                ret['params'].append(p0rev.pop())
        assert len(p0rev) == 0
        ret['penalty'] = penalty
        return ret

    def get_fitted_params(self):
        ret = ['vel']
        if self.fitVsini:
            ret.append('vsini')
        for x in self.specParams:
            if x not in self.fixParam:
                ret.append(x)
        return ret


def chisq_func0(pdict, args, outside_penalty=True):
    """vel_fit.chisq_func0 (vel_fit.py:210-230): chi-square + priors of ONE spectrum
    at the parameter dictionary `pdict` (ParamMapper.forward of one vector); `args` as
    the reference builds it in process (specdata, paramMapper, resolParams, options,
    config, priors).  For user code that drives its own sampler over the objective of
    `process`; process itself evaluates S such objectives per kernel launch."""
    chisq = 0
    if args.get('priors') is not None:
        priors = args['priors']
        for i, k in enumerate(args['paramMapper'].specParams):
            if k in priors:
                chisq += ((priors[k][0] - pdict['params'][i]) / priors[k][1])**2
    chisq += spec_fit.get_chisq(args['specdata'], pdict['vel'],
                                tuple(pdict['params']), pdict['rot_params'],
                                args.get('resolParams'), options=args['options'],
                                config=args['config'],
                                outside_penalty=outside_penalty)
    return chisq


def chisq_func0_grad(pdict, args, outside_penalty=True, vsini_grad=False):
    """chisq_func0 and its analytic gradient with respect to (vel, *specParams), in
    physical units: returns (float, ndarray [1 + ndim]).  The Normal priors add
    2 (p - mu) / sigma^2 to their parameter's component.  The outside-grid penalty
    is piecewise (a distance to the nearest grid point times a constant, switched
    on at the grid's edge): it is part of the value and is NOT differentiated.
    vsini (pdict['rot_params']) is held fixed unless vsini_grad: then the gradient is
    [2 + ndim] with d/dvsini (per km/s) last, and pdict['rot_params'] must be set."""
    chisq, grad = spec_fit.get_chisq_grad(
        args['specdata'], pdict['vel'], tuple(pdict['params']), pdict['rot_params'],
        options=args['options'], config=args['config'],
        outside_penalty=outside_penalty, resol_params=args.get('resolParams'),
        vsini_grad=vsini_grad)
    grad = np.array(grad, dtype=np.float64)
    if args.get('priors') is not None:
        priors = args['priors']
        for i, k in enumerate(args['paramMapper'].specParams):
            if k in priors:
                mu, sig = priors[k]
                chisq += ((mu - pdict['params'][i]) / sig)**2
                grad[1 + i] += 2.0 * (pdict['params'][i] - mu) / sig**2
    return chisq, grad


def chisq_func(p, args):
    """vel_fit.chisq_func (vel_fit.py:233-257): the function process minimises --
    1e30 outside [min_vel, max_vel] or at a non-finite parameter, else chisq_func0 +
    the vsini penalty"""
    pdict = args['paramMapper'].forward(p)
    if (pdict['vel'] > args['max_vel'] or pdict['vel'] < args['min_vel']
            or (~np.isfinite(np.asarray(pdict['params'], dtype=float))).any()):
        return 1e30
    return chisq_func0(pdict, args) + pdict['penalty']


def chisq_func_grad(p, args):
    """chisq_func and its gradient with respect to the optimiser's own vector `p`, in
    the order of paramMapper.get_fitted_params() (fixed parameters dropped): returns
    (float, ndarray [len(p)]) -- the `fun` of scipy.optimize.minimize(..., jac=True).
    The vsini component is the physical derivative where 0 < x < max_vsini; outside
    that range VSiniMapper clamps, so the physical derivative is 0 and the penalty's
    2 (x - clamp(x)) stands alone.  Priors as in chisq_func0_grad.  Where chisq_func
    returns 1e30 (velocity out of bounds, non-finite parameter): (1e30, zeros)."""
    mapper = args['paramMapper']
    pdict = mapper.forward(p)
    if (pdict['vel'] > args['max_vel'] or pdict['vel'] < args['min_vel']
            or (~np.isfinite(np.asarray(pdict['params'], dtype=float))).any()):
        return 1e30, np.zeros(len(p))
    chisq, g0 = chisq_func0_grad(pdict, args, vsini_grad=mapper.fitVsini)
    return chisq + pdict['penalty'], _optimiser_grad(p, mapper, pdict, g0)


def _optimiser_grad(p, mapper, pdict, g0):
    # the gradient over (vel, *specParams[, vsini]) in the optimiser's own columns
    grad = []
    for x, name in zip(p, mapper.get_fitted_params()):
        if name == 'vel':
            grad.append(g0[0])
        elif name == 'vsini':
            vsini = pdict['vsini']
            inside = 0 < x < mapper.vsiniMapper.max_vsini
            grad.append((g0[-1] if inside else 0.0) + 2.0 * (x - vsini))
        else:
            grad.append(g0[1 + list(mapper.specParams).index(name)])
    assert len(grad) == len(p)
    return np.array(grad, dtype=np.float64)


def chisq_func_fisher(p, args):
    """chisq_func_grad with the Gauss-Newton Hessian of chisq_func in the optimiser's
    own vector: returns (float, ndarray [n], ndarray [n, n]), n = len(p) -- the public
    form of a row of optimizer.GradChain(fisher=True) and what the Levenberg-Marquardt
    polish (config['second_minimizer_lm']) steps on.  Value and gradient are
    chisq_func_grad's.  H_ab = 2 F_ab with F the Fisher matrix of
    spec_fit.get_chisq_fisher (which is in the 0.5 chi^2 convention) over the fitted
    parameters; fixed parameters have no row or column; a Normal prior adds 2 / sigma^2
    to its parameter's diagonal; the vsini row and column are the matrix's where
    0 < x < max_vsini, else 0, and where x is outside [0, max_vsini] the clamp
    penalty's second derivative, 2, stands on the diagonal.  log det A and the outside
    penalty add nothing.  Where chisq_func returns 1e30: (1e30, zeros, zeros)."""
    mapper = args['paramMapper']
    pdict = mapper.forward(p)
    n = len(p)
    if (pdict['vel'] > args['max_vel'] or pdict['vel'] < args['min_vel']
            or (~np.isfinite(np.asarray(pdict['params'], dtype=float))).any()):
        return 1e30, np.zeros(n), np.zeros((n, n))
    chisq, g0, F0 = spec_fit.get_chisq_fisher(
        args['specdata'], pdict['vel'], tuple(pdict['params']), pdict['rot_params'],
        options=args['options'], config=args['config'], outside_penalty=True,
        resol_params=args.get('resolParams'), vsini_grad=mapper.fitVsini)
    g0 = np.array(g0, dtype=np.float64)
    priors = args.get('priors') or {}
    specParams = list(mapper.specParams)
    for i, k in enumerate(specParams):
        if k in priors:
            mu, sig = priors[k]
            chisq += ((mu - pdict['params'][i]) / sig)**2
            g0[1 + i] += 2.0 * (pdict['params'][i] - mu) / sig**2
    grad = _optimiser_grad(p, mapper, pdict, g0)
    fitted = mapper.get_fitted_params()
    tan = [0 if k == 'vel' else (F0.shape[0] - 1 if k == 'vsini'
                                 else 1 + specParams.index(k)) for k in fitted]
    H = 2.0 * np.asarray(F0, dtype=np.float64)[np.ix_(tan, tan)]
    for a, (x, k) in enumerate(zip(p, fitted)):
        if k == 'vsini':
            max_vsini = mapper.vsiniMapper.max_vsini
            if not 0 < x < max_vsini:
                H[a, :] = 0.0
                H[:, a] = 0.0
            if x < 0 or x > max_vsini:
                H[a, a] += 2.0
        elif k in priors:
            H[a, a] += 2.0 / priors[k][1]**2
    return chisq + pdict['penalty'], grad, H


def hess_func(p, pdict, args):
    """vel_fit.hess_func (vel_fit.py:260-269): 0.5 chi-square in the stellar parameters
    `p` at the rest of `pdict`"""
    pdict['params'][:] = p[:]
    return 0.5 * chisq_func0(pdict, args)


def get_hess_inv(param_names):
    """vel_fit.get_hess_inv (vel_fit.py:442-461)"""
    diag = np.zeros(len(param_names)) + 0.1**2
    names = np.asarray(param_names)
    diag[np.nonzero(names == 'teff')[0][0]] = 50**2
    vi = np.nonzero(names == 'vsini')[0]
    if len(vi) == 1:
        diag[vi] = 5**2
    diag[0] = 1**2
    return np.diag(diag)


def _uncertainties_from_hessians(H):
    """_uncertainties_from_hessian for a stack [S, n, n] in one LAPACK call (the
    per-matrix Python loop was 0.6 s per 10 000 spectra): np.linalg.inv factors
    every matrix of a stack on its own, so each inverse is the one-matrix
    call's, bit for bit; a singular or non-finite matrix takes the
    diagonal-only branch of the reference.  Returns (diag_err [S, n], covar
    [S, n, n], bad [S])."""
    H = np.asarray(H, dtype=np.float64)
    S, n = H.shape[0], H.shape[1]
    dh = np.diagonal(H, axis1=1, axis2=2)
    with np.errstate(all='ignore'):
        inv_d = 1. / (dh + (dh == 0))
    inv_d = np.where(dh == 0, np.inf, inv_d)
    bad = np.zeros(S, dtype=bool)
    Hinv = np.empty_like(H)
    ok = np.isfinite(H).all(axis=(1, 2))
    if ok.any():
        try:
            Hinv[ok] = np.linalg.inv(H[ok])
        except np.linalg.LinAlgError:    # some matrix is exactly singular
            for i in np.nonzero(ok)[0]:
                try:
                    Hinv[i] = np.linalg.inv(H[i])
                except np.linalg.LinAlgError:
                    ok[i] = False
    for i in np.nonzero(~ok)[0]:
        bad[i] = True
        Hinv[i] = np.diag(inv_d[i])
    e0 = np.array(np.diagonal(Hinv, axis1=1, axis2=2))
    e1 = inv_d
    bad0, bad1 = e0 < 0, e1 < 0
    bad |= bad0.any(axis=1)
    sub1, sub2 = bad0 & ~bad1, bad0 & bad1
    e0[sub1] = e1[sub1]
    e0[sub2] = 0
    with np.errstate(all='ignore'):
        err = np.sqrt(e0)
    err[sub2] = np.nan
    bad |= (~np.isfinite(err)).any(axis=1)
    return err, Hinv, bad


def _uncertainties_from_hessian(hessian):
    """vel_fit._uncertainties_from_hessian (vel_fit.py:464-502), one matrix"""
    diag_hessian = np.diag(hessian)
    with np.errstate(all='ignore'):
        inv_diag_hessian = 1. / (diag_hessian + (diag_hessian == 0))
    inv_diag_hessian[diag_hessian == 0] = np.inf
    bad_hessian = False
    try:
        if not np.isfinite(hessian).all():
            raise ValueError('non finite Hessian')  # scipy.linalg.inv check_finite
        hessian_inv = np.linalg.inv(hessian)
    except (np.linalg.LinAlgError, ValueError):
        bad_hessian = True
        hessian_inv = np.diag(inv_diag_hessian)
    diag_err0 = np.array(np.diag(hessian_inv))
    diag_err1 = inv_diag_hessian
    bad_err0 = diag_err0 < 0
    bad_err1 = diag_err1 < 0
    if bad_err0.any():
        bad_hessian = True
    sub1 = bad_err0 & (~bad_err1)
    sub2 = bad_err0 & bad_err1
    diag_err0[sub1] = diag_err1[sub1]
    diag_err0[sub2] = 0
    with np.errstate(all='ignore'):
        diag_err = np.sqrt(diag_err0)
    diag_err[sub2] = np.nan
    if (~np.isfinite(diag_err)).sum() != 0:
        bad_hessian = True
    return diag_err, hessian_inv, bad_hessian


# iteration cap of a Nelder-Mead run (vel_fit.py:630, 644: maxiter=10000); a
# spectrum that hits it is restarted once from its final simplex
NM_MAXITER = 10000
_SIMPLEX_STD = {'logg': 0.5, 'teff': 300, 'feh': 0.5, 'alpha': 0.25}
HESS_BASE_STEP = {'vsini': 1 / 100, 'logg': 0.1 / 100, 'feh': 0.1 / 100,
                  'alpha': .01 / 100, 'teff': 1 / 100, 'vrad': 1 / 100}


def _get_simplex_start(best_vel, fixParam, specParamNames, paramDict0,
                       vsiniMapper, fitVsini):
    """vel_fit._get_simplex_start (vel_fit.py:272-312) for [S] starting points:
    the same deterministic RandomState(43434) displacement pattern for every
    spectrum."""
    cols = [best_vel]
    std_vec = [5]
    if fitVsini:
        cols.append(vsiniMapper.to_internal(paramDict0['vsini']))
        std_vec.append(3)
    for x in specParamNames:
        if x not in fixParam:
            cols.append(paramDict0[x])
            std_vec.append(_SIMPLEX_STD.get(x) or 0.5)
    curval = torch.stack(cols, dim=1)
    ndim = curval.shape[1]
    R = np.random.RandomState(43434)
    disp = np.array(std_vec)[None, :] * R.normal(size=(ndim, ndim))
    simp = curval[:, None, :].repeat(1, ndim + 1, 1)
    simp[:, 1:, :] = curval[:, None, :] + torch.as_tensor(disp).to(curval.device)
    return curval, simp


class _Objective:
    """chisq_func / chisq_func0 (vel_fit.py:205-254) for J jobs at a time."""

    def __init__(self, batch, mapper, config, options, priors,
                 resolParams=None):
        self.resolParams = resolParams
        self.batch, self.mapper = batch, mapper
        self.config, self.options, self.priors = config, options, priors
        self.min_vel, self.max_vel = config['min_vel'], config['max_vel']
        self.status = torch.zeros(batch.S, dtype=torch.int32,
                                  device=batch.device)
        self.nfev = 0

    def chisq0(self, idx, vel, params, vsini):
        chisq = torch.zeros_like(vel)
        if self.priors is not None:
            for i, k in enumerate(self.mapper.specParams):
                if k in self.priors:
                    m, sg = self.priors[k]
                    m = m[idx] if isinstance(m, torch.Tensor) else m
                    sg = sg[idx] if isinstance(sg, torch.Tensor) else sg
                    chisq = chisq + ((m - params[:, i]) / sg)**2
        c, st = spec_fit.chisq_jobs(self.batch, idx, vel, params, vsini,
                                    self.options, self.config,
                                    resol_params=self.resolParams)
        self.status[idx] |= st
        self.nfev += idx.numel()
        return chisq + c

    def __call__(self, idx, p):
        pd = self.mapper.forward(p, idx)
        vel, params = pd['vel'], pd['params']
        bad = (vel > self.max_vel) | (vel < self.min_vel) | \
            (~torch.isfinite(params)).any(dim=1)
        # rows that the reference answers with 1e30 without evaluating are
        # evaluated at a harmless point and overwritten
        velc = torch.where(bad, torch.zeros_like(vel), vel)
        parc = torch.where(bad[:, None], self.safe_params[idx], params)
        ret = self.chisq0(idx, velc, parc, pd['vsini']) + pd['penalty']
        return torch.where(bad, torch.full_like(ret, 1e30), ret)


def _as_param_tensors(paramDict0, S, dev):
    out = {}
    for k, v in paramDict0.items():
        if isinstance(v, torch.Tensor):
            t = v.to(dev, torch.float64).reshape(-1)
        else:
            t = torch.as_tensor(np.asarray(v, dtype=np.float64)).to(dev
                                                                     ).reshape(-1)
        out[k] = t.expand(S).contiguous() if t.numel() == 1 else t.contiguous()
        assert out[k].shape[0] == S
    return out


def _hessian_stage(obj, names, vel, params, vsini):
    """vel_fit.py:699-725 for S spectra: the Hessian of 0.5 * chisq_func0 in the
    stellar parameters at (vel, params, vsini), as numdifftools computes it
    (numdiff.py), and vel_fit._uncertainties_from_hessian per spectrum.
    First ndf.Hessian(step=MinStepGenerator(base_step)) = the central rule at
    one step; rows flagged bad are redone with the default step generator
    (15 steps, Richardson + Wynn extrapolation).  Returns numpy arrays
    (param_err [S, n], param_covar [S, n, n], bad_hessian [S])."""
    dev = params.device
    S = params.shape[0]

    def hess_func(idx, p):   # vel_fit.hess_func (vel_fit.py:257-269)
        return 0.5 * obj.chisq0(idx, vel[idx], p.contiguous(),
                                None if vsini is None else vsini[idx])

    base = torch.as_tensor([HESS_BASE_STEP[_] for _ in names],
                           dtype=torch.float64, device=dev)
    bad_hessian = np.zeros(S, dtype=bool)
    diag_err = np.zeros((S, len(names)))
    covar = np.zeros((S, len(names), len(names)))
    todo = np.arange(S)
    for attempt in range(2):
        if len(todo) == 0:
            break
        tt = torch.as_tensor(todo).to(dev)
        xx = params[tt]
        fn = lambda i, p: hess_func(tt[i], p)   # noqa: E731
        if attempt == 0:
            H = numdiff.hessian_central(fn, xx, numdiff.first_try_step(base, xx)
                                        ).cpu().numpy()
        else:
            H = numdiff.hessian_retry(fn, xx)
        diag_err[todo], covar[todo], bad_hessian[todo] = \
            _uncertainties_from_hessians(H)
        todo = todo[bad_hessian[todo]]
    return diag_err, covar, bad_hessian


def param_uncertainties(specdata, vel, atm_params, vsini=None, options=None,
                        config=None, resolParams=None, priors=None):
    """The uncertainty stage of `process` on its own (vel_fit.py:699-725): the
    finite-difference Hessian of 0.5 chi^2 in the stellar parameters at the given
    point.  One spectrum (list of SpecData; atm_params a dict or sequence in
    the interpolator's parameter order): dict(param_err {name: sigma},
    param_covar, bad_hessian); a SpecBatch with [S] / [S, n] tensors: arrays
    with a leading S axis."""
    batch, is_batch = as_batch(specdata)
    options = options or {}
    dev = batch.device
    S = batch.S
    names = list(spec_inter.getSpecParams(batch.names[0], config))
    if isinstance(atm_params, dict):
        atm_params = [atm_params[k] for k in names]
    pt = torch.as_tensor(np.asarray(
        atm_params.cpu() if isinstance(atm_params, torch.Tensor) else atm_params,
        dtype=np.float64)).to(dev).reshape(-1, len(names))
    pt = pt.expand(S, len(names)).contiguous()
    pd = _as_param_tensors(dict(vel=vel), S, dev)
    vs = None
    if vsini is not None:
        vs = _as_param_tensors(dict(vsini=vsini), S, dev)['vsini']
    mapper = types.SimpleNamespace(specParams=names)
    obj = _Objective(batch, mapper, config, options, priors, resolParams)
    err, covar, bad = _hessian_stage(obj, names, pd['vel'], pt, vs)
    if is_batch:
        return dict(param_err={k: err[:, i] for i, k in enumerate(names)},
                    param_covar=covar, bad_hessian=bad, status=obj.status)
    return dict(param_err=dict(zip(names, err[0])), param_covar=covar[0],
                bad_hessian=bool(bad[0]))


def _uncertainties_from_fisher(F, names, stellar, prior_isig2=None, fixParam=()):
    """The host part of fisher_uncertainties on plain numpy: F [S, K, K] over `names`
    (K = len(names)), `stellar` the names among them that are stellar parameters,
    prior_isig2 {name: 1 / sigma^2, scalar or [S]}, fixParam the names to drop.
    Both inverses go through _uncertainties_from_hessians (the reference's rule and its
    diagonal fallback) after the symmetric scaling diag(F)^-1/2 F diag(F)^-1/2: K beside
    dex gives condition numbers of 1e8 ... 1e10 unscaled.  A zero row (a parameter the
    model does not depend on: a point outside the grid) keeps its scale 1, makes the
    matrix singular and takes the fallback: an infinite error, bad_fisher, no
    exception."""
    F = np.array(F, dtype=np.float64)
    S = F.shape[0]
    assert F.shape[1:] == (len(names), len(names))
    for k, v in (prior_isig2 or {}).items():
        if k in names:
            i = list(names).index(k)
            F[:, i, i] += np.broadcast_to(np.asarray(v, dtype=np.float64), (S, ))
    keep = [i for i, k in enumerate(names) if k not in fixParam]
    names = [names[i] for i in keep]
    F = F[:, keep][:, :, keep]

    def scaled_inverse(M):
        d = np.diagonal(M, axis1=1, axis2=2)
        with np.errstate(all='ignore'):
            sc = np.where(d > 0, 1. / np.sqrt(np.where(d > 0, d, 1.)), 1.)
        err, inv, bad = _uncertainties_from_hessians(M * sc[:, :, None] * sc[:, None, :])
        return err * sc, inv * sc[:, :, None] * sc[:, None, :], bad

    err, covar, bad = scaled_inverse(F)
    ist = [i for i, k in enumerate(names) if k in stellar]
    perr, pcovar, pbad = scaled_inverse(F[:, ist][:, :, ist])
    nan = np.full(S, np.nan)
    return dict(names=names, fisher=F, covar=covar,
                err={k: err[:, i] for i, k in enumerate(names)},
                vel_err=err[:, names.index('vel')] if 'vel' in names else nan,
                param_err={names[i]: perr[:, n] for n, i in enumerate(ist)},
                param_covar=pcovar, bad_fisher=bad | pbad)


def fisher_uncertainties(specdata, vel, atm_params, vsini=None, options=None,
                         config=None, priors=None, fixParam=None, vsini_grad=False,
                         resolParams=None):
    """Uncertainties from the Fisher matrix of the continuum-marginalised fit
    (spec_fit.get_chisq_fisher) at the given point: one deterministic call instead of the
    33+ objective evaluations of param_uncertainties, and positive semi-definite at any
    point, where the finite-difference Hessian holds only at an exact optimum.
    names = ['vel'] + the stellar parameters not in fixParam (+ ['vsini'] with
    vsini_grad, which needs vsini).  Normal priors {name: (mean, sigma)} add 1 / sigma^2
    to their diagonal entry.  Returns a dict:
      names, fisher [n, n], covar [n, n] = fisher^-1 (joint: every error is
      marginalised over the other names), err {name: sigma}, vel_err,
      param_err {name: sigma} / param_covar: the stellar block inverted on its own, i.e.
      with velocity and vsini held -- the reference's definition (vel_fit.py:699-725),
      comparable with param_uncertainties and process,
      bad_fisher: an inverse that could not be formed or gave a non-finite error.
    One spectrum (list of SpecData; atm_params a dict or a sequence in the
    interpolator's order): floats and arrays as listed; a SpecBatch: the same with a
    leading S axis.  The scope is get_chisq_grad's (ValueError otherwise): resolution
    matrices -- resolParams, or the SpecData's own -- with config['resol_gradient']."""
    batch, is_batch = as_batch(specdata)
    dev, S = batch.device, batch.S
    stellar = list(spec_inter.getSpecParams(batch.names[0], config))
    if isinstance(atm_params, dict):
        atm_params = [atm_params[k] for k in stellar]
    pt = torch.as_tensor(np.asarray(
        atm_params.cpu() if isinstance(atm_params, torch.Tensor) else atm_params,
        dtype=np.float64)).to(dev).reshape(-1, len(stellar))
    pt = pt.expand(S, len(stellar)).contiguous()
    velt = _as_param_tensors(dict(vel=vel), S, dev)['vel']
    vs = None
    if vsini is not None:
        vs = _as_param_tensors(dict(vsini=vsini), S, dev)['vsini']
    _, _, F = spec_fit.get_chisq_fisher(batch, velt, pt, vs, options=options,
                                        config=config, resol_params=resolParams,
                                        vsini_grad=vsini_grad)
    names = ['vel'] + stellar + (['vsini'] if vsini_grad else [])
    isig2 = {}
    for k, (_, sg) in (priors or {}).items():
        sg = sg.cpu().numpy() if isinstance(sg, torch.Tensor) else np.asarray(sg)
        isig2[k] = 1. / np.asarray(sg, dtype=np.float64)**2
    res = _uncertainties_from_fisher(F.cpu().numpy(), names, stellar, isig2,
                                     list(fixParam) if fixParam is not None else [])
    if is_batch:
        return res

    def one(v):
        if isinstance(v, dict):
            return {k: one(x) for k, x in v.items()}
        if isinstance(v, list):
            return v
        return v[0] if v[0].ndim else v[0].item()
    return one(res)


# A SpecBatch of at least PROCESS_SPLIT_MIN spectra is fitted as two interleaved
# halves by two host threads on two HIP streams: the optimiser's rounds run in C
# (rvs_nm_run, no interpreter lock), so while one half is in the latency-bound
# tail of its rounds the other's kernels fill the CUs.  Results are those of the
# unsplit run, bit for bit (no spectrum sees another;
# test_process_two_halves_equal_one_batch).  1 switches it off.
PROCESS_STREAMS = int(os.environ.get('RVS_PROCESS_STREAMS', '2'))
# the second minimiser's rounds on the device (rvs_bfgs_run) wherever the library
# launches the objective itself; False: the host machines around the Python objective
# (what Delaunay evaluators without a bucket grid and resolution matrices wider than
# the objective kernel's band take anyway) -- the two run the
# same state machine (test_process_bfgs_device_equals_host)
BFGS_ON_DEVICE = os.environ.get('RVS_BFGS_ON_DEVICE', '1') != '0'
# (64: the stellar targets of one DESI petal are 100-200 spectra -- split, 100 spectra
# 832 -> 879 per second, 200: 1207 -> 1272; it was 256 until the end of round 5)
PROCESS_SPLIT_MIN = int(os.environ.get('RVS_PROCESS_SPLIT_MIN', '64'))


_tls = threading.local()


@contextlib.contextmanager
def single_stream():
    """process() calls of this thread inside the block are not split: for
    callers whose own host threads already keep the GPU and the interpreter busy
    (desi_fit.proc_many, which conditions the next group of files meanwhile --
    there the split measured 5 % slower)."""
    old = getattr(_tls, 'single', False)
    _tls.single = True
    try:
        yield
    finally:
        _tls.single = old


def _merge_parts(parts, idxs, S):
    """results of process() on the spectra idxs[k] -> one result over S"""
    first = parts[0]
    n0 = len(idxs[0])

    def merge(vals):
        v = vals[0]
        if isinstance(v, dict):
            return {k: merge([x[k] for x in vals]) for k in v}
        if isinstance(v, (list, tuple)):
            return [merge([x[i] for x in vals]) for i in range(len(v))]
        if isinstance(v, torch.Tensor) and v.dim() >= 1 and v.shape[0] == n0:
            if v.dim() == 2 and len({x.shape[1] for x in vals}) > 1:
                # per-pixel rows of a grid set: each part is as wide as the longest
                # grid IT holds (ArmData.subset); zeros behind a spectrum's pixels
                out = torch.zeros((S, max(x.shape[1] for x in vals)),
                                  dtype=v.dtype, device=v.device)
                for x, ix in zip(vals, idxs):
                    out[ix, :x.shape[1]] = x
                return out
            out = torch.empty((S, ) + tuple(v.shape[1:]), dtype=v.dtype,
                              device=v.device)
            for x, ix in zip(vals, idxs):
                out[ix] = x
            return out
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == n0:
            out = np.empty((S, ) + v.shape[1:], dtype=v.dtype)
            for x, ix in zip(vals, idxs):
                out[ix.cpu().numpy()] = x
            return out
        return v
    out = {k: merge([p[k] for p in parts]) for k in first}
    out['nm_rounds'] = max(p['nm_rounds'] for p in parts)
    out['objective_evals'] = sum(p['objective_evals'] for p in parts)
    out['nm_launched_rows'] = sum(p.get('nm_launched_rows', 0) for p in parts)
    if 'bfgs' in first:
        out['bfgs']['rounds'] = max(p['bfgs']['rounds'] for p in parts)
    return out


_SPLIT_STREAMS = {}


@contextlib.contextmanager
def stream_lane(lane):
    """process() calls of this thread inside the block run their halves on the
    streams of `lane` (desi_fit.proc_many with two fit threads: a pair of streams
    per thread, so that two groups' rounds do not queue behind one another)"""
    old = getattr(_tls, 'lane', 0)
    _tls.lane = int(lane)
    try:
        yield
    finally:
        _tls.lane = old


def _split_stream(dev, k, lane=0):
    # kept: the caching allocator's pools are per stream
    key = (dev.index, k, lane)
    if key not in _SPLIT_STREAMS:
        _SPLIT_STREAMS[key] = torch.cuda.Stream(device=dev)
    return _SPLIT_STREAMS[key]


def _subset_priors(priors, idx):
    # per-spectrum priors are tensors (see _Objective.chisq0)
    if not priors:
        return priors
    return {n_: tuple(v[idx].contiguous()
                      if isinstance(v, torch.Tensor) and v.dim() else v for v in mv)
            for n_, mv in priors.items()}


def _process_split(batch, paramDict0, kwargs):
    S, dev = batch.S, batch.device
    nparts = max(2, int(PROCESS_STREAMS))
    idxs = [torch.arange(k, S, nparts, device=dev) for k in range(nparts)]
    pd = _as_param_tensors(paramDict0, S, dev)
    pri = kwargs.get('priors')
    # template libraries are loaded (uploaded) here, before either thread
    spec_inter.get_libs(batch.names, kwargs['config'])
    torch.cuda.current_stream().synchronize()
    parts, errs = [None] * nparts, [None] * nparts
    lane = getattr(_tls, 'lane', 0)

    def run(k):
        try:
            st = _split_stream(dev, k, lane)
            with torch.cuda.stream(st):
                sub = batch.subset(idxs[k])
                pdk = {n: v[idxs[k]].contiguous() for n, v in pd.items()}
                kw = dict(kwargs, priors=_subset_priors(pri, idxs[k]))
                parts[k] = _process_one(sub, pdk, **kw)
            st.synchronize()
        except BaseException as e:  # noqa: BLE001 -- re-raised by the caller
            errs[k] = e
    th = [threading.Thread(target=run, args=(k, )) for k in range(nparts)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for e in errs:
        if e is not None:
            raise e
    return _merge_parts(parts, idxs, S)


def _rounds_run_in_c(batch, config, resolParams, options=None):
    """the optimiser's rounds of this batch run inside the library (rvs_nm_run:
    regular-grid, MLP and bucketed Delaunay libraries, with resolution matrices
    where engine.can_fuse_objective admits them); only then do two host threads
    help -- rounds driven from Python (other evaluators, resolution matrices wider
    than the objective kernel's band) share the interpreter lock (round 3, NN
    rounds still in Python: 432 against 586 spectra/s split in two)"""
    libs = spec_inter.get_libs(batch.names, config)
    npoly = (options or {}).get('npoly') or 5
    form = engine.objective_form(batch, libs,
                                 spec_fit._resols(batch, resolParams), npoly)
    return engine.rounds_in_library(batch, libs, form)


def process(specdata, paramDict0, fixParam=None, options=None, config=None,
            resolParams=None, priors=None, timers=None):
    """vel_fit.process (see _process_one); a large SpecBatch is fitted as two
    concurrent halves (PROCESS_STREAMS)."""
    if config is None:
        raise RuntimeError('Config must be provided')
    if (PROCESS_STREAMS >= 2 and isinstance(specdata, SpecBatch)
            and specdata.S >= PROCESS_SPLIT_MIN and timers is None
            and not getattr(_tls, 'single', False)
            and _rounds_run_in_c(specdata, config, resolParams, options)):
        return _process_split(specdata, paramDict0, dict(
            fixParam=fixParam, options=options, config=config,
            resolParams=resolParams, priors=priors))
    return _process_one(specdata, paramDict0, fixParam=fixParam, options=options,
                        config=config, resolParams=resolParams, priors=priors,
                        timers=timers)


def _process_one(specdata, paramDict0, fixParam=None, options=None, config=None,
                 resolParams=None, priors=None, timers=None):
    """vel_fit.process (vel_fit.py:505-737): velocity grid at the starting
    parameters -> Nelder-Mead (deterministic start simplex, fatol 1e-3, xatol
    1e-2, up to two runs) -> [BFGS] -> velocity refinement -> full output ->
    finite-difference Hessian -> parameter uncertainties.

    One spectrum (list of SpecData) returns the reference's dict.  A SpecBatch
    (paramDict0 values scalars or [S] arrays) returns [S]-leading device
    tensors; the S optimisers advance in lock-step (optimizer.DeviceNelderMead), every
    objective evaluation is one batched template build + chi^2 launch set.

    config['second_minimizer'] (default True in utils.read_config, as in the
    reference) adds scipy's BFGS (csrc/bfgs_host.cpp; host state per spectrum,
    batched objective).  The Hessian is numdifftools' (vel_fit.py:713-716)
    restated in numdiff.py: MinStepGenerator(base_step) -> one central step;
    the step=None retry of rows with a bad Hessian -> 15 steps, Richardson +
    Wynn extrapolation; every displacement pattern is one batched objective
    call (param_err pinned to 1e-3: test_param_uncertainties_at_reference_optimum)."""
    if config is None:
        raise RuntimeError('Config must be provided')
    options = options or {}
    batch, is_batch = as_batch(specdata)
    S, dev = batch.S, batch.device
    min_vel, max_vel = config['min_vel'], config['max_vel']
    vel_step0 = config['vel_step0']
    max_vsini = config['max_vsini']
    min_vel_step = config['min_vel_step']
    fixParam = list(fixParam) if fixParam is not None else []
    names = spec_inter.getSpecParams(batch.names[0], config)
    pd0 = _as_param_tensors(paramDict0, S, dev)
    curparam = torch.stack([pd0[_] for _ in names], dim=1)
    vsiniMapper = None
    if 'vsini' not in pd0:
        vsini0, fitVsini = None, False
    else:
        vsini0 = pd0['vsini']
        fitVsini = 'vsini' not in fixParam
        if fitVsini:
            vsiniMapper = VSiniMapper(max_vsini)
    tm = timers if timers is not None else {}
    # config['second_minimizer_jac']: the BFGS polish on the analytic gradient
    # (rvs_bfgs_run_grad).  What the gradient does not cover is refused here, before
    # anything is built: nothing falls back to differences
    bfgs_jac = bool(config.get('second_minimizer')
                    and config.get('second_minimizer_jac'))
    # config['second_minimizer_lm']: Levenberg-Marquardt on the Fisher matrix (rvs_lm_run)
    # in the place of the BFGS polish; the scope is the gradient's, asked here as well
    lm_polish = bool(config.get('second_minimizer')
                     and config.get('second_minimizer_lm'))
    if lm_polish and config.get('second_minimizer_jac'):
        raise ValueError("config['second_minimizer_lm'] and "
                         "config['second_minimizer_jac'] name two polishes: set one")
    # config['fused_gradient']: the polish's rows from rvs_objective_grad, one kernel
    # per (row, arm) (rvs_bfgs_run_grad_fused).  What needs the chain's tangent rows
    # beside the key is an error that says so; nothing changes path silently.  With
    # config['resol_gradient'] beside it resolution matrices go into the kernel
    # (rvs_bfgs_run_grad_fused_resol); a band it does not take is an error too
    fused_grad = bool(config.get('fused_gradient'))
    if fused_grad:
        engine.check_fused_grad_scope(
            batch, spec_inter.get_libs(batch.names, config), options.get('npoly') or 5,
            spec_fit._resols(batch, resolParams), bool(options.get('fast_interp')),
            vsini_grad=fitVsini, nn_gradient=bool(config.get('nn_gradient')),
            tri_gradient=bool(config.get('tri_gradient')),
            resol_gradient=bool(config.get('resol_gradient')),
            what="config['second_minimizer_lm'] (the Levenberg-Marquardt polish on the "
                 "Fisher matrix)" if lm_polish else
                 ("config['fisher_uncertainties'] (the Fisher matrix)"
                  if config.get('fisher_uncertainties') else None))
    # config['fused_fisher']: the Fisher matrix -- the rows of the Levenberg-Marquardt
    # polish (rvs_lm_run_fused) and config['fisher_uncertainties'] -- from
    # rvs_objective_fisher, one forward-mode kernel per (row, arm).  What the kernel does
    # not cover beside the key is an error that says so
    fused_fisher = bool(config.get('fused_fisher'))
    if fused_fisher and (lm_polish or config.get('fisher_uncertainties')):
        engine.check_fused_fisher_scope(
            batch, spec_inter.get_libs(batch.names, config), options.get('npoly') or 5,
            spec_fit._resols(batch, resolParams), bool(options.get('fast_interp')),
            vsini_grad=fitVsini)
    if lm_polish and not fused_fisher:   # (the fused form holds no row buffers to budget)
        try:
            engine.check_grad_scope(batch, spec_inter.get_libs(batch.names, config),
                                    options.get('npoly') or 5,
                                    spec_fit._resols(batch, resolParams),
                                    bool(options.get('fast_interp')),
                                    vsini_grad=fitVsini,
                                    nn_gradient=bool(config.get('nn_gradient')),
                                    resol_gradient=bool(config.get('resol_gradient')))
        except ValueError as e:
            raise ValueError("config['second_minimizer_lm']: %s" % e) from None
        _libs = spec_inter.get_libs(batch.names, config)
        optimizer.GradChain.choose_cap(
            S, [_libs[a.name].ntp for a in batch.arms],
            len(names) + (1 if fitVsini else 0),
            2 if fitVsini else (1 if 'vsini' in pd0 else 0), fisher=True)
    if bfgs_jac:
        engine.check_grad_scope(batch, spec_inter.get_libs(batch.names, config),
                                options.get('npoly') or 5,
                                spec_fit._resols(batch, resolParams),
                                bool(options.get('fast_interp')),
                                vsini_grad=fitVsini,
                                nn_gradient=bool(config.get('nn_gradient')),
                                resol_gradient=bool(config.get('resol_gradient')))
        # (and the batch must fit the chain's chunks: known here, not after the
        # simplex stage)
        _libs = spec_inter.get_libs(batch.names, config)
        if not fused_grad:   # (the fused form holds no row buffers to budget)
            optimizer.GradChain.choose_cap(
                S, [_libs[a.name].ntp for a in batch.arms],
                len(names) + (1 if fitVsini else 0),
                2 if fitVsini else (1 if 'vsini' in pd0 else 0))

    # config['fisher_uncertainties']: the joint covariance of (vel, parameters[, vsini])
    # from the Fisher matrix at the returned optimum, beside the Hessian's products.
    # The scope is the gradient's and is checked here, before anything is built
    fisher_unc = bool(config.get('fisher_uncertainties'))
    if fisher_unc and not fused_fisher:   # (fused: checked with the key above)
        try:
            engine.check_grad_scope(batch, spec_inter.get_libs(batch.names, config),
                                    options.get('npoly') or 5,
                                    spec_fit._resols(batch, resolParams),
                                    bool(options.get('fast_interp')),
                                    vsini_grad=fitVsini,
                                    nn_gradient=bool(config.get('nn_gradient')),
                                    resol_gradient=bool(config.get('resol_gradient')))
        except ValueError as e:
            raise ValueError("config['fisher_uncertainties']: %s" % e) from None

    def _tick(k, t0):
        # (stage clocks only when somebody asked for them: the device-wide
        # synchronisation they need would make the two halves of a split batch wait
        # for one another at every stage boundary)
        if timers is None:
            return
        if str(dev).startswith('cuda'):
            torch.cuda.synchronize()
        tm[k] = tm.get(k, 0.) + time.time() - t0

    # vel_fit.py:596-602
    t0 = time.time()
    vg = torch.as_tensor(np.arange(min_vel, max_vel, vel_step0,
                                   dtype=np.float64)).to(dev)
    chisq, st0, _ = spec_fit.chisq_grid_jobs(batch, vg, curparam[:, None, :],
                                             vsini0, options, config,
                                             resol_params=resolParams)
    res, _, mst = engine.grid_moments(chisq.reshape(S, -1), vg, Np=1)
    best_vel = res[:, 1].contiguous()
    _tick('grid0', t0)

    t0 = time.time()
    curval, simplex = _get_simplex_start(best_vel, fixParam, names, pd0,
                                         vsiniMapper, fitVsini)
    mapper = ParamMapper(names, pd0, fixParam, vsiniMapper, fitVsini=fitVsini)
    obj = _Objective(batch, mapper, config, options, priors, resolParams)
    obj.safe_params = curparam
    stats = {}
    libs = spec_inter.get_libs(batch.names, config)

    def process_objective(b, pd, pri, safe):
        # optimizer.ProcessObjective of the batch, or of the spectra of a second run
        return optimizer.ProcessObjective(
            b, libs, names, pd, fixParam, fitVsini, config, options, pri, safe,
            resols=spec_fit._resols(b, resolParams))

    pobj = process_objective(batch, pd0, priors, curparam)
    nm = optimizer.DeviceNelderMead(S, simplex.shape[2], dev).minimize(
        pobj, simplex, fatol=1e-3, xatol=1e-2, maxiter=NM_MAXITER, stats=stats)
    obj.status |= pobj.status
    obj.nfev += pobj.jobs
    slots = pobj.slots
    success = nm['success']
    x, nit, nfev = nm['x'], nm['nit'], nm['nfev']
    redo = torch.nonzero(~success).reshape(-1)
    if redo.numel():
        # vel_fit.py:624-649: a second run restarts from the final simplex; the
        # unconverged spectra form a batch of their own on the same kernels
        sub = batch.subset(redo)
        pobj2 = process_objective(
            sub, {k_: v[redo].contiguous() for k_, v in pd0.items()},
            _subset_priors(priors, redo), curparam[redo].contiguous())
        nm2 = optimizer.DeviceNelderMead(sub.S, simplex.shape[2], dev).minimize(
            pobj2, nm['final_simplex'][0][redo].contiguous(), fatol=1e-3,
            xatol=1e-2, maxiter=NM_MAXITER, stats=stats)
        obj.status[redo] |= pobj2.status
        obj.nfev += pobj2.jobs
        slots += pobj2.slots
        x[redo] = nm2['x']
        success[redo] = nm2['success']
        nit[redo] += nm2['nit']
        nfev[redo] += nm2['nfev']
    _tick('neldermead', t0)

    allidx = torch.arange(S, device=dev)
    # vel_fit.py:653-658: optional BFGS polish from the simplex optimum
    second_run = False
    bfgs_info = None
    lm_info = None
    if lm_polish:
        # Levenberg-Marquardt on (value, gradient, Fisher matrix) rows: the Fisher form
        # of the gradient chain as the objective, its rounds inside the library
        # (RVS_BFGS_ON_DEVICE=0: the same machine on the host around the same chain
        # driven from Python); gtol is the BFGS polish's
        from . import lm
        t0 = time.time()
        jobs_before = pobj.jobs
        slots_before = pobj.slots
        chain = optimizer.GradChain(pobj, fisher=True, fused_fisher=fused_fisher)
        if BFGS_ON_DEVICE:
            br = lm.minimize_lockstep_device(pobj, x, chain=chain)
            x = br['x']
            br = {k_: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v)
                  for k_, v in br.items()}
        else:
            br = lm.minimize_lockstep_native(chain.rows, x.cpu().numpy())
            x = torch.as_tensor(br['x']).to(dev)
        obj.status |= pobj.status
        obj.nfev += pobj.jobs - jobs_before
        slots += pobj.slots - slots_before
        lm_info = dict(nit=br['nit'], nfev=br['nfev'], status=br['status'],
                       mu=br['mu'], fun=br['fun'], rounds=br['rounds'],
                       device=BFGS_ON_DEVICE)
        if fused_fisher:   # (the rows came from rvs_objective_fisher)
            lm_info['fused'] = True
        second_run = True
        _tick('lm', t0)
    elif config.get('second_minimizer'):
        from . import bfgs
        t0 = time.time()
        hess_inv0 = get_hess_inv(mapper.get_fitted_params())
        if bfgs_jac:
            # scipy's jac=True on vel_fit.chisq_func_grad: the gradient chain as the
            # objective, its rounds inside the library (RVS_BFGS_ON_DEVICE=0: the
            # same machine on the host around the same chain driven from Python)
            jobs_before = pobj.jobs
            slots_before = pobj.slots
            chain = optimizer.GradChain(pobj, fused=fused_grad)
            if BFGS_ON_DEVICE:
                br = bfgs.minimize_lockstep_device(pobj, x, hess_inv0=hess_inv0,
                                                   jac=True, chain=chain)
                x = br['x']
                br = {k_: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v)
                      for k_, v in br.items()}
            else:
                br = bfgs.minimize_lockstep_native(chain.rows, x.cpu().numpy(),
                                                   hess_inv0=hess_inv0, jac=True)
                x = torch.as_tensor(br['x']).to(dev)
            obj.status |= pobj.status
            obj.nfev += pobj.jobs - jobs_before
            slots += pobj.slots - slots_before
            bfgs_info = dict(nit=br['nit'], nfev=br['nfev'], njev=br['njev'],
                             status=br['status'], rounds=br['rounds'],
                             device=BFGS_ON_DEVICE, jac=True, fused=fused_grad)
        elif BFGS_ON_DEVICE and optimizer.NATIVE_ROUNDS and pobj.native:
            # the rounds inside the library (rvs_bfgs_run), on the objective the
            # simplex stage ran on
            jobs_before = pobj.jobs
            slots_before = pobj.slots
            br = bfgs.minimize_lockstep_device(pobj, x, hess_inv0=hess_inv0)
            obj.status |= pobj.status
            obj.nfev += pobj.jobs - jobs_before
            slots += pobj.slots - slots_before
            x = br['x']
            bfgs_info = dict(nit=br['nit'].cpu().numpy(),
                             nfev=br['nfev'].cpu().numpy(),
                             status=br['status'].cpu().numpy(),
                             rounds=br['rounds'], device=True)
        else:
            def rows(idx_np, X_np):
                it = torch.as_tensor(idx_np).to(dev)
                return obj(it, torch.as_tensor(X_np).to(dev)).cpu().numpy()

            br = bfgs.minimize_lockstep_native(rows, x.cpu().numpy(),
                                               hess_inv0=hess_inv0,
                                               max_rows=max(S, 1024))
            x = torch.as_tensor(br['x']).to(dev)
            bfgs_info = dict(nit=br['nit'], nfev=br['nfev'], status=br['status'],
                             rounds=br['rounds'], device=False)
        second_run = True
        _tick('bfgs', t0)
    best = mapper.forward(x, allidx)
    nm_vel = best['vel'].contiguous()
    bparams = best['params'].contiguous()
    bvsini = best['vsini']

    # vel_fit.py:672-682
    t0 = time.time()
    vel_in = nm_vel.cpu().numpy()
    r = _minimum_sampler_batch(batch, vel_in, bparams, bvsini, config, options,
                               resolParams=resolParams)
    best_vel = torch.as_tensor(r['best_vel']).to(dev)
    _tick('vel_refine', t0)

    # vel_fit.py:689-696
    t0 = time.time()
    outp = spec_fit.get_chisq(batch, best_vel, bparams,
                              None if bvsini is None else bvsini, resolParams,
                              options=options, config=config, full_output=True)
    _tick('full_output', t0)

    # vel_fit.py:699-725: Hessian of 0.5*chisq_func0 in ALL stellar parameters
    # at the optimiser's velocity (best_param is not updated by the refinement)
    t0 = time.time()

    diag_err, covar, bad_hessian = _hessian_stage(obj, names, nm_vel, bparams,
                                                  bvsini)
    _tick('hessian', t0)

    ret = {}
    if is_batch:
        ret['param'] = {k: bparams[:, i] for i, k in enumerate(names)}
        if fitVsini:
            ret['vsini'] = bvsini
        ret['vel'] = best_vel
        ret['vel_err'] = torch.as_tensor(r['vel_err']).to(dev)
        ret['vel_skewness'] = torch.as_tensor(r['skewness']).to(dev)
        ret['vel_kurtosis'] = torch.as_tensor(r['kurtosis']).to(dev)
        ret['param_err'] = {k: diag_err[:, i] for i, k in enumerate(names)}
        ret['param_covar'] = covar
        ret['minimize_success'] = success
        ret['bad_hessian'] = bad_hessian
        ret['yfit'] = outp['models']
        ret['raw_models'] = outp['raw_models']
        ret['chisq'] = outp['chisq']
        ret['logl'] = outp['logl']
        ret['chisq_array'] = outp['chisq_array']
        ret['npix_array'] = outp['npix_array']
        ret['status'] = obj.status | outp['status'] | st0.reshape(S, -1)[:, 0]
    else:
        if int(obj.status[0].item()) & _lib_nonfinite():
            raise RuntimeError('non-finite likelihood during the optimisation')
        bp = bparams[0].cpu().numpy()
        ret['param'] = dict(zip(names, [float(_) for _ in bp]))
        if fitVsini:
            ret['vsini'] = float(bvsini[0].item())
        ret['vel'] = float(r['best_vel'][0])
        ret['vel_err'] = float(r['vel_err'][0])
        ret['vel_skewness'] = float(r['skewness'][0])
        ret['vel_kurtosis'] = float(r['kurtosis'][0])
        ret['param_err'] = dict(zip(names, diag_err[0]))
        ret['param_covar'] = covar[0]
        ret['minimize_success'] = bool(success[0].item())
        ret['bad_hessian'] = bool(bad_hessian[0])
        ret['yfit'] = [m[0].cpu().numpy() for m in outp['models']]
        ret['raw_models'] = [m[0].cpu().numpy() for m in outp['raw_models']]
        ret['chisq'] = float(outp['chisq'][0].item())
        ret['logl'] = -0.5 * ret['chisq']
        ret['chisq_array'] = [float(_) for _ in outp['chisq_array'][0]]
        ret['npix_array'] = [int(_) for _ in outp['npix_array'][0]]
    if fisher_unc:
        t0 = time.time()
        fu = fisher_uncertainties(batch if is_batch else specdata, best_vel, bparams,
                                  bvsini, options=options, config=config,
                                  priors=priors, fixParam=fixParam, vsini_grad=fitVsini,
                                  resolParams=resolParams)
        ret['covar_fisher'] = fu['covar']
        ret['names_fisher'] = fu['names']
        ret['vel_err_fisher'] = torch.as_tensor(fu['vel_err']).to(dev) if is_batch \
            else fu['vel_err']
        ret['param_err_fisher'] = fu['param_err']
        _tick('fisher', t0)
    ret['nm_vel'] = nm_vel if is_batch else float(nm_vel[0].item())
    ret['nm_nit'] = nit if is_batch else int(nit[0].item())
    ret['nm_nfev'] = nfev if is_batch else int(nfev[0].item())
    ret['nm_rounds'] = stats.get('rounds', 0)
    ret['objective_evals'] = obj.nfev
    # rows the lock-step Nelder-Mead launched (an upper bound known on the host);
    # the rows behind the device counts are skipped by the objective kernel
    ret['nm_launched_rows'] = slots
    ret['second_minimizer_run'] = second_run
    if bfgs_info is not None:
        ret['bfgs'] = bfgs_info
    if lm_info is not None:
        ret['lm'] = lm_info
    ret['optimizer_run'] = True
    return ret


def _lib_nonfinite():
    from . import _lib
    return _lib.ST_NONFINITE


# --------------------------------------------------------------------------
# the joint fit of a star's epochs: shared parameters, one velocity each
# --------------------------------------------------------------------------
def _epochs_batch(specdata):
    """SpecBatch of the epochs: a SpecBatch as it is, or a list of epochs, each the list
    of SpecData of its arms (the same arms in every epoch)"""
    if isinstance(specdata, SpecBatch):
        return specdata
    epochs = [list(e) if isinstance(e, (list, tuple)) else [e] for e in specdata]
    if not epochs:
        raise ValueError('process_epochs: no epochs')
    arms = [sd.name for sd in epochs[0]]
    for i, e in enumerate(epochs):
        if [sd.name for sd in e] != arms:
            raise ValueError('process_epochs: epoch %d has the arms %s, epoch 0 has %s'
                             % (i, [sd.name for sd in e], arms))
    return SpecBatch.from_specdata(epochs)


def _arrow_uncertainties(rows, m, eoff):
    """Uncertainties from the arrow rows (alm.row_size) at the optimum, mu = 0, on the
    host.  The rows hold the Gauss-Newton Hessian of chi^2, twice the Fisher matrix:
    with S = Htt - sum_e c_e c_e^T / h_e the parameter covariance is 2 S^-1 (through
    _uncertainties_from_hessians after the symmetric scaling _uncertainties_from_fisher
    uses) and the variance of a velocity, marginalised over the parameters, is
    2 (1 / h_e + c_e^T S^-1 c_e / h_e^2).  Returns theta_err [N, m], covar [N, m, m],
    vel_err [S] (nan where h_e <= 0), bad [N]."""
    from . import alm
    eoff = np.asarray(eoff, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.float64)
    N = len(eoff) - 1
    nE = np.diff(eoff)
    ro = alm.offsets(m, eoff)[1]
    il = np.tril_indices(m)
    head = 1 + m + len(il[0])
    Sm = np.zeros((N, m, m))
    groups = []
    # (stars of the same number of epochs together: their rows are one 2-d block)
    for E in np.unique(nE):
        sel = np.nonzero(nE == E)[0]
        R = rows[ro[sel, None] + np.arange(alm.row_size(m, int(E)))[None, :]]
        H = np.zeros((len(sel), m, m))
        H[:, il[0], il[1]] = R[:, 1 + m:head]
        H[:, il[1], il[0]] = R[:, 1 + m:head]
        rec = R[:, head:].reshape(len(sel), int(E), 2 + m)
        h, c = rec[:, :, 1], rec[:, :, 2:]
        with np.errstate(all='ignore'):
            Sm[sel] = H - np.einsum('kei,kej->kij', c / h[:, :, None], c)
        groups.append((sel, h, c))
    M = 0.5 * Sm
    d = np.diagonal(M, axis1=1, axis2=2)
    with np.errstate(all='ignore'):
        sc = np.where(d > 0, 1. / np.sqrt(np.where(d > 0, d, 1.)), 1.)
    err, inv, bad = _uncertainties_from_hessians(M * sc[:, :, None] * sc[:, None, :])
    err, covar = err * sc, inv * sc[:, :, None] * sc[:, None, :]
    vel_err = np.full(int(eoff[-1]), np.nan)
    for sel, h, c in groups:
        with np.errstate(all='ignore'):
            # (covar = 2 S^-1)
            var = 2.0 / h + np.einsum('kei,kij,kej->ke', c, covar[sel], c) / (h * h)
            ve = np.sqrt(var)
        ve[~(h > 0)] = np.nan
        vel_err[(eoff[sel, None] + np.arange(h.shape[1])[None, :]).reshape(-1)] = \
            ve.reshape(-1)
        bad[sel] |= ~np.isfinite(ve).all(axis=1)
    return err, covar, vel_err, bad


def process_epochs(specdata, star, paramDict0, vel0, fixParam=None, options=None,
                   config=None, resolParams=None, priors=None, gtol=1e-5,
                   cap_star=None, cap_epoch=None):
    """The joint fit of the epochs of N stars: ONE set of stellar parameters (and one
    vsini) per star, one velocity per epoch -- Levenberg-Marquardt (alm.py) on the sum
    of the epochs' objectives, whose Gauss-Newton matrix is an arrowhead.  The template
    stage of a row runs once per star, not once per epoch (optimizer.EpochChain).

    specdata     a SpecBatch of the S epochs, or a list of epochs, each the list of
                 SpecData of its arms
    star         int [S]: the star (0 .. N - 1) of every epoch, in any order
    paramDict0   the start, one value per star ([N] or a scalar): the stellar
                 parameters, and 'vsini' where the templates are broadened (fitted
                 unless it is in fixParam)
    vel0         [S] start velocities in km/s (epochs_start: from a per-epoch run)
    priors       {name: (mean, sigma)} per star, counted once per star
    Returns numpy arrays: vel, vel_err, chisq [S] in the order of the input; param,
    param_err {name: [N]}; vsini, vsini_err [N] where fitted; param_covar [N, m, m] over
    the fitted columns ([vsini,] free parameters); chisq_tot (with the priors), status
    (alm.py), nit, nfev, bad_fisher [N]; spec_status [N].  The uncertainties are those
    of the arrow matrix at the returned point (_arrow_uncertainties).  The scope is the
    analytic gradient's (engine.check_grad_scope); anything else raises ValueError."""
    from . import alm
    if config is None:
        raise RuntimeError('Config must be provided')
    t_begin = time.time()
    options = options or {}
    fixParam = list(fixParam) if fixParam is not None else []
    batch = _epochs_batch(specdata)
    S, dev = batch.S, batch.device
    vel0 = np.asarray(vel0, dtype=np.float64).reshape(-1)
    if vel0.shape != (S, ):
        raise ValueError('vel0 has %d entries, there are %d epochs' % (len(vel0), S))
    lens = {np.size(v) for v in paramDict0.values()} - {1}
    if len(lens) > 1:
        raise ValueError('paramDict0: values of %s stars' % sorted(lens))
    order, eoff = spec_fit.epochs_order(star, S, lens.pop() if lens else None)
    N = len(eoff) - 1
    names = spec_inter.getSpecParams(batch.names[0], config)
    missing = [k for k in names if k not in paramDict0]
    if missing:
        raise ValueError('paramDict0 lacks %s' % missing)
    pd0 = _as_param_tensors(paramDict0, N, dev)
    fitVsini = 'vsini' in pd0 and 'vsini' not in fixParam
    if not np.array_equal(order, np.arange(S)):
        batch = batch.subset(torch.as_tensor(order).to(dev))
    libs = spec_inter.get_libs(batch.names, config)
    if config.get('fused_gradient'):
        engine.check_fused_grad_scope(batch, libs, options.get('npoly') or 5,
                                      what='the joint fit of a star\'s epochs '
                                           '(process_epochs: its rows are Fisher rows)')
    if config.get('fused_fisher'):
        engine.check_fused_fisher_scope(batch, libs, options.get('npoly') or 5,
                                        what='the joint fit of a star\'s epochs '
                                             '(process_epochs)')
    safe = torch.stack([pd0[_] for _ in names], dim=1)
    try:
        chain = optimizer.EpochChain(
            batch, libs, names, pd0, fixParam, fitVsini, config, options, priors, safe,
            eoff, resols=spec_fit._resols(batch, resolParams), cap_star=cap_star,
            cap_epoch=cap_epoch)
    except ValueError as e:
        raise ValueError('process_epochs: %s' % e) from None
    m = chain.m
    fitted = (['vsini'] if fitVsini else []) + [k for k in names if k not in fixParam]
    th0 = np.stack([pd0[k].cpu().numpy() for k in fitted], axis=1)
    xo = alm.offsets(m, eoff)[0]
    x0 = np.empty(xo[-1])
    vs = vel0[order]
    for n in range(N):
        x0[xo[n]:xo[n] + m] = th0[n]
        x0[xo[n] + m:xo[n + 1]] = vs[eoff[n]:eoff[n + 1]]
    t_setup = time.time()
    # the rounds inside the library (rvs_alm_run); RVS_BFGS_ON_DEVICE=0: the same
    # machines on the host around the same chain driven from Python
    if BFGS_ON_DEVICE:
        res = alm.minimize_lockstep_device(chain, x0, gtol=gtol)
    else:
        res = alm.minimize_lockstep_native(chain.objective, m, eoff, x0, gtol=gtol)
    t_min = time.time()
    x = res['x']
    at = xo[:-1, None] + np.arange(m)[None, :]
    isvel = np.ones(int(xo[-1]), dtype=bool)
    isvel[at.reshape(-1)] = False
    theta, vel_s = x[at], x[isvel]
    if 'chi_x' in res:
        # the device rounds kept the epochs' chi at x; the mapping of theta is host
        # arithmetic (a fitted column as it is, vsini clipped; a star whose first row
        # was bad keeps its start, which is what `safe` holds)
        rows = res['row']
        ro_ = alm.offsets(m, eoff)[1]
        started = ~np.isnan(res['chi_x'][eoff[:-1]])
        rows = rows.copy()
        rows[ro_[:-1][~started]] = res['fun'][~started]
        th0c = th0.copy()
        use = np.where(started[:, None], theta, th0c)
        ep = dict(chi=res['chi_x'],
                  params=np.stack([use[:, fitted.index(k)] if k in fitted
                                   else pd0[k].cpu().numpy() for k in names], axis=1),
                  vsini=np.clip(use[:, 0], 0.0, float(config['max_vsini']))
                  if fitVsini else None)
    else:
        # the epochs' own chi^2 at the result (and the row the uncertainties come from)
        chain.keep_epochs = 'values'
        rows = chain.rows(np.arange(N), theta, vel_s)
        chain.keep_epochs = False
        ep = chain.epochs
    terr, covar, verr_s, bad = _arrow_uncertainties(rows, m, eoff)
    inv = np.empty(S, dtype=np.int64)
    inv[order] = np.arange(S)
    ret = dict(vel=vel_s[inv], vel_err=verr_s[inv], chisq=ep['chi'][inv])
    ret['param'] = {k: ep['params'][:, i].copy() for i, k in enumerate(names)}
    nan = np.full(N, np.nan)
    ret['param_err'] = {k: (terr[:, fitted.index(k)] if k in fitted else nan.copy())
                        for k in names}
    if fitVsini:
        ret['vsini'] = ep['vsini'].copy()
        ret['vsini_err'] = terr[:, 0]
    ret['param_covar'] = covar
    ret['names_covar'] = fitted
    ro = alm.offsets(m, eoff)[1]
    ret['chisq_tot'] = rows[ro[:-1]].copy()
    ret['status'], ret['nit'], ret['nfev'] = res['status'], res['nit'], res['nfev']
    ret['bad_fisher'] = bad
    ret['spec_status'] = chain.status.cpu().numpy()
    ret['rounds'] = res['rounds']
    ret['template_rows'], ret['epoch_jobs'] = chain.star_rows, chain.epoch_jobs
    ret['seconds'] = dict(setup=t_setup - t_begin, minimise=t_min - t_setup,
                          closing=time.time() - t_min)
    return ret


def epochs_start(results, star):
    """The start of process_epochs from a per-epoch `process` run: `results` is its
    batch output (or a list of its single-spectrum dicts), `star` int [S].  Returns
    (paramDict0, vel0): the velocities as fitted; every parameter the inverse-variance
    mean over the star's epochs of `param` with `param_err`, and the plain mean where an
    error is not finite or not positive ('vsini' likewise, with the plain mean: process
    gives it no error)."""
    def arr(v):
        return v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)

    if isinstance(results, (list, tuple)):
        keys = list(results[0]['param'])
        results = dict(
            vel=np.array([r['vel'] for r in results]),
            param={k: np.array([r['param'][k] for r in results]) for k in keys},
            param_err={k: np.array([r['param_err'][k] for r in results]) for k in keys},
            **({'vsini': np.array([r['vsini'] for r in results])}
               if 'vsini' in results[0] else {}))
    vel0 = arr(results['vel']).astype(np.float64)
    S = len(vel0)
    order, eoff = spec_fit.epochs_order(star, S)
    N = len(eoff) - 1
    star = np.asarray(star)
    pd = {}
    for k, v in results['param'].items():
        v = arr(v).astype(np.float64)
        e = arr(results['param_err'][k]).astype(np.float64)
        out = np.empty(N)
        for n in range(N):
            sel = star == n
            en = e[sel]
            if np.isfinite(en).all() and (en > 0).all():
                w = 1.0 / (en * en)
                out[n] = (w * v[sel]).sum() / w.sum()
            else:
                out[n] = v[sel].mean()
        pd[k] = out
    if 'vsini' in results:
        v = arr(results['vsini']).astype(np.float64)
        pd['vsini'] = np.array([v[star == n].mean() for n in range(N)])
    return pd, vel0
