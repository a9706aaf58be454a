"""The reference's regularize_grid under its names: the rows of a template grid with
holes (missing models, alpha planes that exist only for some feh, a coarse feh axis) ->
the rows of a complete (teff, logg) footprint x new feh grid x new alpha grid, by
multiquadric interpolation in rank coordinates, window of teff values by window, on the
device (rbf.RBFInterpolator).

regularize is converter's body (regularize_grid.py:45-151) without its files: it takes
what make_interpol.build_specs returns and returns the same dictionary with `specs` and
`vec` replaced, so that make_nd.regular_library and make_ccf.build_ccf_set take it
unchanged.
"""
import numpy as np
import torch

from . import rbf

OPTIONS = dict(smooth=0., min_feh=-4., max_feh=1.2, step_feh=.25, min_alpha=-.4,
               max_alpha=1.2, step_alpha=.2)


def findbestoverlaps(x, intervals):
    """for every x the index of the interval it lies deepest inside (the first one on
    ties): intervals [0,10], [1,11], .., [6,16] and x = 8 give [3,13]"""
    x = np.asarray(x)
    depth = np.array([(x - i[0]) * (x - i[-1]) for i in intervals]).reshape(
        len(intervals), len(x))
    depth = np.minimum(depth, 1e10)
    best = np.argmin(depth, axis=0)            # argmin takes the first of equal values
    best[depth.min(axis=0) >= 1e10] = 0
    return best


def check_holes_2d(x, y):
    """raises when the (x, y) locations form a grid with a hole: a missing interior
    node of which at least three diagonal neighbours exist"""
    ux, ix = np.unique(x, return_inverse=True)
    uy, iy = np.unique(y, return_inverse=True)
    have = np.zeros((len(ux) + 2, len(uy) + 2), dtype=int)
    have[np.ravel(ix) + 1, np.ravel(iy) + 1] = 1
    inner = have[1:-1, 1:-1]
    diag = have[:-2, :-2] + have[2:, 2:] + have[:-2, 2:] + have[2:, :-2]
    interior = np.zeros_like(inner, dtype=bool)
    interior[1:-1, 1:-1] = True
    if np.any((inner == 0) & interior & (diag >= 3)):
        raise Exception('the grid has holes')


def rank_mappers(axes):
    """the reference's axis mappers (regularize_grid.py:76-82): per axis the smoothing
    spline through (value, rank) with FITPACK's default smoothing -- not s = 0.  scipy
    (>= 1.9, as the reference asks) is imported here and nowhere else in the package."""
    import scipy.interpolate
    import scipy.version
    if [int(_) for _ in scipy.version.version.split('.')[:2]] < [1, 9]:
        raise RuntimeError('scipy 1.9.0+ is required')
    return [scipy.interpolate.UnivariateSpline(u, np.arange(len(u)),
                                               k=min(3, len(u) - 1)) for u in axes]


def plan(vec, min_feh=-4., max_feh=1.2, step_feh=.25, min_alpha=-.4, max_alpha=1.2,
         step_alpha=.2, width=12, mappers=None):
    """The bookkeeping of converter, host only: the mapped nodes [N, 4], and per window
    of `width` + 1 consecutive teff values (rows, points [4, M] in physical units, mapped
    points [M, 4]) -- the rows it is fitted through and the points it predicts, which are
    the footprint nodes that lie deepest in it x the new feh grid x the new alpha grid."""
    vec = np.asarray(vec, dtype=np.float64)
    if vec.shape[0] != 4:
        raise ValueError('regularize: (teff, logg, feh, alpha) grids only')
    # half a step more so that the last value is included
    newfeh = np.arange(min_feh, max_feh + step_feh / 2., step_feh)
    newalpha = np.arange(min_alpha, max_alpha + step_alpha / 2., step_alpha)
    teff, logg = vec[0], vec[1]
    uteff, teffid = np.unique(teff, return_inverse=True)
    teffid = np.ravel(teffid)
    axes = [uteff] + [np.unique(v) for v in vec[1:]]
    if mappers is None:
        mappers = rank_mappers(axes)
    ymap = np.array([np.asarray(mappers[i](vec[i]), dtype=np.float64)
                     for i in range(4)]).T
    # the footprint in the order the reference meets it (a set of float pairs)
    foot = np.array(list(set(zip(teff.tolist(), logg.tolist())))).T
    check_holes_2d(teff, logg)
    foot_rank = np.digitize(foot[0], uteff) - 1
    edges = np.arange(0, max(1, len(uteff) - width))
    intervals = np.array([(e, e + width) for e in edges])
    best = findbestoverlaps(foot_rank, intervals)
    windows = []
    for ii, (e1, e2) in enumerate(intervals):
        rows = np.nonzero((teffid >= e1) & (teffid <= e2))[0]
        sel = best == ii
        shape = (int(sel.sum()), len(newfeh), len(newalpha))
        pts = np.array([
            np.broadcast_to(foot[0][sel][:, None, None], shape).ravel(),
            np.broadcast_to(foot[1][sel][:, None, None], shape).ravel(),
            np.broadcast_to(newfeh[None, :, None], shape).ravel(),
            np.broadcast_to(newalpha[None, None, :], shape).ravel()])
        mapped = np.array([np.asarray(mappers[i](pts[i]), dtype=np.float64)
                           for i in range(4)]).T.reshape(-1, 4)
        windows.append((rows, pts, mapped))
    return ymap, windows


def regularize(specs_dict, smooth=0., min_feh=-4., max_feh=1.2, step_feh=.25,
               min_alpha=-.4, max_alpha=1.2, step_alpha=.2, width=12, mappers=None):
    """converter on a dictionary.  specs_dict: what make_interpol.build_specs returns
    (`specs` a device tensor or an array [T, npix], float32 or float64; `vec` [4, T]).
    Returns a copy with `specs` (a device tensor of the same dtype, made and kept on the
    device) and `vec` replaced, rows in the reference's order: window by window,
    footprint point x feh x alpha.  `mappers`: four callables value -> rank coordinate
    instead of the reference's splines.  The other keys are passed on as they are (as
    the reference does; `lognorms` keeps the length of the input)."""
    D = dict(specs_dict)
    specs = D['specs']
    if not isinstance(specs, torch.Tensor):
        specs = torch.as_tensor(np.ascontiguousarray(specs))
    specs = specs.to('cuda') if specs.device.type == 'cpu' else specs
    if specs.dtype != torch.float32:
        specs = specs.to(torch.float64)
    if specs.shape[0] != np.shape(D['vec'])[1]:
        raise ValueError('regularize: %d rows for %d parameter vectors'
                         % (specs.shape[0], np.shape(D['vec'])[1]))
    ymap, windows = plan(D['vec'], min_feh, max_feh, step_feh, min_alpha, max_alpha,
                         step_alpha, width, mappers)
    total = sum(w[1].shape[1] for w in windows)
    out = torch.empty((total, specs.shape[1]), dtype=specs.dtype, device=specs.device)
    done = 0
    for rows, pts, mapped in windows:
        m = pts.shape[1]
        if m == 0:
            continue
        idx = torch.as_tensor(rows, device=specs.device)
        rr = rbf.RBFInterpolator(ymap[rows], specs.index_select(0, idx),
                                 smoothing=smooth, kernel='multiquadric', epsilon=1.,
                                 device=specs.device)
        rr(mapped, out=out[done:done + m])
        del rr
        done += m
    D['specs'] = out
    D['vec'] = np.concatenate([w[1] for w in windows], axis=1)
    return D
