"""regularize_grid on the device (rbf.RBFInterpolator, regularize_grid.regularize,
TemplateLibrary.from_models(regularize=...)) against the reference's converter
(tests/golden/regularize_cases.npz), scipy's RBFInterpolator and the long-double truth
of tests/rbf_truth.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rbf_truth  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')


def _ordered(a):
    """float32 -> integers whose differences count representable values"""
    v = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(v < 0, -(v & 0x7fffffff), v)


def _scipy(y, d, x, smooth):
    import scipy.interpolate
    return scipy.interpolate.RBFInterpolator(y, d, smoothing=smooth,
                                             kernel='multiquadric', epsilon=1)(x)


def _windows(name):
    """per window of a golden case: (nodes, rows, points, golden rows)"""
    from rvspecfit_amd import regularize_grid
    g = np.load(os.path.join(GOLD, 'regularize_cases.npz'))
    D, opts = rbf_truth.case_inputs(name)
    smooth = opts.pop('smooth')
    ymap, wins = regularize_grid.plan(D['vec'], **opts)
    out, done = [], 0
    for rows, pts, mapped in wins:
        m = pts.shape[1]
        out.append((ymap[rows], D['specs'][rows], mapped,
                    g[name + '/specs'][done:done + m]))
        done += m
    return out, smooth


def _accuracy(tag, y, d, x, smooth):
    """e_ref = max |scipy - truth| and e_dev = max |device - truth| on the same
    columns; the device may be 4 times as far as scipy, for another elimination and
    summation order on the same condition number, no more"""
    from rvspecfit_amd import rbf
    truth = rbf_truth.interpolate(y, d, x, smooth)
    ref = _scipy(y, d, x, smooth)
    dev = rbf.RBFInterpolator(y, d, smoothing=smooth)(x).cpu().numpy()
    e_ref = float(np.abs(ref - truth).max())
    e_dev = float(np.abs(dev - truth).max())
    print('%s: N %d S %d M %d  e_ref %.3e  e_dev %.3e' % (tag, len(y), d.shape[1],
                                                         len(x), e_ref, e_dev))
    assert np.all(np.isfinite(dev))
    assert e_dev <= 4 * e_ref
    return e_ref


@pytest.mark.parametrize('name', list(rbf_truth.CASES))
def test_windows_against_the_truth(name):
    wins, smooth = _windows(name)
    for i, (y, d, x, gold) in enumerate(wins):
        _accuracy('%s window %d' % (name, i), y, d, x, smooth)


def test_large_window_against_the_truth():
    """one window of the size of a real grid's: about 3000 nodes of a holey 4-D grid in
    the rank coordinates of uneven axes"""
    from rvspecfit_amd import regularize_grid, synth
    axes = ([3500., 3600., 3700., 3800., 4000., 4250., 4500., 5000., 5500., 6000., 7000.,
             8000., 10000.], np.linspace(0., 5., 7), [-4., -3., -2.5, -2., -1.5, -1.,
                                                       -0.5, 0., 0.5], np.linspace(0, .8, 5))
    _, vec = synth.regular_grid(axes=axes)
    rng = np.random.default_rng(5)
    vec = vec[:, rng.random(vec.shape[1]) >= 0.25]
    mappers = regularize_grid.rank_mappers([np.asarray(a, dtype=float) for a in axes])
    y = np.array([mappers[i](vec[i]) for i in range(4)]).T
    lam = np.linspace(4500., 4530., 4)
    d = np.array([np.log(synth.spectrum(lam, *v)) for v in vec.T])
    x = rng.random((300, 4)) * (y.max(axis=0) - y.min(axis=0)) + y.min(axis=0)
    assert 2900 < len(y) < 3250
    _accuracy('large', y, d, x, 0.)


@pytest.mark.parametrize('name', list(rbf_truth.CASES))
@pytest.mark.parametrize('bits', [64, 32])
def test_regularize_against_the_reference(name, bits):
    """regularize on what build_specs returns against converter's file: vec and the row
    order exactly; float64 rows within e_dev + e_ref <= 5 e_ref of the reference's;
    float32 rows 2 ulp from float32(reference), or that absolute floor"""
    import torch
    from rvspecfit_amd import regularize_grid
    g = np.load(os.path.join(GOLD, 'regularize_cases.npz'))
    D, opts = rbf_truth.case_inputs(name)
    wins, smooth = _windows(name)
    e_ref = max(float(np.abs(_scipy(y, d, x, smooth)
                             - rbf_truth.interpolate(y, d, x, smooth)).max())
                for y, d, x, _ in wins)
    dt = torch.float64 if bits == 64 else torch.float32
    D['specs'] = torch.as_tensor(D['specs']).to('cuda').to(dt)
    R = regularize_grid.regularize(D, **opts)
    assert R['specs'].is_cuda and R['specs'].dtype == dt
    assert sorted(R) == sorted(D)
    assert np.array_equal(R['vec'], g[name + '/vec'])
    got = R['specs'].cpu().numpy()
    want = g[name + '/specs']
    assert got.shape == want.shape and np.all(np.isfinite(got))
    dev = np.abs(got.astype(np.float64) - want)
    if bits == 64:
        print('%s: max |device - reference| %.3e, e_ref %.3e' % (name, dev.max(), e_ref))
        assert dev.max() <= 5 * e_ref
        return
    # float32 rows in: the interpolant of the rounded rows against the reference's of
    # the same rounded rows
    want32 = np.concatenate([_scipy(y, d.astype(np.float32).astype(np.float64), x, smooth)
                             for y, d, x, _ in wins]).astype(np.float32)
    ulp = np.abs(_ordered(got) - _ordered(want32))
    dev = np.abs(got.astype(np.float64) - want32.astype(np.float64))
    print('%s: %d x %d values, bit-equal %.6f, one ulp %.2e, more %d, max |diff| %.2e'
          % (name, got.shape[0], got.shape[1], np.mean(ulp == 0), np.mean(ulp == 1),
             int(np.sum(ulp > 1)), dev.max()))
    assert np.all((ulp <= 2) | (dev <= 5 * e_ref))
    assert np.mean(ulp == 0) > 0.97


def test_the_interpolant_interpolates():
    """smooth = 0: the output rows at nodes the input has are the input's rows, as
    closely as the reference's own (times the factor of the accuracy tests)"""
    import torch
    from rvspecfit_amd import regularize_grid
    name = 'windows'
    g = np.load(os.path.join(GOLD, 'regularize_cases.npz'))
    D, opts = rbf_truth.case_inputs(name)
    assert opts['smooth'] == 0
    rows_in = D['specs']
    R = regularize_grid.regularize(dict(D, specs=torch.as_tensor(rows_in).to('cuda')),
                                   **opts)
    got = R['specs'].cpu().numpy()
    key = lambda v: tuple(np.round(v, 6))
    where = {key(v): i for i, v in enumerate(D['vec'].T)}
    pairs = [(o, where[key(v)]) for o, v in enumerate(R['vec'].T) if key(v) in where]
    assert len(pairs) > 500
    o, i = np.array(pairs).T
    e_ref = np.abs(g[name + '/specs'][o] - rows_in[i]).max()
    e_dev = np.abs(got[o] - rows_in[i]).max()
    print('at %d input nodes: reference %.3e, device %.3e' % (len(o), e_ref, e_dev))
    assert e_dev <= 4 * e_ref


@pytest.mark.parametrize('N,S,M,f32', [(200, 7, 33, False), (37, 1, 1, False),
                                       (64, 3, 64, True), (129, 130, 65, True),
                                       (500, 257, 200, False)])
def test_interpolator_against_scipy(N, S, M, f32):
    """shapes that are no multiple of a tile, fewer nodes than one panel, one column,
    one point; float32 and float64 values; a vector of smoothing values.  With a
    handful of outputs (one, for M = S = 1) max |scipy - truth| is no measure of scipy's
    error: a single value can be right to the last bit by luck.  The bound is therefore
    4 times the larger of it and one float64 rounding of the sum as it has to be formed,
    eps * max_m sum_j |K(x_m, y_j)| |c_j| (c from the truth): no evaluation in float64
    can promise less."""
    import torch
    from rvspecfit_amd import rbf
    rng = np.random.default_rng(N)
    y = rng.random((N, 3)) * 6
    d = np.sin(y.sum(axis=1))[:, None] + 0.1 * rng.standard_normal((N, S))
    if f32:
        d = d.astype(np.float32)
    x = rng.random((M, 3)) * 6
    sm = 1e-3 * (1 + rng.random(N))
    want = _scipy(y, d.astype(np.float64), x, sm)
    truth = rbf_truth.interpolate(y, d.astype(np.float64), x, sm)
    c, lam, _ = rbf_truth.solve(y, d.astype(np.float64), sm)
    floor = float(np.finfo(np.float64).eps * (
        np.abs(rbf_truth._kernel(x, y, 1.)) @ np.abs(c) + np.abs(lam)[None, :]).max())
    e_ref = max(float(np.abs(want - truth).max()), floor)
    rr = rbf.RBFInterpolator(torch.as_tensor(y).to('cuda') if f32 else y, d, smoothing=sm)
    got = rr(x)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (M, S)
    e_dev = np.abs(got.cpu().numpy() - truth).max()
    print('N %d S %d M %d: e_ref %.3e (floor %.3e) e_dev %.3e' % (N, S, M, e_ref, floor,
                                                                e_dev))
    assert e_dev <= 4 * e_ref
    # 1-D values as scipy takes them; epsilon scales the coordinates
    r1 = rbf.RBFInterpolator(y * 2, d[:, 0], smoothing=sm, epsilon=0.5)(x * 2)
    assert tuple(r1.shape) == (M, )
    assert np.abs(r1.cpu().numpy() - truth[:, 0]).max() <= 4 * e_ref + 1e-14


def test_error_paths():
    """a holey footprint raises as the reference's check does; non-finite rows raise; a
    duplicate node (a singular system) raises and nothing is returned"""
    import torch
    from rvspecfit_amd import rbf, regularize_grid
    D, opts = rbf_truth.case_inputs('single')
    teff, logg = D['vec'][0], D['vec'][1]
    cut = (teff == 5500.) & (logg == 3.)
    H = dict(D, specs=D['specs'][~cut], vec=D['vec'][:, ~cut])
    with pytest.raises(Exception, match='the grid has holes'):
        regularize_grid.regularize(H, **opts)
    bad = D['specs'].copy()
    bad[17, 3] = np.nan
    with pytest.raises(ValueError, match='not finite'):
        regularize_grid.regularize(dict(D, specs=bad), **opts)
    y = np.random.default_rng(0).random((90, 4))
    y[70] = y[3]
    with pytest.raises(np.linalg.LinAlgError, match='Singular'):
        rbf.RBFInterpolator(y, np.ones((90, 2)))
    with pytest.raises(ValueError, match='not finite'):
        rbf.RBFInterpolator(np.where(np.arange(360).reshape(90, 4) == 5, np.inf, y),
                            np.ones((90, 2)))
    assert torch.cuda.is_available()


GRID4 = dict(nteff=4, nlogg=4, nfeh=4, nalpha=4, teff_range=(3500., 7500.),
             logg_range=(1., 4.), feh_range=(-2., 0.), alpha_range=(0., 0.6))


def _holey_models():
    """high-resolution models of a 4^4 grid with alpha != 0 missing at both ends of the
    feh axis and the nodes around (4833, 2, -0.667, 0.2) missing"""
    from rvspecfit_amd import synth
    u, vec = synth.regular_grid(**GRID4)
    teff, logg, feh, alpha = vec
    keep = ~((alpha != 0) & ((feh == u[2][0]) | (feh == u[2][-1])))
    keep &= ~((teff == u[0][1]) & (logg == u[1][1]) & (alpha == u[3][1]))
    keep &= ~((teff == u[0][2]) & (logg == u[1][2]) & (feh == u[2][2]))
    vec = vec[:, keep]
    lam_hr = np.linspace(4300, 5040, 37001)
    rows = np.array([synth.spectrum(lam_hr, *v) for v in vec.T], dtype=np.float32)
    return lam_hr, rows, vec


def test_from_models_fills_the_holes():
    """from_models(regularize={...}, ccf={...}) on a holey grid: a library without holes
    inside the footprint and a CCF set; fitter_ccf.fit and vel_fit.process on stars
    whose parameters lie in a former hole find the velocity within the bound of
    test_fit_fake (the reference's own pin); regularize=None is what it was"""
    import torch
    from rvspecfit_amd import (fitter_ccf, make_interpol, make_nd, regularize_grid,
                               spec_fit, spec_inter, synth, vel_fit)
    from rvspecfit_amd.library import TemplateLibrary
    from conftest import GOLD_CONFIG
    d = np.load(os.path.join(GOLD, 'lib_gold_b.npz'))
    conf = dict(logl0=float(d['ccf_logl0']), logl1=float(d['ccf_logl1']),
                npoints=int(d['ccf_npoints']), continuum=True,
                maxcontpts=int(d['ccf_maxcontpts']),
                splinestep=float(d['ccf_splinestep']))
    lam_hr, rows, vec = _holey_models()
    setup = ('gold_b', 4380., 4740., make_interpol.Resolution(resol=2000.), 0.4, True)
    opts = dict(min_feh=-2., max_feh=0., step_feh=.5, min_alpha=0., max_alpha=.6,
                step_alpha=.2)
    S = make_interpol.build_specs(lam_hr, rows, vec, setup)
    plain = make_nd.regular_library(S)
    assert (plain['idgrid'] < 0).sum() > 20
    lib0 = TemplateLibrary.from_models('gold_b', lam_hr, rows, vec, setup)
    assert torch.equal(lib0.dats, TemplateLibrary('gold_b', plain).dats)
    assert lib0.ngrid == vec.shape[1]
    filled = make_nd.regular_library(regularize_grid.regularize(S, **opts))
    assert filled['idgrid'].shape == (4, 4, 5, 4) and (filled['idgrid'] >= 0).all()
    lib = TemplateLibrary.from_models(
        'gold_b', lam_hr, rows, vec, setup, regularize=opts,
        ccf=dict(ccfconf=conf, every=10, vsinis=[0., 100.]))
    assert lib.kind == 'regulargrid' and lib.ccf is not None
    assert torch.equal(lib.dats, TemplateLibrary('gold_b', filled).dats)
    root = 'regularized://'
    spec_inter.register_library(lib, root)
    cfg = dict(GOLD_CONFIG, template_lib=root)
    lam = dict(np.load(os.path.join(GOLD, 'cases.npz')))['c0/gold_b/lam']
    for seed in (1, 2, 3):
        rng = np.random.RandomState(seed)
        v0 = rng.normal(0, 100)
        spec, espec = synth.fake_observation(lam, 4900., 2.1, -0.7, 0.2, v0, 100., rng,
                                             wresol=4700. / 2000 / 2.35)
        sd = [spec_fit.SpecData('gold_b', lam, spec, espec)]
        r = fitter_ccf.fit(sd, cfg)
        assert abs(r['best_vel'] - v0) < 10, (seed, r['best_vel'], v0)
        res = vel_fit.process(sd, dict(logg=2, teff=5000, feh=-0.5, alpha=0.2,
                                       vsini=0.1), fixParam=[], config=cfg,
                              options=dict(npoly=15))
        print('seed %d: v0 %.2f ccf %.2f process %.2f +- %.2f'
              % (seed, v0, r['best_vel'], res['vel'], res['vel_err']))
        assert abs(res['vel'] - v0) < max(10, 3 * res['vel_err']), \
            (seed, res['vel'], v0, res['vel_err'])
