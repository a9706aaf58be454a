"""What of regularize_grid can be checked without a device: the argument checks of the
rvs_rbf_* entry points, the truth of tests/rbf_truth.py against scipy and the golden
rows, and the bookkeeping of regularize_grid.plan (windows, overlaps, axes, row order)
against the reference's converter (tests/golden/regularize_cases.npz) with scipy doing
the numbers."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rbf_truth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')


def _scipy(y, d, x, smooth):
    import scipy.interpolate
    return scipy.interpolate.RBFInterpolator(y, d, smoothing=smooth,
                                             kernel='multiquadric', epsilon=1)(x)


def test_argument_checks_without_a_device():
    from rvspecfit_amd import _lib
    L = _lib.lib()
    one = np.ones(64)
    p = one.ctypes.data
    assert _lib.ABI_VERSION >= 17 and _lib.ST_RBF_NOTPD == 0x400
    assert L.rvs_rbf_work_size(100, 10) == 8 + 128 * 128 + 128 * 16 + 16
    assert L.rvs_rbf_work_size(0, 10) == -1
    assert L.rvs_rbf_work_size(16385, 10) == -1
    assert L.rvs_rbf_work_size(100, 0) == -1
    assert L.rvs_rbf_factor(None, 10, 4, 1., None, p, p, None) == -1
    assert L.rvs_rbf_factor(p, 0, 4, 1., None, p, p, None) == -1
    assert L.rvs_rbf_factor(p, 16385, 4, 1., None, p, p, None) == -1
    assert L.rvs_rbf_factor(p, 10, 9, 1., None, p, p, None) == -1
    assert L.rvs_rbf_factor(p, 10, 0, 1., None, p, p, None) == -1
    assert L.rvs_rbf_factor(p, 10, 4, 0., None, p, p, None) == -1
    assert L.rvs_rbf_factor(p, 10, 4, float('nan'), None, p, p, None) == -1
    assert L.rvs_rbf_factor(p, 10, 4, 1., None, p, None, None) == -1
    assert L.rvs_rbf_solve(None, 0, 4, 10, 4, p, p, None) == -1
    assert L.rvs_rbf_solve(p, 0, 3, 10, 4, p, p, None) == -1       # stride < S
    assert L.rvs_rbf_solve(p, 0, 4, 10, 0, p, p, None) == -1
    assert L.rvs_rbf_eval(p, 0, p, 10, 4, 1., p, 4, 64, p, 4, None) == -1
    assert L.rvs_rbf_eval(p, 5, p, 10, 4, 1., p, 4, 16, p, 4, None) == -1
    assert L.rvs_rbf_eval(p, 5, p, 10, 4, 1., p, 4, 64, p, 3, None) == -1
    assert L.rvs_rbf_eval(p, 5, p, 10, 9, 1., p, 4, 64, p, 4, None) == -1
    assert L.rvs_rbf_eval(p, 5, None, 10, 4, 1., p, 4, 64, p, 4, None) == -1


def test_interpolator_takes_the_reference_subset_only():
    from rvspecfit_amd import rbf
    y, d = np.zeros((5, 2)), np.zeros(5)
    for kw in (dict(kernel='thin_plate_spline'), dict(neighbors=3), dict(degree=1),
               dict(epsilon=0.)):
        with pytest.raises(ValueError):
            rbf.RBFInterpolator(y, d, **kw)


def test_truth_against_scipy():
    """the refined long-double solution interpolates the nodes to rounding, its
    refinement converges in a few steps, and scipy sits within the error its condition
    number allows (1e-10 on values of order 1 .. 10)"""
    rng = np.random.default_rng(3)
    y = rng.random((150, 4)) * 5
    d = rng.standard_normal((150, 3))
    c, lam, steps = rbf_truth.solve(y, d)
    assert 1 <= len(steps) <= 6 and steps[-1] < 1e-13
    assert float(np.abs(c.sum(axis=0)).max()) < 1e-12
    back = rbf_truth.evaluate(y, y, c, lam)
    assert float(np.abs(back - d).max()) < 1e-15
    x = rng.random((40, 4)) * 5
    e = np.abs(_scipy(y, d, x, 0.) - rbf_truth.interpolate(y, d, x)).max()
    print('scipy against the truth: %.3e' % e)
    assert e < 1e-10


@pytest.mark.parametrize('name', list(rbf_truth.CASES))
def test_plan_and_scipy_against_the_reference(name):
    """plan's windows, points and row order are converter's: vec equal to the last bit,
    and scipy on plan's nodes gives the golden rows; these lie as close to the truth as
    the issue's trial found (a few 1e-12 at most)"""
    from rvspecfit_amd import regularize_grid
    g = np.load(os.path.join(GOLD, 'regularize_cases.npz'))
    D, opts = rbf_truth.case_inputs(name)
    assert D['vec'].shape[1] == int(g[name + '/nrows_in'])
    smooth = opts.pop('smooth')
    ymap, wins = regularize_grid.plan(D['vec'], **opts)
    nteff = len(np.unique(D['vec'][0]))
    assert len(wins) == max(1, nteff - 12)
    vec = np.concatenate([w[1] for w in wins], axis=1)
    assert np.array_equal(vec, g[name + '/vec'])
    assert len(set(map(tuple, vec.T))) == vec.shape[1]          # no duplicates
    newfeh = np.arange(opts['min_feh'], opts['max_feh'] + opts['step_feh'] / 2,
                       opts['step_feh'])
    assert np.array_equal(np.unique(vec[2]), newfeh)
    foot = set(zip(D['vec'][0], D['vec'][1]))
    assert set(zip(vec[0], vec[1])) == foot
    done = 0
    for k, (rows, pts, mapped) in enumerate(wins):
        ids = np.searchsorted(np.unique(D['vec'][0]), D['vec'][0][rows])
        assert ids.min() == k and ids.max() == k + 12 or len(wins) == 1
        m = pts.shape[1]
        got = _scipy(ymap[rows], D['specs'][rows], mapped, smooth)
        want = g[name + '/specs'][done:done + m]
        assert np.abs(got - want).max() < 1e-11
        if k == 0:
            e = np.abs(want - rbf_truth.interpolate(ymap[rows], D['specs'][rows], mapped,
                                                    smooth)).max()
            print('%s window 0: reference against the truth %.3e' % (name, e))
            assert e < 1e-10
        done += m
    assert done == vec.shape[1]


def test_findbestoverlaps_and_holes():
    from rvspecfit_amd import regularize_grid
    iv = [(i, i + 10) for i in range(7)]
    assert list(regularize_grid.findbestoverlaps(np.array([8, 0, 16, 5]), iv)) == \
        [3, 0, 6, 0]
    x, y = [_.ravel() for _ in np.meshgrid(np.arange(5.), np.arange(4.), indexing='ij')]
    regularize_grid.check_holes_2d(x, y)
    corner = ~((x == 4) & (y == 0))
    regularize_grid.check_holes_2d(x[corner], y[corner])
    inner = ~((x == 2) & (y == 1))
    with pytest.raises(Exception, match='holes'):
        regularize_grid.check_holes_2d(x[inner], y[inner])


def test_command_line_options():
    from rvspecfit_amd import make_interpol
    base = ['--setup', 's', '--lambda0', '1', '--lambda1', '2', '--step', '1',
            '--templprefix', 'p', '--wavefile', 'w', '--resol', '1000']
    a = make_interpol.make_parser().parse_args(base)
    assert a.regularize is False
    assert (a.min_feh, a.max_feh, a.step_feh, a.min_alpha, a.max_alpha, a.step_alpha,
            a.smooth) == (-4, 1.2, .25, -.4, 1.2, .2, 0.)
    a = make_interpol.make_parser().parse_args(base + ['--regularize', '--smooth', '0.1',
                                                       '--step_feh', '0.5'])
    assert a.regularize is True and a.smooth == 0.1 and a.step_feh == 0.5
