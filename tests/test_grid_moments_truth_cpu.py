"""The exact reference of the grid summary (tests/grid_moments_truth.py) pinned without
a GPU: over every group of every launch that tests/test_grid_moments_gpu.py makes, the
project's float64 numpy restatement (oracle.rvs_oracle.grid_summary) lies inside the
a-priori bounds, the argmin is numpy's, the "reference would have asserted" flag is the
restatement's own exception, and a result that is wrong by 1e-12 lies outside.

The worst |restatement - truth| / bound per quantity is printed (run with -s) and
recorded in the docstring of grid_moments_truth.py; nothing here asserts it."""
import warnings

import numpy as np
import pytest

import grid_moments_truth as gt
from oracle import rvs_oracle as orc

FAMILIES = ['plain', 'ends', 'nvel', 'ties', 'parabola', 'moments', 'nan', 'empty']
WORST = {}


def _note(key, r):
    WORST[key] = max(WORST.get(key, 0.0), r)


def _oracle(v, c, quadratic):
    """grid_summary on the reference's [nv, Np] layout, or None where it raises"""
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        try:
            return orc.grid_summary(v, np.ascontiguousarray(c.T), bool(quadratic))
        except (AssertionError, np.linalg.LinAlgError, ValueError):
            return None


def _polyfit_conditioning(x):
    """condition number of the column-scaled Vandermonde matrix np.polyfit solves"""
    V = np.vander(x, 3)
    return float(np.linalg.cond(V / np.sqrt((V * V).sum(axis=0))))


@pytest.mark.parametrize('family', FAMILIES)
def test_restatement_inside_the_bounds(family):
    for L in gt.by_family(family):
        for g in range(L['G']):
            v, c = gt.group_inputs(L, g)
            t = gt.group_truth(L, g)
            what = (L['name'], g)
            if t['empty']:
                assert t['i1'] == t['i2'] == -1 and t['best_chi'] == np.inf
                continue
            # numpy's own argmin, NaN rule included
            i1, i2 = np.unravel_index(np.argmin(c.T), c.T.shape)
            assert (t['i1'], t['i2']) == (int(i1), int(i2)), what
            q = L['quadratic']
            s = _oracle(v, c, q)
            assert (s is None) == t['asserts'], what
            interior = bool(q) and 0 < t['i1'] < len(v) - 1
            if s is None:
                # what does not depend on best_vel still compares
                s, ta, moments = _oracle(v, c, 0), t, False
            elif interior:
                # the restatement's vertex is np.polyfit's: its moments are held to
                # the truth about ITS best_vel, the vertex itself only recorded
                ta = gt.truth(v, c, q, about=s['best_vel'])
                r = gt.ratio(s['best_vel'], t['best_vel'], t['bound']['best_vel'])
                _note('polyfit_vertex', r)
                x = v[t['i1'] - 1:t['i1'] + 2]
                # and against the conditioning of polyfit's own solve, on the scale
                # of the bracket: recorded, like the ratio above
                _note('polyfit_vertex_cond', abs(float(t['best_vel']) - s['best_vel'])
                      / (_polyfit_conditioning(x) * gt.U * (x[2] - x[0])))
                assert x[0] < s['best_vel'] < x[2], what
                moments = True
            else:
                assert s['best_vel'] == float(t['best_vel']) == v[t['i1']], what
                ta, moments = t, True
            assert s['i2'] == t['i2'], what
            if np.isnan(t['best_chi']):
                assert np.isnan(s['best_chi']) and np.all(np.isnan(s['probs'])), what
            else:
                assert s['best_chi'] == t['best_chi'], what
            _note('best_chi', 0.0)
            for i in range(len(v)):
                r = gt.ratio(s['probs'][i], t['probs'][i], t['bound']['probs'][i])
                _note('probs', r)
                assert r <= 1, what + (i, )
            if moments:
                for k in ('vel_err', 'kurtosis', 'skewness'):
                    r = gt.ratio(s[k], ta[k], ta['bound'][k])
                    _note(k, r)
                    assert r <= 1, what + (k, float(s[k]), float(ta[k]),
                                           ta['bound'][k])
            assert not t['switch_ambiguous'], what
    print('grid-moments restatement/bound', family,
          ' '.join('%s %.3g' % kv for kv in sorted(WORST.items())))


def test_every_shape_of_the_issue_is_in_the_list():
    Ls = gt.launches()
    assert set(L['Nv'] for L in Ls if L['family'] == 'plain') == set(gt.NVS)
    assert set(L['Np'] for L in Ls if L['family'] == 'plain') == set(gt.NPS)
    sizes = set()
    for L in Ls:
        for g in range(L['G']):
            v, c = gt.group_inputs(L, g)
            sizes.add(c.size)
    assert any(0 < s < 64 for s in sizes) and any(64 <= s < 256 for s in sizes)
    assert any(L['vels'].ndim == 1 for L in Ls) and any(L['vels'].ndim == 2 for L in Ls)


def test_families_contain_what_they_name():
    """the edits of each family did what the family is for (judged by the truth)"""
    for L in gt.by_family('plain'):
        if L['Nv'] >= 3:
            for g in range(L['G']):
                assert 0 < gt.group_truth(L, g)['i1'] < L['Nv'] - 1, L['name']
    for L in gt.by_family('ends'):
        for g in range(L['G']):
            t = gt.group_truth(L, g)
            assert t['i1'] == L['want_i1'][g] and not t['asserts']
            assert float(t['best_vel']) == gt.group_inputs(L, g)[0][t['i1']]
        nv = int(L['nvel'][2])       # the padded entry is below the minimum
        assert L['chisq'][2][:, nv].min() < gt.group_truth(L, 2)['best_chi']
    for L in gt.by_family('ties'):
        for g in range(L['G']):
            t = gt.group_truth(L, g)
            assert (t['i1'], t['i2']) == L['want_i'][g], (L['name'], g)
            assert (L['chisq'][g] == t['best_chi']).sum() == 2
    for L in gt.by_family('parabola'):
        for g, kind in enumerate(L['kinds']):
            t = gt.group_truth(L, g)
            assert t['asserts'] == kind.startswith('inf'), (L['name'], kind)
            if kind == 'plateau2':
                v = gt.group_inputs(L, g)[0]
                mid = (gt.mpf(v[t['i1']]) + gt.mpf(v[t['i1'] + 1])) / 2
                assert t['best_vel'] == mid
    for L in gt.by_family('moments'):
        for g, kind in enumerate(L['kinds']):
            t = gt.group_truth(L, g)
            p = np.array([float(_) for _ in t['probs']])
            if kind.startswith('symmetric'):
                assert t['bound']['skewness'] < 1e-12
                assert abs(t['skewness']) <= t['bound']['skewness']
            elif kind == 'sharp':
                assert t['vel_err'] < 1e-10 and t['kurtosis'] == 0 == t['skewness']
            elif kind == 'span1.5e3':
                assert np.any((p > 0) & (p < 2.0**-1022)) and np.any(p == 0)
                assert np.any((t['bound']['probs'] > 0) & (p == 0))
            elif kind == 'span1e6':
                assert (p == 0).sum() >= L['Nv'] // 2
            elif kind == 'constant':
                assert np.all(p == 1. / L['Nv']) or L['Nv'] & (L['Nv'] - 1)
                assert (t['i1'], t['i2']) == (0, 0)
            elif kind == 'inf_away':
                assert (p == 0).sum() >= 4 and t['bound']['probs'][0] == 0
    for L in gt.by_family('nan'):
        for g in range(L['G']):
            assert np.isnan(gt.group_truth(L, g)['best_chi']) == (g not in L['clean'])
    for L in gt.by_family('empty'):
        assert (L['nvel'] == 0).sum() >= 3


def test_the_bounds_bite():
    """a probability wrong by a relative 1e-12, or a third moment wrong by 1e-12 of
    sum |t_i|, lies outside"""
    for name, g in (('plain-65x1-shared-q0', 1), ('moments-65x1-q1', 0),
                    ('plain-257x3-pergroup-q1', 1), ('plain-4097x1-shared-q0', 0)):
        L = gt.by_name(name)
        v, c = gt.group_inputs(L, g)
        t = gt.group_truth(L, g)
        s = _oracle(v, c, 0)
        i = t['i1']
        assert gt.ratio(s['probs'][i], t['probs'][i], t['bound']['probs'][i]) <= 1
        assert gt.ratio(s['probs'][i] * (1 + 1e-12), t['probs'][i],
                        t['bound']['probs'][i]) > 1
        ta = gt.truth(v, c, 0)
        m3 = float(np.sum(s['probs'] * (v - v[ta['i1']])**3))
        assert gt.ratio(m3, ta['m3'], ta['bound']['m3']) <= 1
        assert gt.ratio(m3 + 1e-12 * float(ta['abs3']), ta['m3'],
                        ta['bound']['m3']) > 1


def test_truth_against_closed_forms():
    """two points of equal chi^2 one apart: probs 1/2, vel_err about the first = sqrt
    (1/2), skewness sqrt 2, kurtosis 2; three points on an exact parabola: its vertex"""
    t = gt.truth(np.array([0., 1.]), np.array([[7., 7.]]), True)
    assert (t['i1'], t['i2']) == (0, 0) and t['best_vel'] == 0
    assert t['probs'] == [gt.mpf(0.5)] * 2 and t['psum'] == 2
    assert abs(t['vel_err']**2 - gt.mpf(0.5)) < 1e-50
    assert abs(t['kurtosis'] - 2) < 1e-50 and abs(t['skewness']**2 - 2) < 1e-50
    x = np.array([1., 2., 4.])
    y = 3. * (x - 2.25)**2 + 1.          # exact in float64
    t = gt.truth(x, y[None, :], True)
    assert t['i1'] == 1 and t['best_vel'] == gt.mpf(2.25) and not t['asserts']
    assert 0 < t['bound']['best_vel'] < 1e-14
