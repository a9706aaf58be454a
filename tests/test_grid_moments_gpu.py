"""rvs_grid_moments (grid_moments_kernel, csrc/chisq.hip) through the C ABI against the
exact reference of tests/grid_moments_truth.py, which tests/
test_grid_moments_truth_cpu.py pins without a GPU.  One launch per entry of
grid_moments_truth.launches(), many groups per launch; every group of every launch is
held to the truth of that group alone: i1, i2 and best_chi exactly, best_vel, vel_err,
kurtosis, skewness, res[7] and every probability inside the truth's a-priori float64
bounds, probs past nvel[g] exactly 0, status[g] = RVS_ST_QUAD_ASSERT exactly where the
reference would have raised.  res, probs and status lie inside sentinel-filled margins
that must come back untouched.  What a family adds to that is in its test.

A flat triple (three equal minima in one template) cannot reach the 0/0 of the vertex
formula: the argmin takes the first of the three, whose left neighbour is strictly
greater, so the triple the parabola sees is a two-point plateau and the reference
does not raise.  The case is here and held to that."""
import math

import numpy as np
import pytest
import torch

import grid_moments_truth as gt

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 64
SENT = -12345.678
SENT_I = -1234567
WORST = {}


def _lib_():
    from rvspecfit_amd import _lib
    _lib.require_gpu()
    return _lib, _lib.lib()


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD, ), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, fill, what):
    g = torch.full((GUARD, ), fill, dtype=buf.dtype, device=DEV)
    assert torch.equal(buf[:GUARD], g), 'write in front of ' + what
    assert torch.equal(buf[-GUARD:], g), 'write behind ' + what


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


_device_inputs = {}


def _inputs(L):
    if L['name'] not in _device_inputs:
        _device_inputs[L['name']] = (
            _dev(L['chisq']), _dev(L['vels']),
            None if L['nvel'] is None else _dev(L['nvel']))
    return _device_inputs[L['name']]


def run(L, group=None, want_probs=True, want_status=True):
    """one rvs_grid_moments on launch L (or on its group `group` alone) ->
    res [G, 8], probs [G, Nv] or None, status [G] or None (numpy)"""
    _lib, lib = _lib_()
    chisq, vels, nvel = _inputs(L)
    G, Np, Nv = L['G'], L['Np'], L['Nv']
    stride = 0 if vels.dim() == 1 else Nv
    if group is not None:
        chisq = chisq[group:group + 1]
        vels = vels if stride == 0 else vels[group]
        nvel = None if nvel is None else nvel[group:group + 1]
        G = 1
    rbuf, res = _guarded(G * 8, torch.float64, SENT)
    pbuf, probs = _guarded(G * Nv, torch.float64, SENT)
    sbuf, status = _guarded(G, torch.int32, SENT_I)
    status.zero_()
    rc = lib.rvs_grid_moments(_lib.ptr(chisq), _lib.ptr(vels), stride, _lib.ptr(nvel),
                              G, Np, Nv, L['quadratic'], _lib.ptr(res),
                              _lib.ptr(probs) if want_probs else None,
                              _lib.ptr(status) if want_status else None,
                              _lib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    _intact(rbuf, SENT, 'res')
    _intact(pbuf, SENT, 'probs')
    _intact(sbuf, SENT_I, 'status')
    if not want_probs:
        assert torch.all(probs == SENT)
    if not want_status:
        assert torch.all(status == 0)
    return (res.view(G, 8).cpu().numpy(),
            probs.view(G, Nv).cpu().numpy() if want_probs else None,
            status.cpu().numpy() if want_status else None)


_results = {}


def result(L):
    """the full launch, once per session"""
    if L['name'] not in _results:
        _results[L['name']] = run(L)
    return _results[L['name']]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _hold(key, got, want, bound, what):
    r = gt.ratio(got, want, bound)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1, what + (key, float(got), float(want), bound, r)


def check_group(L, g, res, probs, status):
    """group g of launch L against the truth of that group"""
    from rvspecfit_amd import _lib
    t = gt.group_truth(L, g)
    v, c = gt.group_inputs(L, g)
    nv, what = len(v), (L['name'], g)
    r = res[g]
    assert (int(r[5]), int(r[6])) == (t['i1'], t['i2']) and r[5] == t['i1'] and \
        r[6] == t['i2'], what + (r[5], r[6], t['i1'], t['i2'])
    assert _same_bits(r[0], np.float64(t['best_chi'])) or \
        (np.isnan(r[0]) and np.isnan(t['best_chi'])), what + (r[0], t['best_chi'])
    assert np.all(probs[g, nv:] == 0), what
    if t['empty']:
        assert np.all(np.isnan(r[1:5])) and r[7] == 0 and status[g] == 0, what
        return
    if t['bound']['best_vel'] == 0 and not gt._ctx.isnan(t['best_vel']):
        assert _same_bits(r[1], v[t['i1']]), what       # vels[i1], bit for bit
    else:
        _hold('best_vel', r[1], t['best_vel'], t['bound']['best_vel'], what)
    for j, k in ((2, 'vel_err'), (3, 'kurtosis'), (4, 'skewness'), (7, 'psum')):
        _hold(k, r[j], t[k], t['bound'][k], what)
    if t['vel_err'] < gt.SWITCH:
        assert r[3] == 0 and r[4] == 0, what
    for i in range(nv):
        _hold('probs', probs[g, i], t['probs'][i], t['bound']['probs'][i], what + (i, ))
    if not np.isnan(t['best_chi']):
        total = math.fsum(probs[g, :nv])
        assert abs(total - 1) <= float(t['bound']['probs'].sum()), what + (total, )
    assert status[g] == (_lib.ST_QUAD_ASSERT if t['asserts'] else 0), what
    assert not t['switch_ambiguous'], what


def check_launch(L):
    res, probs, status = result(L)
    for g in range(L['G']):
        check_group(L, g, res, probs, status)
    return res, probs, status


def _report(family):
    print('grid-moments device/bound %-8s %s' % (
        family, ' '.join('%s %.3g' % kv for kv in sorted(WORST.items()))))


def test_plain():
    """minimum in the interior; uniform and non-uniform grids, per-group (vel_stride =
    Nv) and shared (0), with and without the parabola, at every Nv and Np"""
    for L in gt.by_family('plain'):
        res, _, _ = check_launch(L)
        if not L['quadratic']:
            for g in range(L['G']):
                assert _same_bits(res[g, 1], gt.group_inputs(L, g)[0][int(res[g, 5])])
    _report('plain')


def test_ends():
    """minimum at index 0, at nv - 1 = Nv - 1, and at nv - 1 with a smaller padded
    entry behind it: vels[i1] exactly, the padding not chosen"""
    for L in gt.by_family('ends'):
        res, _, status = check_launch(L)
        for g in range(L['G']):
            v = gt.group_inputs(L, g)[0]
            assert int(res[g, 5]) == L['want_i1'][g] < len(v)
            assert _same_bits(res[g, 1], v[L['want_i1'][g]]) and status[g] == 0
    _report('ends')


def test_nvel_padding_is_never_read():
    """per-group lengths; the padding of chisq NaN (and of vels NaN), -1e300, or the
    last valid value: the three results are bit-identical"""
    for L in gt.by_family('nvel'):
        check_launch(L)
        first = gt.by_name(L['same_as'])
        for a, b in zip(result(L), result(first)):
            assert _same_bits(a, b), (L['name'], first['name'])
    _report('nvel')


def test_ties():
    """equal minima across templates and velocities, in the same thread's stride, in
    different threads and in different waves: the first in velocity-major order"""
    for L in gt.by_family('ties'):
        res, _, _ = check_launch(L)
        for g in range(L['G']):
            assert (int(res[g, 5]), int(res[g, 6])) == L['want_i'][g], (L['name'], g)
    _report('ties')


def test_parabola_edge_cases():
    """two-point plateau and flat triple: the midpoint, no flag; a +inf neighbour:
    RVS_ST_QUAD_ASSERT in that group's status and in no other's, best_chi / i1 / i2
    still exact (check_group); status == NULL: the call succeeds and res is the same"""
    from rvspecfit_amd import _lib
    for L in gt.by_family('parabola'):
        res, probs, status = check_launch(L)
        for g, kind in enumerate(L['kinds']):
            assert status[g] == (_lib.ST_QUAD_ASSERT if kind.startswith('inf') else 0)
            if kind in ('plateau2', 'flat3'):
                v = gt.group_inputs(L, g)[0]
                i1 = int(res[g, 5])
                assert v[i1] < res[g, 1] < v[i1 + 1]
        res2, probs2, _ = run(L, want_status=False)
        assert _same_bits(res, res2) and _same_bits(probs, probs2)
    _report('parabola')


def test_moments():
    """a symmetric posterior (skewness inside a bound of order 1e-13), vel_err < 1e-10
    (kurtosis and skewness exactly 0), chi^2 spans whose exp is subnormal or 0, a
    constant grid, +inf away from the minimum (probs exactly 0)"""
    for L in gt.by_family('moments'):
        res, probs, _ = check_launch(L)
        for g, kind in enumerate(L['kinds']):
            t = gt.group_truth(L, g)
            if kind.startswith('symmetric'):
                assert t['bound']['skewness'] < 1e-12   # and check_group held it
            elif kind == 'sharp':
                assert res[g, 2] < 1e-10 and res[g, 3] == 0 and res[g, 4] == 0
            elif kind == 'span1e6':
                assert (probs[g] == 0).sum() >= L['Nv'] // 2
            elif kind == 'inf_away':
                assert np.all(probs[g][np.isinf(L['chisq'][g, int(res[g, 6])])] == 0)
    _report('moments')


def test_nan():
    """numpy's argmin returns the first NaN: i1, i2 are numpy's, best_chi is NaN, and
    the group's neighbours in the launch are untouched"""
    for L in gt.by_family('nan'):
        res, probs, status = check_launch(L)
        for g in range(L['G']):
            assert np.isnan(res[g, 0]) == (g not in L['clean'])
            if g in L['clean']:
                assert np.all(np.isfinite(res[g])) and np.all(np.isfinite(probs[g]))
                assert status[g] == 0
    _report('nan')


def test_empty_groups():
    """nvel[g] = 0: best_chi = +inf, four NaNs, i1 = i2 = -1, res[7] = 0, probs 0;
    the other groups of the launch as if alone"""
    for L in gt.by_family('empty'):
        res, probs, status = check_launch(L)
        for g in np.nonzero(L['nvel'] == 0)[0]:
            assert res[g, 0] == np.inf and np.all(np.isnan(res[g, 1:5]))
            assert res[g, 5] == -1 and res[g, 6] == -1 and res[g, 7] == 0
            assert np.all(probs[g] == 0) and status[g] == 0
        res2, _, _ = run(L, want_probs=False, want_status=False)
        assert _same_bits(res, res2)
    _report('empty')


def test_groups_are_independent_and_runs_repeat():
    """every group of a launch equals the same group launched alone, bit for bit,
    and a second run of the launch equals the first"""
    for L in gt.launches():
        if L['Nv'] > 600:
            continue
        res, probs, status = result(L)
        for a, b in zip(run(L), (res, probs, status)):
            assert _same_bits(a, b), L['name']
        for g in range(L['G']):
            r1, p1, s1 = run(L, group=g)
            assert _same_bits(r1[0], res[g]) and _same_bits(p1[0], probs[g]) and \
                s1[0] == status[g], (L['name'], g)


def test_arguments():
    """G, Np or Nv below 1: RVS_E_ARG before any launch; probs == NULL leaves res as
    it is with probs"""
    _lib, lib = _lib_()
    E_ARG = -1
    for G, Np, Nv in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1, -3, 5),
                      (2, 2, -1)):
        assert lib.rvs_grid_moments(None, None, 0, None, G, Np, Nv, 1, None, None,
                                    None, None) == E_ARG
    for name in ('plain-65x3-pergroup-q1', 'nvel-70x3-pad-nan', 'nan-300x3'):
        L = gt.by_name(name)
        res2, none, status2 = run(L, want_probs=False)
        assert none is None and _same_bits(res2, result(L)[0])
        assert _same_bits(status2, result(L)[2])


def test_engine_grid_moments_equals_the_direct_call():
    """engine.grid_moments with a 2-D vels and nvel (what the velocity refinement
    passes), and with a 1-D vels (find_best, pipeline)"""
    from rvspecfit_amd import engine
    for name in ('nvel-70x3-pad-last', 'nvel-70x1-pad-low', 'empty-257x3',
                 'plain-257x3-shared-q1', 'plain-65x7-shared-q0'):
        L = gt.by_name(name)
        chisq, vels, nvel = _inputs(L)
        res, probs, status = engine.grid_moments(
            chisq.reshape(L['G'] * L['Np'], L['Nv']), vels, Np=L['Np'], nvel=nvel,
            quadratic=bool(L['quadratic']))
        torch.cuda.synchronize()
        want = result(L)
        for a, b in zip((res, probs, status), want):
            assert _same_bits(a.cpu().numpy(), b), name
