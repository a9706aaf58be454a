"""The yardstick of the analytic gradient under resolution matrices, pinned on the CPU
before any kernel is held against it (tests/chisq_grad_resol_truth.py against the
oracle's get_chisq with resol_params), the four new entry points against their
declarations, and the scope check with and without config['resol_gradient'].

Observed on the CPU, jobs 0 ... 4 with matrices of 9 ... 25 diagonals: the truth's value
is within 2.1e-13 (relative) of the oracle's at npoly 5 / 10 / 16, its velocity
derivative within 6.3e-8 of the Richardson central difference."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import chisq_grad_resol_truth as rtruth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JOBS = list(range(5))


def _oracle(cases, gold_libs, gold_config, job, npoly):
    s, vel, par, vs = truth.JOBS[job]
    sds = truth.spectra(cases, orc.SpecData)[s]
    mats = rtruth.matrices(sds, job)
    rp = {sd.name: R for sd, R in zip(sds, mats)}

    def f(v):
        return orc.get_chisq(sds, float(v), tuple(par), None if vs is None else (vs, ),
                             options=dict(npoly=npoly), config=gold_config,
                             libs=gold_libs, resol_params=rp)
    return sds, mats, f


def test_the_bands_cross_the_block_stride(cases):
    """9 ... 25 diagonals on arms of 401 and 301 pixels: wider than one pixel, narrower
    than a tile, and on both sides of pixel 256"""
    nds = []
    for job in JOBS:
        sds = truth.spectra(cases, orc.SpecData)[truth.JOBS[job][0]]
        assert [len(sd.lam) for sd in sds] == [401, 301]
        nds += [rtruth.ndiag(R) for R in rtruth.matrices(sds, job)]
    print('diagonals', nds)
    assert min(nds) == 9 and max(nds) == 25


@pytest.mark.parametrize('npoly', [5, 10, 16])
def test_truth_value_is_the_oracles(cases, gold_libs, gold_config, npoly):
    """the bound of test_chisq_grad_gpu.py::test_values_are_chisq_points"""
    for job in JOBS:
        s, vel, par, vs = truth.JOBS[job]
        sds, mats, f = _oracle(cases, gold_libs, gold_config, job, npoly)
        val, _ = rtruth.chisq_and_grad(sds, gold_libs, mats, vel, par, vs, npoly=npoly)
        ref = f(vel)
        print('npoly %d job %d truth %.15g oracle %.15g relative difference %.3g'
              % (npoly, job, val, ref, abs(val - ref) / abs(ref)))
        assert abs(val - ref) <= 1e-11 * max(abs(ref), 1e3), (job, val, ref)


@pytest.mark.parametrize('job', JOBS)
def test_truth_velocity_derivative_is_the_oracles_central_difference(
        cases, gold_libs, gold_config, job):
    """Richardson's combination of the central differences at h = 0.5 and 0.25 km/s of
    the oracle's value (test_chisq_grad_cpu.py), bound 1e-6 relative"""
    npoly = 10
    s, vel, par, vs = truth.JOBS[job]
    sds, mats, f = _oracle(cases, gold_libs, gold_config, job, npoly)
    _, g = rtruth.chisq_and_grad(sds, gold_libs, mats, vel, par, vs, npoly=npoly)
    d = [(f(vel + h) - f(vel - h)) / (2 * h) for h in (0.5, 0.25)]
    rich = (4 * d[1] - d[0]) / 3
    print('job %d truth %.12g richardson %.12g relative difference %.3g'
          % (job, g[0], rich, abs(g[0] - rich) / abs(rich)))
    assert abs(g[0] - rich) <= 1e-6 * abs(rich), (job, g[0], rich)


def test_header_and_binding_agree():
    """the four new names are declared in include/rvsgpu.h with the argument lists of
    the pair without _resol, carry the kinds the ctypes table gives them, are exported,
    and refuse before any launch (fake pointers, never dereferenced) what the header
    lists; the pair without _resol goes on refusing taps; the ABI number did not move"""
    from rvspecfit_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
    lds_max = int(eval(re.search(r'#define RVS_GRAD_RESOL_LDS_MAX \(([^)]*)\)',
                                 hdr).group(1)))
    txt = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    decl = {}
    for base in ('rvs_chisq_point_grad', 'rvs_chisq_point_fisher'):
        for name in (base, base + '_work_size', base + '_resol',
                     base + '_resol_work_size'):
            m = re.search(r'\bint(?:64_t)?\s+%s\s*\(([^;]*?)\)\s*;' % name, txt,
                          flags=re.S)
            assert m, name + ' is not declared'
            decl[name] = [' '.join(a.split()) for a in m.group(1).split(',')]
        assert decl[base + '_resol'] == decl[base]
        assert decl[base + '_resol_work_size'] == decl[base + '_work_size']
        assert _lib.SIGNATURES[base + '_resol'] == _lib.SIGNATURES[base]
        assert _lib.SIGNATURES[base + '_resol_work_size'] == \
            _lib.SIGNATURES[base + '_work_size']
    L = _lib.lib()
    assert L.rvs_abi_version() == 18
    for J, narm, ntan in ((1, 1, 0), (7, 2, 4), (8192, 3, 6), (0, 1, 4), (1, 0, 4),
                          (1, 1, 7), (1, 1, -1)):
        assert L.rvs_chisq_point_grad_resol_work_size(J, narm, ntan) == \
            L.rvs_chisq_point_grad_work_size(J, narm, ntan)
        assert L.rvs_chisq_point_fisher_resol_work_size(J, narm, ntan) == \
            L.rvs_chisq_point_fisher_work_size(J, narm, ntan)

    def arm(**kw):
        p = _lib.PointArm()
        p.npix, p.ntp, p.S, p.G = 100, 10, 1, 1
        p.taps, p.nd = 64, 11
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    a = ctypes.c_void_p(64)     # never dereferenced

    def grad(p, npoly, ntan, resol='_resol'):
        f = getattr(L, 'rvs_chisq_point_grad' + resol)
        return f(ctypes.addressof(p), 1, npoly, ntan, None, None, 1, a, 1.0, None, a, a,
                 a, a, None)

    def fisher(p, npoly, ntan, resol='_resol', F=a):
        f = getattr(L, 'rvs_chisq_point_fisher' + resol)
        return f(ctypes.addressof(p), 1, npoly, ntan, None, None, 1, a, 1.0, None, a, a,
                 a, F, a, None)
    for call in (grad, fisher):
        assert call(arm(nd=10), 10, 4) == -1        # even nd
        assert call(arm(nd=0), 10, 4) == -1
        assert call(arm(nd=-3), 10, 4) == -1
        assert call(arm(G=2), 10, 4) == -1          # a grid set
        assert call(arm(fast_interp=1), 10, 4) == -1
        assert call(arm(), 0, 4) == -1              # npoly outside 1 .. 16
        assert call(arm(), 17, 4) == -1
        assert call(arm(), 10, 7) == -1             # ntan outside 0 .. 6
        assert call(arm(), 10, -1) == -1
        # the first band whose tiles do not fit: (2 + ntan) (255 + nd) 8 > the limit
        for ntan in (0, 4, 6):
            nd = lds_max // (8 * (2 + ntan)) - 255
            nd += 1 + nd % 2                        # the next odd number
            assert (2 + ntan) * (255 + nd) * 8 > lds_max >= \
                (2 + ntan) * (255 + nd - 2) * 8
            assert call(arm(nd=nd), 10, ntan) == -1
        # the pair without _resol: any taps
        assert call(arm(), 10, 4, '') == -1
    assert fisher(arm(), 10, 4, F=None) == -1


class _Arm:
    def __init__(self, name, G=1, resol=None):
        self.name, self.G, self.resol = name, G, resol


class _Batch:
    def __init__(self, arms):
        self.arms = arms


class _Lib:
    kind, ndim = 'regulargrid', 4


def test_scope_with_and_without_the_key():
    from rvspecfit_amd import engine
    libs = {'gold_b': _Lib, 'gold_r': _Lib}
    rs = dict(taps=None, nd=11, stride=0)
    own = _Batch([_Arm('gold_b', resol=rs), _Arm('gold_r')])      # the spectra's own
    plain = _Batch([_Arm('gold_b'), _Arm('gold_r')])
    msg = r'the analytic gradient does not take a resolution matrix \(arm gold_b\)'
    for kw in (dict(), dict(resol_gradient=False), dict(vsini_grad=True)):
        with pytest.raises(ValueError, match=msg):
            engine.check_grad_scope(own, libs, 10, **kw)
        with pytest.raises(ValueError, match=msg):                 # resol_params
            engine.check_grad_scope(plain, libs, 10, [rs, None], **kw)
    engine.check_grad_scope(own, libs, 10, resol_gradient=True)
    engine.check_grad_scope(plain, libs, 10, [None, rs], resol_gradient=True)
    engine.check_grad_scope(plain, libs, 10, [rs, rs], vsini_grad=True,
                            resol_gradient=True)
    # both together raise as the value does
    with pytest.raises(ValueError, match='not allowed to set resol_param'):
        engine.check_grad_scope(own, libs, 10, [rs, None], resol_gradient=True)
    # what stays refused with the key
    grids = _Batch([_Arm('gold_b', G=2), _Arm('gold_r')])
    for kw in (dict(), dict(resol_gradient=True)):
        with pytest.raises(ValueError, match='grid set'):
            engine.check_grad_scope(grids, libs, 10, **kw)
    with pytest.raises(ValueError, match='fast_interp'):
        engine.check_grad_scope(own, libs, 10, fast_interp=True, resol_gradient=True)
    with pytest.raises(ValueError, match='npoly <= 16'):
        engine.check_grad_scope(own, libs, 17, resol_gradient=True)
    # the LDS limit by name
    engine.check_grad_resol_lds(6, 641)
    with pytest.raises(ValueError, match=r'limit is %d \(nd <= 641\)'
                       % engine.GRAD_RESOL_LDS_MAX):
        engine.check_grad_resol_lds(6, 643)
