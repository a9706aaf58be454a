"""The yardstick of the vsini derivative, pinned on the CPU before any kernel is held
against it: the taps w(R) and dw/dR of tests/vsini_grad_truth.py against the oracle's
compute_vsini_kernel and its Richardson central difference, the truth's d chi^2 /
d vsini against a Richardson central difference of the truth's value, and the
declaration of rvs_vsini_convolve_grad against its binding."""
import os
import re

import numpy as np
import pytest

from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import vsini_grad_truth as vtruth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# below, at, between and far above the integers at which the tap count changes
R_VALUES = [0.05, 0.3, 0.999, 1.0, 1.7, 2.0, 2.5, 7.3, 31.4]


def _centred(x, n):
    return np.pad(x, (n - len(x)) // 2)


@pytest.mark.parametrize('R', R_VALUES)
def test_taps_are_the_oracles(R):
    w, dw = vtruth.taps(R)
    ref = orc.compute_vsini_kernel(R)
    assert len(w) == len(ref) == len(dw)
    err = np.abs(w - ref).max()
    print('R %g taps %d max |w - oracle| %.3g' % (R, len(w), err))
    assert err <= 1e-14
    assert abs(w.sum() - 1) <= 1e-14 and abs(dw.sum()) <= 1e-14


@pytest.mark.parametrize('R', R_VALUES)
def test_tap_derivative_is_the_oracles_central_difference(R):
    """D(h) = (w(R+h) - w(R-h)) / 2h of the oracle's kernel, h = 1e-5 max(R, 1), and
    the Richardson combination (4 D(h/2) - D(h)) / 3.  Measured: 3.2e-10 absolute at
    R = 1.0 and 2.0 (the third derivative has a kink at an integer R, so the h^2 term
    does not cancel there), <= 3e-11 elsewhere, on taps of 0.0025-0.4.  The bound is
    15 x the largest, the margin for another libm."""
    w, dw = vtruth.taps(R)
    d = []
    for h in (1e-5 * max(R, 1.0), 0.5e-5 * max(R, 1.0)):
        a, b = orc.compute_vsini_kernel(R + h), orc.compute_vsini_kernel(R - h)
        n = max(len(a), len(b), len(w))
        d.append((_centred(a, n) - _centred(b, n)) / (2 * h))
    rich = (4 * d[1] - d[0]) / 3
    err = np.abs(_centred(dw, len(rich)) - rich).max()
    print('R %g max |dw/dR| %.4g max error %.3g' % (R, np.abs(dw).max(), err))
    assert err <= 5e-9


def test_truth_vsini_component_is_its_central_difference(cases, gold_libs):
    """the broadened job of truth.JOBS: value and first 1 + ndim components are those
    of truth.chisq_and_grad (whose taps are the oracle's); the vsini component against
    the Richardson central difference of that value in vsini, steps 0.2 and 0.1 km/s
    (the velocity's: a pixel is ~25 km/s, R stays inside (1, 2)), with the tolerance
    of test_chisq_grad_cpu.py: 1e-6 of the component + the value's rounding
    (1e-13 |f| + 1e-10) / (h/2) * 5/3"""
    npoly = 10
    s, vel, par, vs = truth.JOBS[3]
    sds = truth.spectra(cases, orc.SpecData)[s]
    val, g = vtruth.chisq_and_grad_vsini(sds, gold_libs, vel, par, vs, npoly=npoly)
    val0, g0 = truth.truth_jobs(cases, gold_libs, npoly)[3]
    assert abs(val - val0) <= 1e-12 * abs(val0)
    assert np.abs(g[:5] - g0).max() <= 1e-12 * np.abs(g0).max()
    h0 = 0.2
    d = []
    for h in (h0, h0 / 2):
        f = [truth.chisq_and_grad(sds, gold_libs, vel, par, vs + e, npoly=npoly)[0]
             for e in (h, -h)]
        d.append((f[0] - f[1]) / (2 * h))
    rich = (4 * d[1] - d[0]) / 3
    noise = (1e-13 * abs(val) + 1e-10) / (h0 / 2) * 5 / 3
    print('d/dvsini truth %.12g richardson %.12g diff %.3g bound %.3g'
          % (g[5], rich, g[5] - rich, 1e-6 * abs(g[5]) + noise))
    assert abs(g[5] - rich) <= 1e-6 * abs(g[5]) + noise
    # the clamp: an unbroadened template does not depend on vsini
    _, gz = vtruth.chisq_and_grad_vsini(sds, gold_libs, vel, par, 0.0, npoly=npoly)
    assert gz[5] == 0.0


def test_header_and_binding_agree():
    """rvs_vsini_convolve_grad is declared in include/rvsgpu.h with the arguments the
    ctypes table gives it, exported, and refuses bad shapes before any launch; the
    ABI number did not move"""
    import ctypes
    from rvspecfit_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
    assert _lib.ABI_VERSION == 18
    txt = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    m = re.search(r'\bint\s+rvs_vsini_convolve_grad\s*\(([^;]*?)\)\s*;', txt, flags=re.S)
    assert m, 'rvs_vsini_convolve_grad is not declared'
    kinds = []
    for a in m.group(1).split(','):
        a = ' '.join(a.split())
        kinds.append(ctypes.c_void_p if '*' in a else
                     {'int': ctypes.c_int, 'double': ctypes.c_double}[a.split()[0]])
    res, args = _lib.SIGNATURES['rvs_vsini_convolve_grad']
    assert res is ctypes.c_int and args == kinds
    assert [a.split()[-1].lstrip('*') for a in m.group(1).split(',')] == \
        ['templ', 'vsini', 'outside', 'lnstep', 'eps', 'ntp', 'R', 'B', 'out', 'stream']
    L = _lib.lib()
    assert L.rvs_abi_version() == 18
    f = L.rvs_vsini_convolve_grad
    a, b = ctypes.c_void_p(64), ctypes.c_void_p(128)    # never dereferenced
    assert f(a, a, None, 1e-4, 0.6, 10, 0, 1, b, None) == -1     # R < 1
    assert f(a, a, None, 1e-4, 0.6, 10, 1, 0, b, None) == -1     # B < 1
    assert f(a, a, None, 1e-4, 0.6, 0, 1, 1, b, None) == -1      # ntp < 1
    assert f(a, a, None, 1e-4, 0.6, 10, 1, 1, a, None) == -1     # out == templ
    assert f(a, a, None, 0.0, 0.6, 10, 1, 1, b, None) == -1      # lnstep <= 0
