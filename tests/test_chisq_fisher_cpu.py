"""The yardstick of the Fisher matrix, pinned on the CPU before any kernel is held against
it (tests/chisq_fisher_truth.py against autograd's Hessian of the profiled chi^2 at zero
residual), the two new entry points against their declarations, and the host part of
vel_fit.fisher_uncertainties on plain numpy matrices.

Observed on the CPU, the five in-cell jobs at npoly 5 / 10 / 16: |F - H/2|_il is at most
1.2e-14 / 1.9e-14 / 1.7e-14 of sqrt(F_ii F_ll); cond(A) <= 1.73, F_ii / G_ii >= 0.53
(npoly 10: cond(A) <= 1.59, F_ii / G_ii >= 0.73)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import gold_lib_dict
from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import chisq_fisher_truth as ftruth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def olibs():
    return {n: orc.Library(gold_lib_dict(n)) for n in ('gold_b', 'gold_r')}


@pytest.mark.parametrize('npoly', [5, 10, 16])
def test_truth_is_half_the_profiled_hessian_at_zero_residual(cases, olibs, npoly):
    """data := fitted model: the Gauss-Newton matrix is the whole Hessian of 0.5 x the
    profiled chi^2.  Bound 1e-12 of sqrt(F_ii F_ll): two chains of ~4000-term float64
    sums (1e-16 * sqrt(4000) each) and the second derivative through a Cholesky solve
    with cond(A) < 100 stay two decades below it."""
    sp = truth.spectra(cases, orc.SpecData)
    want = ftruth.truth_jobs(cases, olibs, npoly)
    for j in truth.INSIDE:
        s, vel, par, vs = truth.JOBS[j]
        F, G, cond = want[j]
        H = ftruth.profiled_half_hessian(sp[s], olibs, vel, par, vs, npoly=npoly)
        d = np.sqrt(np.diag(F))
        rel = np.abs(F - H) / (d[:, None] * d[None, :])
        print('npoly %d job %d largest |F - H/2| / sqrt(F_ii F_ll) %.3g, cond(A) %.3g, '
              'smallest F_ii / G_ii %.3g' % (npoly, j, rel.max(), cond,
                                             (np.diag(F) / np.diag(G)).min()))
        assert rel.max() <= 1e-12, (npoly, j, rel.max())
        assert np.linalg.eigvalsh(F / (d[:, None] * d[None, :])).min() > 0
        assert np.array_equal(F, F.T) or np.abs(F - F.T).max() <= 1e-15 * np.abs(F).max()


def test_truth_of_the_penalised_jobs(cases, olibs):
    """outside the grid the template is the nearest node's: only the velocity entry is
    left; with a non-finite parameter every arm is skipped"""
    want = ftruth.truth_jobs(cases, olibs, 10)
    F5 = want[5][0]
    assert F5[0, 0] > 0 and not F5[1:].any() and not F5[:, 1:].any()
    assert not want[6][0].any() and not want[6][1].any()


def test_header_and_binding_agree():
    """rvs_chisq_point_fisher_work_size / rvs_chisq_point_fisher are declared in
    include/rvsgpu.h with the arguments of the gradient entries (plus `fisher`), carry
    the kinds the ctypes table gives them, are exported, and refuse what the gradient
    refuses -- and a NULL fisher -- before any launch; the ABI number did not move"""
    from rvspecfit_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
    txt = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    decl = {}
    for name in ('rvs_chisq_point_grad', 'rvs_chisq_point_fisher',
                 'rvs_chisq_point_grad_work_size', 'rvs_chisq_point_fisher_work_size'):
        m = re.search(r'\bint(?:64_t)?\s+%s\s*\(([^;]*?)\)\s*;' % name, txt, flags=re.S)
        assert m, name + ' is not declared'
        decl[name] = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert decl['rvs_chisq_point_fisher_work_size'] == \
        decl['rvs_chisq_point_grad_work_size']
    g, f = decl['rvs_chisq_point_grad'], decl['rvs_chisq_point_fisher']
    assert f[:13] == g[:13] and f[13] == 'double *fisher' and f[14:] == g[13:]
    kinds = [ctypes.c_void_p if '*' in a else
             {'int': ctypes.c_int, 'double': ctypes.c_double}[a.split()[0]] for a in f]
    res, args = _lib.SIGNATURES['rvs_chisq_point_fisher']
    assert res is ctypes.c_int and args == kinds
    assert _lib.SIGNATURES['rvs_chisq_point_fisher_work_size'] == \
        _lib.SIGNATURES['rvs_chisq_point_grad_work_size']
    L = _lib.lib()
    assert L.rvs_abi_version() == 18
    ws = L.rvs_chisq_point_fisher_work_size
    for J, narm, ntan in ((1, 1, 0), (7, 2, 4), (8192, 3, 6)):
        K = 1 + ntan
        assert ws(J, narm, ntan) == narm * J * ((1 + K + K * K) * 8 + 4)
        assert ws(J, narm, ntan) == L.rvs_chisq_point_grad_work_size(J, narm, ntan) \
            + narm * J * K * K * 8
    assert ws(0, 1, 4) == 0 and ws(1, 0, 4) == 0 and ws(1, 1, 7) == 0
    assert ws(1, 1, -1) == 0

    def arm(**kw):
        p = _lib.PointArm()
        p.npix, p.ntp, p.S, p.G = 100, 10, 1, 1
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    a = ctypes.c_void_p(64)     # never dereferenced

    def call(p, npoly, ntan, fisher=a):
        return L.rvs_chisq_point_fisher(ctypes.addressof(p), 1, npoly, ntan, None, None,
                                        1, a, 1.0, None, a, a, a, fisher, a, None)
    ok = arm()
    assert call(ok, 10, 7) == -1            # ntan > 6
    assert call(ok, 10, -1) == -1
    assert call(ok, 0, 4) == -1             # npoly outside 1 .. 16
    assert call(ok, 17, 4) == -1
    assert call(ok, 10, 4, None) == -1      # fisher == NULL
    assert call(arm(G=2), 10, 4) == -1      # a grid set
    assert call(arm(taps=64), 10, 4) == -1  # a resolution matrix
    assert call(arm(fast_interp=1), 10, 4) == -1


# ---- the host part of fisher_uncertainties -------------------------------------------
NAMES = ['vel', 'teff', 'logg', 'feh', 'alpha']
STELLAR = NAMES[1:]


def _psd(rng, n, scales, rank=None):
    A = rng.standard_normal((rank or 3 * n, n)) * np.asarray(scales)[None, :]
    return A.T @ A


def test_prior_adds_its_inverse_variance_and_fixed_parameters_leave():
    from rvspecfit_amd.vel_fit import _uncertainties_from_fisher
    rng = np.random.default_rng(5)
    F = np.array([_psd(rng, 5, [1, 1e-3, 1, 2, 3]) for _ in range(3)])
    r0 = _uncertainties_from_fisher(F, NAMES, STELLAR)
    assert r0['names'] == NAMES and np.array_equal(r0['fisher'], F)
    sig = np.array([150.0, 100.0, 50.0])
    r1 = _uncertainties_from_fisher(F, NAMES, STELLAR, {'teff': 1 / sig**2,
                                                        'feh': 1 / 0.3**2})
    want = F.copy()
    want[:, 1, 1] += 1 / sig**2
    want[:, 3, 3] += 1 / 0.3**2
    assert np.array_equal(r1['fisher'], want)
    r2 = _uncertainties_from_fisher(F, NAMES, STELLAR, fixParam=['logg'])
    assert r2['names'] == ['vel', 'teff', 'feh', 'alpha']
    keep = [0, 1, 3, 4]
    assert np.array_equal(r2['fisher'], F[:, keep][:, :, keep])
    assert list(r2['param_err']) == ['teff', 'feh', 'alpha']
    assert r2['covar'].shape == (3, 4, 4) and r2['param_covar'].shape == (3, 3, 3)
    # the inverses: joint over names, the stellar block on its own
    for s in range(3):
        inv = np.linalg.inv(F[s])
        assert np.allclose(r0['covar'][s], inv, rtol=1e-9, atol=0)
        assert np.allclose(r0['vel_err'][s], np.sqrt(inv[0, 0]), rtol=1e-9)
        pinv = np.linalg.inv(F[s][1:, 1:])
        assert np.allclose(r0['param_covar'][s], pinv, rtol=1e-9, atol=0)
        for i, k in enumerate(STELLAR):
            assert np.isclose(r0['param_err'][k][s], np.sqrt(pinv[i, i]), rtol=1e-9)
            assert r0['err'][k][s] >= r0['param_err'][k][s] * (1 - 1e-12)
    assert not r0['bad_fisher'].any()


def test_zero_row_is_bad_and_takes_the_diagonal():
    """a parameter the model does not depend on: no exception, bad_fisher, the
    reference's diagonal fallback 1 / F_ii (infinite for the zero entry)"""
    from rvspecfit_amd.vel_fit import _uncertainties_from_fisher
    rng = np.random.default_rng(6)
    F = np.array([_psd(rng, 5, [1, 1e-3, 1, 2, 3]) for _ in range(2)])
    F[1, 2, :] = 0
    F[1, :, 2] = 0
    r = _uncertainties_from_fisher(F, NAMES, STELLAR)
    assert list(r['bad_fisher']) == [False, True]
    d = np.diag(F[1])
    with np.errstate(all='ignore'):
        want = np.sqrt(1 / d)
    assert np.isinf(r['err']['logg'][1]) and np.isinf(r['param_err']['logg'][1])
    for i, k in enumerate(NAMES):
        if k != 'logg':
            assert np.isclose(r['err'][k][1], want[i], rtol=1e-12)
    assert np.isfinite(r['vel_err'][1])
    # an all-zero matrix (every arm skipped)
    r = _uncertainties_from_fisher(np.zeros((1, 5, 5)), NAMES, STELLAR)
    assert r['bad_fisher'][0] and np.isinf(r['vel_err'][0])


def test_psd_input_gives_no_nan_where_the_references_rule_gives_a_number():
    from rvspecfit_amd.vel_fit import (_uncertainties_from_fisher,
                                       _uncertainties_from_hessian)
    rng = np.random.default_rng(7)
    mats = []
    for t in range(40):
        scales = 10.0**rng.uniform(-5, 3, 5)            # K beside dex and worse
        mats.append(_psd(rng, 5, scales, rank=[15, 5, 4, 2][t % 4]))
    F = np.array(mats)
    r = _uncertainties_from_fisher(F, NAMES, STELLAR)
    err = np.array([r['err'][k] for k in NAMES]).T
    for s in range(len(F)):
        ref = _uncertainties_from_hessian(F[s])[0]
        assert not np.isnan(err[s][~np.isnan(ref)]).any(), (s, err[s], ref)
        assert not np.isnan(err[s]).any()
    full = np.array([t % 4 == 0 for t in range(40)])
    assert not r['bad_fisher'][full].any() and np.isfinite(err[full]).all()
