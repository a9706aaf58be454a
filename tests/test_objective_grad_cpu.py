"""The fused objective-and-gradient entry points (csrc/objective_grad.hip) without a
GPU: their declarations against the binding, what rvs_objective_grad_ok admits and
refuses, argument errors before any launch -- and the adjoint method itself, restated
in numpy (tests/objective_adjoint_restated.py), against the float64 autograd truth of
tests/chisq_grad_truth.py.

The restatement's errors against the truth, measured on the five in-cell JOBS, both
golden arms (relative to max(|g_k|, 1e-6 |g|_inf); values relative to
max(|chi^2|, 1e3)):
    npoly  5: gradient 1.3e-13    npoly 10: 2.6e-13    npoly 16: 1.2e-12
    values within 2.6e-13
The bounds below are 10 x those."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import objective_adjoint_restated as adj
import vsini_grad_truth as vtruth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    'rvs_objective_grad_ok': 'int npoly, int npix, int ntp, int ndim, int vsini_grad',
    'rvs_objective_grad_work_size': 'int J, int narm, int ntan',
    'rvs_objective_grad':
        'const rvs_objective_arm *arms, int narm, int npoly, int ntan, '
        'const double *params, const double *vsini, const int32_t *job_spec, int J, '
        'const double *vel, double badchi, const double *basis_const, void *scratch, '
        'double *out, double *grad, int32_t *status, void *stream',
    'rvs_bfgs_run_grad_fused':
        'const rvs_bfgs_state *b, const rvs_nm_objective *o, const rvs_grad_chain *g, '
        'const rvs_objective_arm *garms, const double *basis_const, void *gwork, '
        'int sync_every, int64_t *stats, void *stream',
}
# (npix, ntp): the three DESI arms, the two golden arms
DESI = [(2751, 6215), (2326, 5303), (2881, 6449)]
GOLDEN = [(401, 977), (301, 781)]


def _norm(decl):
    return ' '.join(decl.replace('*', ' * ').split())


def test_symbols_and_signatures():
    """the four symbols are declared as the issue states them, bound with matching
    ctypes lists and exported; the ABI number did not move"""
    from rvspecfit_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
    assert _lib.ABI_VERSION == 18
    txt = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    L = _lib.lib()
    assert L.rvs_abi_version() == 18
    for name, want in NEW.items():
        m = re.search(r'\b(int|int64_t)\s+%s\s*\(([^;]*?)\)\s*;' % name, txt, flags=re.S)
        assert m, name + ' is not declared'
        got = [_norm(a) for a in m.group(2).split(',')]
        assert got == [_norm(a) for a in want.split(',')], name
        kinds = [ctypes.c_void_p if '*' in a else
                 {'int': ctypes.c_int, 'double': ctypes.c_double}[a.split()[0]]
                 for a in got]
        res, args = _lib.SIGNATURES[name]
        assert args == kinds, name
        assert res is (ctypes.c_int64 if m.group(1) == 'int64_t' else ctypes.c_int)
        assert hasattr(L, name)


def test_grad_ok_admits_and_refuses():
    from rvspecfit_amd import _lib
    ok = _lib.lib().rvs_objective_grad_ok
    for npix, ntp in DESI + GOLDEN:
        for vg in (0, 1):
            assert ok(10, npix, ntp, 4, vg) == 1, (npix, ntp, vg)
            assert ok(1, npix, ntp, 1, vg) == 1
    assert ok(10, 10, 31, 4, 0) == 0          # ntp < 32
    assert ok(10, 16, 32, 4, 0) == 1
    assert ok(10, 17, 32, 4, 0) == 0          # 2 npix > ntp
    assert ok(10, 401, 977, 5, 0) == 0        # ndim 5
    assert ok(10, 401, 977, 0, 0) == 0
    assert ok(0, 401, 977, 4, 0) == 0         # npoly 0
    assert ok(17, 401, 977, 4, 0) == 0        # npoly 17
    assert ok(10, 3000, 8000, 4, 0) == 0      # three buffers do not fit LDS


def test_work_size():
    from rvspecfit_amd import _lib
    ws = _lib.lib().rvs_objective_grad_work_size
    assert ws(100, 2, 5) == 2 * 100 * (4 + 5) * 8
    for bad in ((0, 1, 4), (10, 0, 4), (10, 5, 4), (10, 1, 0), (10, 1, 6), (-1, 1, 4)):
        assert ws(*bad) == 0, bad


def test_argument_validation_without_gpu():
    """RVS_E_ARG for NULL or out-of-range arguments, before any device is touched"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    a = ctypes.c_void_p(64)      # never dereferenced
    f = L.rvs_objective_grad
    assert f(None, 1, 10, 4, a, None, None, 1, a, 1.0, None, a, a, a, a, None) == -1
    arr = (_lib.ObjectiveArm * 1)()
    arms = ctypes.addressof(arr)
    arr[0].ndim, arr[0].ntp = 4, 977
    arr[0].pt.npix, arr[0].pt.ntp = 401, 977
    for fld in ('dats', 'idgrid', 'uvecs', 'vecs_s', 'factors'):
        setattr(arr[0], fld, 64)
    good = [arms, 1, 10, 4, a, None, None, 1, a, 1.0, None, a, a, a, a, None]

    def call(**kw):
        names = ['arms', 'narm', 'npoly', 'ntan', 'params', 'vsini', 'job_spec', 'J',
                 'vel', 'badchi', 'basis_const', 'scratch', 'out', 'grad', 'status',
                 'stream']
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    assert call(J=0) == -1
    assert call(narm=0) == -1 and call(narm=5) == -1
    assert call(npoly=0) == -1 and call(npoly=11) == -1 and call(npoly=17) == -1
    assert call(ntan=3) == -1 and call(ntan=6) == -1
    assert call(ntan=5) == -1                     # vsini fitted without vsini
    for k in ('params', 'vel', 'scratch', 'out', 'grad', 'status'):
        assert call(**{k: None}) == -1, k
    arr[0].pt.npix = 600                          # 2 npix > ntp
    assert call() == -1
    arr[0].pt.npix = 401
    arr[0].pt.fast_interp = 1
    assert call() == -1
    arr[0].pt.fast_interp = 0
    arr[0].pt.taps = 64                           # a resolution matrix
    assert call() == -1
    arr[0].pt.taps = None
    arr[0].pt.G = 2                               # a grid set
    assert call() == -1
    arr[0].pt.G = 0
    arr[0].ndim = 5
    assert call(ntan=5) == -1
    g = L.rvs_bfgs_run_grad_fused
    assert g(None, None, None, None, None, None, 1, None, None) == -1
    b, o, gc = _lib.BfgsState(), _lib.NmObjective(), _lib.GradChain()
    assert g(ctypes.addressof(b), ctypes.addressof(o), ctypes.addressof(gc), arms, None,
             a, 1, None, None) == -1              # empty descriptors
    b.S, b.n, o.n = 1, 1, 1
    assert g(ctypes.addressof(b), ctypes.addressof(o), ctypes.addressof(gc), arms, None,
             a, 0, None, None) == -1              # sync_every < 1


# ---- the method ---------------------------------------------------------------------
def _err(g, ref):
    return float((np.abs(g - ref) / np.maximum(np.abs(ref),
                                                1e-6 * np.abs(ref).max())).max())


@pytest.mark.parametrize('npoly,bound', [(5, 1.3e-12), (10, 2.6e-12), (16, 1.2e-11)])
def test_restatement_against_the_truth(cases, gold_libs, npoly, bound):
    sp = truth.spectra(cases, orc.SpecData)
    ref = truth.truth_jobs(cases, gold_libs, npoly)
    worst_g = worst_v = 0.0
    for job in truth.INSIDE:
        s, vel, par, vs = truth.JOBS[job]
        val, g = adj.chisq_and_grad(sp[s], gold_libs, vel, par, vs, npoly=npoly)
        worst_g = max(worst_g, _err(g, ref[job][1]))
        worst_v = max(worst_v, abs(val - ref[job][0]) / max(abs(ref[job][0]), 1e3))
    print('npoly %d largest gradient error %.3g value error %.3g'
          % (npoly, worst_g, worst_v))
    assert worst_g <= bound
    assert worst_v <= 2.6e-12


def test_restatement_outside_and_nonfinite(cases, gold_libs):
    """job 5 (outside the grid): parameter components exactly 0, velocity component the
    truth's; job 6: the penalty and a zero gradient"""
    sp = truth.spectra(cases, orc.SpecData)
    ref = truth.truth_jobs(cases, gold_libs, 10)
    for job in (5, 6):
        s, vel, par, vs = truth.JOBS[job]
        val, g = adj.chisq_and_grad(sp[s], gold_libs, vel, par, vs, npoly=10)
        assert abs(val - ref[job][0]) <= 2.6e-12 * max(abs(ref[job][0]), 1e3)
        assert np.all(g[1:] == 0)
        assert abs(g[0] - ref[job][1][0]) <= 2.6e-12 * max(abs(ref[job][1][0]), 1e-30)
    assert g[0] == 0


def test_restatement_intermediates(cases, gold_libs):
    """the adjoint rows are exposed and consistent: <mbar, dm> = <tbar, dt> for a
    perturbation dt of the template pushed forward through FIR, spline and
    resampling (the transposes are the transposes)"""
    sp = truth.spectra(cases, orc.SpecData)
    s, vel, par, vs = truth.JOBS[3]
    _, _, arms = adj.chisq_and_grad(sp[s], gold_libs, vel, par, vs, npoly=10,
                                    details=True)
    rng = np.random.default_rng(5)
    for a, sd in zip(arms, sp[s]):
        for k in ('mbar', 'ybar', 'zbar', 'u', 'tbar'):
            assert np.all(np.isfinite(a[k])), k
        lib = gold_libs[sd.name]
        N = len(lib.lam)
        assert a['ybar'].shape == a['tbar'].shape == (N, )
        assert a['zbar'].shape == a['u'].shape == (N - 2, )
        dt = rng.standard_normal(N) * a['t']
        w, _ = vtruth.taps((vs / truth.C_KMS) / vtruth.lnstep(lib))
        import torch
        f = np.sqrt((1 - vel / truth.C_KMS) / (1 + vel / truth.C_KMS))
        dm = truth.spline_eval(lib.lam, torch.as_tensor(np.convolve(dt, w, 'same')),
                               torch.as_tensor(sd.lam * f)).numpy()
        lhs, rhs = a['mbar'] @ dm, a['tbar'] @ dt
        assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs))


def test_restatement_vsini_component(cases, gold_libs):
    """the derived d chi^2 / d vsini = sum_n vbar_n t_n against the Richardson central
    difference of the truth's value, as test_vsini_grad_cpu.py holds the truth's own"""
    npoly = 10
    s, vel, par, vs = truth.JOBS[3]
    sds = truth.spectra(cases, orc.SpecData)[s]
    val, g = adj.chisq_and_grad(sds, gold_libs, vel, par, vs, npoly=npoly,
                                vsini_grad=True)
    h0 = 0.2
    d = []
    for h in (h0, h0 / 2):
        f = [truth.chisq_and_grad(sds, gold_libs, vel, par, vs + e, npoly=npoly)[0]
             for e in (h, -h)]
        d.append((f[0] - f[1]) / (2 * h))
    rich = (4 * d[1] - d[0]) / 3
    noise = (1e-13 * abs(val) + 1e-10) / (h0 / 2) * 5 / 3
    print('d/dvsini adjoint %.12g richardson %.12g diff %.3g bound %.3g'
          % (g[5], rich, g[5] - rich, 1e-6 * abs(g[5]) + noise))
    assert abs(g[5] - rich) <= 1e-6 * abs(g[5]) + noise
    _, gt = vtruth.chisq_and_grad_vsini(sds, gold_libs, vel, par, vs, npoly=npoly)
    assert _err(g, gt) <= 2.6e-12
    _, gz = adj.chisq_and_grad(sds, gold_libs, vel, par, 0.0, npoly=npoly,
                               vsini_grad=True)
    assert gz[5] == 0.0
