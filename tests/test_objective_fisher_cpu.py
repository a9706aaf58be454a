"""The fused value / gradient / Fisher entry points (csrc/objective_fisher.hip, DESIGN
4.23) without a GPU: their declarations against the binding, what
rvs_objective_fisher_ok admits and refuses against a Python statement of its rule,
argument errors before any launch -- and the forward-mode method itself, restated in
numpy (tests/objective_fisher_restated.py), against the float64 truths of
tests/chisq_fisher_truth.py (autograd Jacobian, QR projection) and
tests/chisq_grad_truth.py / vsini_grad_truth.py.

The bounds are the project's own for these sums: the Fisher matrix within
test_chisq_fisher_gpu.BOUND (10 x 5.84e-13) of sqrt(G_ii G_ll), the gradient within the
same figure in the measure of test_objective_grad_gpu._rel.  The restatement measures,
over the five in-cell JOBS on both golden arms (npoly 5 / 10, without / with the vsini
column): Fisher matrix 1.2e-15 ... 5.6e-15, gradient 1.5e-13 ... 2.2e-13, value 2.5e-13
of max(|chi^2|, 1e3) -- all inside, so the device tests keep the same bounds."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import chisq_fisher_truth as ftruth
import objective_fisher_restated as fwd
import vsini_grad_truth as vtruth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED_REL_ERR = 5.84e-13          # tests/test_chisq_grad_gpu.py
BOUND = 10 * MEASURED_REL_ERR        # tests/test_chisq_fisher_gpu.py
NEW = {
    'rvs_objective_fisher_ok': 'int npoly, int npix, int ntp, int ndim, int vsini_grad',
    'rvs_objective_fisher_work_size': 'int J, int narm, int ntan, int npix_max',
    'rvs_objective_fisher':
        'const rvs_objective_arm *arms, int narm, int npoly, int ntan, '
        'const double *params, const double *vsini, const int32_t *job_spec, int J, '
        'const double *vel, double badchi, const double *basis_const, void *work, '
        'int64_t work_bytes, double *out, double *grad, double *fisher, '
        'int32_t *status, void *stream',
}
# (npix, ntp): the three DESI arms, the two golden arms
DESI = [(2751, 6215), (2326, 5303), (2881, 6449)]
GOLDEN = [(401, 977), (301, 781)]


def _norm(decl):
    return ' '.join(decl.replace('*', ' * ').split())


def test_constants_are_the_gpu_modules():
    """(the GPU modules cannot be imported by a CPU test's collection on every machine:
    the figures are restated here and compared where they can be)"""
    src = open(os.path.join(REPO, 'tests', 'test_chisq_grad_gpu.py')).read()
    assert re.search(r'^MEASURED_REL_ERR = 5\.84e-13', src, flags=re.M)
    src = open(os.path.join(REPO, 'tests', 'test_chisq_fisher_gpu.py')).read()
    assert re.search(r'^BOUND = 10 \* MEASURED_REL_ERR', src, flags=re.M)


def test_symbols_and_signatures():
    from rvspecfit_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
    txt = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    L = _lib.lib()
    for name, want in NEW.items():
        m = re.search(r'\b(int|int64_t)\s+%s\s*\(([^;]*?)\)\s*;' % name, txt, flags=re.S)
        assert m, name + ' is not declared'
        got = [_norm(a) for a in m.group(2).split(',')]
        assert got == [_norm(a) for a in want.split(',')], name
        kinds = [ctypes.c_void_p if '*' in a else
                 {'int': ctypes.c_int, 'double': ctypes.c_double,
                  'int64_t': ctypes.c_int64}[a.split()[0]] for a in got]
        res, args = _lib.SIGNATURES[name]
        assert args == kinds, name
        assert res is (ctypes.c_int64 if m.group(1) == 'int64_t' else ctypes.c_int)
        assert hasattr(L, name)


def _rule(npoly, npix, ntp, ndim, vsini_grad):
    """rvs_objective_fisher_ok in Python: npoly 1..10, ndim 1..4, 32 <= ntp (and within
    the chunk table of the spline factors), the pixels twice in one buffer, three
    buffers of ntp doubles beside 8 KB of static LDS within 160 KB"""
    return int(1 <= npoly <= 10 and npix >= 1 and 32 <= ntp <= 512 * 16 and
               1 <= ndim <= 4 and vsini_grad in (0, 1) and 2 * npix <= ntp and
               3 * ntp * 8 + 8192 <= 160 * 1024)


def test_fisher_ok_is_its_rule():
    from rvspecfit_amd import _lib
    ok = _lib.lib().rvs_objective_fisher_ok
    geoms = list(DESI + GOLDEN)
    geoms += [(10, 31), (10, 32), (16, 32), (17, 32), (15, 31), (16, 33), (17, 33)]
    geoms += [(n // 2, n) for n in (6400, 6485, 6486, 8000)]
    geoms += [(n // 2 + 1, n) for n in (976, 977)]           # 2 npix = ntp + 1 (+ 2)
    geoms += [(488, 976), (0, 977), (3000, 8000)]
    seen = set()
    for npix, ntp in geoms:
        for npoly in (0, 1, 5, 10, 11, 17):
            for ndim in (0, 1, 4, 5):
                for vg in (0, 1, 2):
                    want = _rule(npoly, npix, ntp, ndim, vg)
                    assert ok(npoly, npix, ntp, ndim, vg) == want, \
                        (npoly, npix, ntp, ndim, vg)
                    seen.add(want)
    assert seen == {0, 1}
    # what the issue names: the DESI arms at npoly 10 with and without the vsini row, ...
    for npix, ntp in DESI:
        assert ok(10, npix, ntp, 4, 0) == 1 and ok(10, npix, ntp, 4, 1) == 1
    # ... the edges ntp = 31 / 32, 2 npix = ntp / ntp + 1, npoly 10 / 11, ndim 4 / 5
    assert ok(10, 10, 31, 4, 0) == 0 and ok(10, 10, 32, 4, 0) == 1
    assert ok(10, 16, 32, 4, 0) == 1 and ok(10, 17, 33, 4, 0) == 0
    assert ok(10, 401, 977, 4, 0) == 1 and ok(11, 401, 977, 4, 0) == 0
    assert ok(10, 401, 977, 5, 0) == 0
    # the same arms as rvs_objective_grad_ok
    gok = _lib.lib().rvs_objective_grad_ok
    for npix, ntp in geoms:
        assert ok(10, npix, ntp, 4, 1) == gok(10, npix, ntp, 4, 1)


def test_work_size():
    from rvspecfit_amd import _lib
    ws = _lib.lib().rvs_objective_fisher_work_size
    K = 6
    per = (3 + K + K * K + (K + 2) * 401) * 8
    assert ws(1, 2, 5, 401) == 2 * per
    assert ws(100, 2, 5, 401) == 100 * ws(1, 2, 5, 401)
    for bad in ((0, 1, 4, 10), (10, 0, 4, 10), (10, 5, 4, 10), (10, 1, 0, 10),
                (10, 1, 6, 10), (-1, 1, 4, 10), (10, 1, 4, 0)):
        assert ws(*bad) == 0, bad


def test_argument_validation_without_gpu():
    """RVS_E_ARG for NULL or out-of-range arguments and for a work buffer below the
    one-job size, before any device is touched"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    a = ctypes.c_void_p(64)      # never dereferenced
    f = L.rvs_objective_fisher
    arr = (_lib.ObjectiveArm * 1)()
    arms = ctypes.addressof(arr)
    arr[0].ndim, arr[0].ntp = 4, 977
    arr[0].pt.npix, arr[0].pt.ntp = 401, 977
    for fld in ('dats', 'idgrid', 'uvecs', 'vecs_s', 'factors'):
        setattr(arr[0], fld, 64)
    one = L.rvs_objective_fisher_work_size(1, 1, 4, 401)
    names = ['arms', 'narm', 'npoly', 'ntan', 'params', 'vsini', 'job_spec', 'J', 'vel',
             'badchi', 'basis_const', 'work', 'work_bytes', 'out', 'grad', 'fisher',
             'status', 'stream']
    # (the work buffer one byte short: the only call here that passes the other checks)
    good = [arms, 1, 10, 4, a, None, None, 1, a, 1.0, None, a, one - 1, a, a, a, a, None]

    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    assert call() == -1                                  # work_bytes < one job
    assert call(work_bytes=0) == -1 and call(work_bytes=-8) == -1
    assert call(arms=None, work_bytes=one) == -1
    assert call(J=0, work_bytes=one) == -1
    assert call(narm=0, work_bytes=one) == -1 and call(narm=5, work_bytes=one) == -1
    for p in (0, 11, 17):
        assert call(npoly=p, work_bytes=one) == -1
    assert call(ntan=3, work_bytes=one) == -1 and call(ntan=6, work_bytes=one) == -1
    assert call(ntan=5, work_bytes=10 * one) == -1       # vsini fitted without vsini
    for k in ('params', 'vel', 'work', 'out', 'grad', 'fisher', 'status'):
        assert call(work_bytes=one, **{k: None}) == -1, k
    arr[0].pt.npix = 600                                 # 2 npix > ntp
    assert call(work_bytes=10 * one) == -1
    arr[0].pt.npix = 401
    arr[0].pt.fast_interp = 1
    assert call(work_bytes=one) == -1
    arr[0].pt.fast_interp = 0
    arr[0].pt.taps = 64                                  # a resolution matrix
    assert call(work_bytes=one) == -1
    arr[0].pt.taps = None
    arr[0].pt.G = 2                                      # a grid set
    assert call(work_bytes=one) == -1
    arr[0].pt.G = 0
    arr[0].ndim = 5
    assert call(ntan=5, work_bytes=10 * one) == -1


# ---- the method -----------------------------------------------------------------------
def _rel(g, ref):                     # tests/test_objective_grad_gpu.py
    return np.abs(g - ref) / np.maximum(np.abs(ref), 1e-6 * np.abs(ref).max())


@pytest.mark.parametrize('vsini_grad', [False, True])
@pytest.mark.parametrize('npoly', [5, 10])
def test_restatement_against_the_truths(cases, gold_libs, npoly, vsini_grad):
    sp = truth.spectra(cases, orc.SpecData)
    gref = truth.truth_jobs(cases, gold_libs, npoly)
    worst_f = worst_g = worst_v = 0.0
    for job in truth.INSIDE:
        s, vel, par, vs = truth.JOBS[job]
        val, g, F, G = fwd.value_grad_fisher(sp[s], gold_libs, vel, par, vs, npoly=npoly,
                                             vsini_grad=vsini_grad)
        Ft, Gt, cond = fwd.fisher_truth(sp[s], gold_libs, vel, par, vs, npoly=npoly,
                                        vsini_grad=vsini_grad)
        K = 5 + int(vsini_grad)
        assert F.shape == Ft.shape == (K, K) and cond < 100
        if vsini_grad:
            _, gt = vtruth.chisq_and_grad_vsini(sp[s], gold_libs, vel, par, vs or 0.0,
                                                npoly=npoly)
            if vs is None:    # the copy branch: row and column exactly 0, also the truth's
                assert not F[5].any() and not F[:, 5].any() and g[5] == 0.0
                assert not Ft[5].any() and not Ft[:, 5].any()
            else:
                assert F[5, 5] > 0
        else:
            gt = gref[job][1]
            # (this module's truth without vsini IS chisq_fisher_truth's)
            want = ftruth.truth_jobs(cases, gold_libs, npoly)[job]
            assert np.array_equal(Ft, want[0])
        ef = fwd.rel_fisher(F, Ft, Gt).max()
        eg = _rel(g, gt).max()
        ev = abs(val - gref[job][0]) / max(abs(gref[job][0]), 1e3)
        print('npoly %d vsini %d job %d Fisher %.3g gradient %.3g value %.3g'
              % (npoly, vsini_grad, job, ef, eg, ev))
        worst_f, worst_g, worst_v = max(worst_f, ef), max(worst_g, eg), max(worst_v, ev)
    print('npoly %d vsini %d largest Fisher error %.3g gradient %.3g value %.3g (bound '
          '%.3g)' % (npoly, vsini_grad, worst_f, worst_g, worst_v, BOUND))
    assert worst_f <= BOUND
    assert worst_g <= BOUND
    assert worst_v <= 2.6e-12


@pytest.mark.parametrize('vsini_grad', [False, True])
def test_column_truth_is_the_autograd_truth(cases, gold_libs, vsini_grad):
    """fisher_truth_columns (the Jacobian's columns through the truth's own linear path:
    what the large shapes of tests/objective_grad_shapes.py can afford) against
    fisher_truth (autograd's Jacobian) on the golden jobs, the outside one included:
    1e-13 of sqrt(G_ii G_ll), a hundred times the rounding of either and far below
    the bound both serve"""
    sp = truth.spectra(cases, orc.SpecData)
    for job in truth.INSIDE + [5]:
        s, vel, par, vs = truth.JOBS[job]
        a = fwd.fisher_truth(sp[s], gold_libs, vel, par, vs, npoly=10,
                             vsini_grad=vsini_grad)
        b = fwd.fisher_truth_columns(sp[s], gold_libs, vel, par, vs, npoly=10,
                                     vsini_grad=vsini_grad)
        ef, eg = fwd.rel_fisher(b[0], a[0], a[1]).max(), \
            fwd.rel_fisher(b[1], a[1], a[1]).max()
        print('job %d vsini %d F %.3g G %.3g' % (job, vsini_grad, ef, eg))
        assert ef <= 1e-13 and eg <= 1e-13
        assert abs(a[2] - b[2]) <= 1e-9 * a[2]


def test_restatement_intermediates(cases, gold_libs):
    """the stages are exposed and are what they claim: the tangent at the pixels is the
    central difference of the model row, B = L^-1 B' is the sum over y(k), F is the
    projected Gram matrix, g is the adjoint restatement's gradient"""
    import objective_adjoint_restated as adj
    sp = truth.spectra(cases, orc.SpecData)
    s, vel, par, vs = truth.JOBS[3]
    _, g, F, G, arms = fwd.value_grad_fisher(sp[s], gold_libs, vel, par, vs, npoly=10,
                                             vsini_grad=True, details=True)
    _, ga = adj.chisq_and_grad(sp[s], gold_libs, vel, par, vs, npoly=10, vsini_grad=True)
    assert _rel(g, ga).max() <= BOUND
    steps = [0.05, 1.0, 1e-3, 1e-3, 1e-3, 0.01]
    for a, sd in zip(arms, sp[s]):
        lib = gold_libs[sd.name]
        N, npix = len(lib.lam), len(sd.lam)
        for k, shape in (('tknots', (6, N)), ('yknots', (6, N)), ('zknots', (6, N)),
                         ('mdot', (npix, 6)), ('J', (npix, 6)), ('Bp', (10, 6)),
                         ('B', (10, 6))):
            assert a[k].shape == shape and np.all(np.isfinite(a[k])), k
        theta = np.array([vel] + list(par) + [vs])
        for i in range(6):
            rows = []
            for sg in (1, -1):
                th = theta.copy()
                th[i] += sg * steps[i]
                rows.append(fwd.arm(sd, lib, th[0], th[1:5], th[5], 10)['m'])
            fd = (rows[0] - rows[1]) / (2 * steps[i])
            err = np.abs(fd - a['mdot'][:, i]).max() / np.abs(a['mdot'][:, i]).max()
            assert err <= 1e-5, (i, err)
        # B against the definition with y(k) = L^-1 phi_k, F against the QR projection
        Q = truth.ortho_basis(sd.lam, 10, True)[0].numpy()
        ST = Q * a['te'][None, :]
        L = np.linalg.cholesky(ST @ ST.T)
        Bdef = (np.linalg.solve(L, Q) * a['te'][None, :]) @ a['J']
        assert np.abs(Bdef - a['B']).max() <= 1e-12 * np.abs(Bdef).max()
        U, _ = np.linalg.qr(ST.T)
        Jp = a['J'] - U @ (U.T @ a['J'])
        assert fwd.rel_fisher(a['fisher'], Jp.T @ Jp, a['gram']).max() <= BOUND


def test_restatement_outside_and_nonfinite(cases, gold_libs):
    """job 5 (outside the grid): parameter rows and columns exactly 0, the velocity
    entry the truth's; job 6: the penalty, a zero gradient and a zero matrix"""
    sp = truth.spectra(cases, orc.SpecData)
    for npoly in (5, 10):
        want = ftruth.truth_jobs(cases, gold_libs, npoly)
        s, vel, par, vs = truth.JOBS[5]
        val, g, F, G = fwd.value_grad_fisher(sp[s], gold_libs, vel, par, vs, npoly=npoly)
        assert not F[1:].any() and not F[:, 1:].any() and not g[1:].any()
        assert abs(F[0, 0] - want[5][0][0, 0]) <= BOUND * want[5][1][0, 0]
        s, vel, par, vs = truth.JOBS[6]
        val, g, F, G = fwd.value_grad_fisher(sp[s], gold_libs, vel, par, vs, npoly=npoly)
        assert not F.any() and not g.any()
        assert val == 2 * 1000.0 * 10 * sum(len(sd.lam) for sd in sp[s])
