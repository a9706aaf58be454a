"""The fused objective-and-gradient entry points under resolution matrices
(csrc/objective_grad.hip, the RESOL form) without a GPU: their declarations
against the binding, what rvs_objective_grad_resol_ok admits and refuses, argument errors
before any launch, the scope checks of config['fused_gradient'] beside
config['resol_gradient'] on stub batches -- and the method itself, restated in numpy
(tests/objective_adjoint_resol_restated.py: the band and its transpose around
objective_adjoint_restated), against the float64 autograd truth under dense matrices of
tests/chisq_grad_resol_truth.py.

The bounds of the restatement are those of tests/test_objective_grad_cpu.py for the same
npoly (gradient relative to max(|g_k|, 1e-6 |g|_inf): 1.3e-12 at npoly 5, 2.6e-12 at
npoly 10; values 2.6e-12 of max(|chi^2|, 1e3)): the band adds nd <= 25 roundings per
pixel to sums of hundreds of terms.  Measured on the five in-cell JOBS under the golden
matrices (9 .. 25 diagonals):
    npoly  5: gradient 1.9e-13 (vsini row 2.1e-14, a matrix on the red arm only 4.7e-13)
    npoly 10: gradient 2.3e-13 (vsini row 4.2e-14, a matrix on the red arm only 1.4e-13)
    values within 2.6e-13
With the matrix on the blue arm only the SUMMED gradient measures 2.6e-12 / 4.4e-12 in that
metric (job 3, d/dfeh): the truth's own per-arm components, -49.9 and +46.4, cancel to
-3.55 there, so an error of 1.5e-11 from the matrix-free red arm -- the same as in the
call without any matrix -- is 14 times larger relative to the sum.  That call is therefore
held to the bound arm by arm, each arm's gradient against the truth of that arm alone,
where nothing cancels between arms: 4.9e-13 / 4.1e-13.

The adjoint row (tbar, from the from-template form) of the restatement under a matrix is
held to float64 autograd with the template row as the leaf through the dense matrix
(tests/adjoint_row_resol_truth.py), relative to the absolute sum behind each entry,
sum_k |mbar_k dm_k/dt_n| (at least 1e-6 of the largest): RESTATED_ROW_ERR, measured 7.3e-13
(3.3e-14 of the row's largest entry).  The restatement and the
truth form the pixels' coordinates x = lam f by the same float64 product; a statement
that forms them otherwise (the kernel: a fused multiply-add behind its own rounding of f)
differs by up to one unit in the last place of x, and the row is that sensitive --
ulp(x) / h = 9e-13 / 0.4 A on the golden libraries: adjoint_row_cases returns what one
ulp of x moves the row by, 2.1e-11 ... 3.1e-10 in the same measure."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import chisq_grad_resol_truth as rtruth
import objective_adjoint_restated as adj
import objective_adjoint_resol_restated as radj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_GRAD = ('const rvs_objective_arm *arms, int narm, int npoly, int ntan, '
         'const double *params, const double *vsini, const int32_t *job_spec, int J, '
         'const double *vel, double badchi, const double *basis_const, void *scratch, '
         'double *out, double *grad, int32_t *status, void *stream')
_FROMT = ('const rvs_objective_arm *arms, int narm, int npoly, int vsini_grad, '
          'const double *const *templ, const double *const *outside, '
          'const double *vsini, const int32_t *job_spec, int J, const double *vel, '
          'double badchi, const double *basis_const, void *scratch, '
          'double *const *tbar, double *out, double *grad, int32_t *status, void *stream')
_RUN = ('const rvs_bfgs_state *b, const rvs_nm_objective *o, const rvs_grad_chain *g, '
        'const rvs_objective_arm *garms, const double *basis_const, void *gwork, ')
NEW = {
    'rvs_objective_grad_resol_ok':
        'int npoly, int npix, int ntp, int ndim, int nd, int vsini_grad',
    'rvs_objective_grad_resol': _GRAD,
    'rvs_objective_grad_from_template_resol': _FROMT,
    'rvs_bfgs_run_grad_fused_resol': _RUN + 'int sync_every, int64_t *stats, void *stream',
    'rvs_bfgs_run_grad_fused_nn_resol':
        _RUN + 'double *const *tbar, void *const *vjp_work, double *const *gparams, '
        'double *grad_vv, int sync_every, int64_t *stats, void *stream',
    'rvs_bfgs_run_grad_fused_tri_resol':
        _RUN + 'double *const *tbar, double *const *gparams, double *grad_vv, '
        'int sync_every, int64_t *stats, void *stream',
}
# the entry points whose arguments the new ones share
PARENT = {'rvs_objective_grad_resol': 'rvs_objective_grad',
          'rvs_objective_grad_from_template_resol': 'rvs_objective_grad_from_template',
          'rvs_bfgs_run_grad_fused_resol': 'rvs_bfgs_run_grad_fused',
          'rvs_bfgs_run_grad_fused_nn_resol': 'rvs_bfgs_run_grad_fused_nn',
          'rvs_bfgs_run_grad_fused_tri_resol': 'rvs_bfgs_run_grad_fused_tri'}
# (npix, ntp): the three DESI arms of bench.py, the two golden arms
DESI = [(2751, 6215), (2326, 5303), (2881, 6449)]
GOLDEN = [(401, 977), (301, 781)]


def _norm(decl):
    return ' '.join(decl.replace('*', ' * ').split())


def test_symbols_and_signatures():
    """the new symbols are declared, bound with matching ctypes lists and exported, with
    the arguments of their parents; the ABI number did not move"""
    from rvspecfit_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
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
        assert res is ctypes.c_int
        assert hasattr(L, name)
        if name in PARENT:
            assert _lib.SIGNATURES[PARENT[name]] == _lib.SIGNATURES[name], name


def test_resol_ok_admits_and_refuses():
    from rvspecfit_amd import _lib
    L = _lib.lib()
    ok = L.rvs_objective_grad_resol_ok
    # the DESI arms of bench.py with 11 diagonals, the golden arms up to 33
    for npix, ntp in DESI:
        for vg in (0, 1):
            assert ok(10, npix, ntp, 4, 11, vg) == 1, (npix, ntp, vg)
            assert ok(10, npix, ntp, 0, 11, vg) == 1          # the from-template form
    for npix, ntp in GOLDEN:
        for nd in (1, 3, 9, 25, 33):
            assert ok(10, npix, ntp, 4, nd, 0) == 1 and ok(1, npix, ntp, 1, nd, 1) == 1
    # nd: odd, 1 .. 33
    for nd in (0, -1, 2, 10, 34, 35, 377):
        assert ok(10, 401, 977, 4, nd, 0) == 0, nd
    # with one diagonal the rule is rvs_objective_grad_ok's
    plain = L.rvs_objective_grad_ok
    for args in ((10, 16, 32, 4, 0), (10, 17, 32, 4, 0), (10, 10, 31, 4, 0),
                 (10, 401, 977, 5, 0), (0, 401, 977, 4, 0), (11, 401, 977, 4, 0),
                 (10, 3000, 8000, 4, 0), (10, 401, 977, 4, 2)):
        npoly, npix, ntp, ndim, vg = args
        assert ok(npoly, npix, ntp, ndim, 1, vg) == plain(*args), args
    # ndim 0 stands for the from-template form: its own rule
    fromt = L.rvs_objective_grad_from_template_ok
    assert ok(10, 401, 977, 0, 1, 0) == fromt(10, 401, 977, 0) == 1
    assert ok(10, 401, 977, -1, 1, 0) == 0
    # the LDS limit: 2 npix + nd - 1 <= ntp
    assert ok(10, 472, 977, 4, 33, 0) == 1         # 944 + 32 = 976
    assert ok(10, 473, 977, 4, 33, 0) == 0         # 946 + 32 = 978
    assert ok(10, 473, 977, 4, 31, 0) == 1         # 946 + 30 = 976
    assert ok(10, 488, 977, 4, 1, 0) == 1 and ok(10, 488, 977, 4, 3, 0) == 0
    assert ok(10, 2881, 6449, 4, 33, 0) == 1 and ok(10, 3209, 6449, 4, 33, 0) == 0


def _arms():
    from rvspecfit_amd import _lib
    arr = (_lib.ObjectiveArm * 1)()
    arr[0].ndim, arr[0].ntp = 4, 977
    arr[0].pt.npix, arr[0].pt.ntp = 401, 977
    for fld in ('dats', 'idgrid', 'uvecs', 'vecs_s', 'factors'):
        setattr(arr[0], fld, 64)
    return arr


def test_argument_validation_without_gpu():
    """RVS_E_ARG for NULL or out-of-range arguments and for a band the kernel does not
    take, before any device is touched; the entry points without the suffix go on
    refusing taps"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    a = ctypes.c_void_p(64)      # never dereferenced
    arr = _arms()
    arms = ctypes.addressof(arr)
    f = L.rvs_objective_grad_resol
    good = [arms, 1, 10, 4, a, None, None, 1, a, 1.0, None, a, a, a, a, None]
    names = ['arms', 'narm', 'npoly', 'ntan', 'params', 'vsini', 'job_spec', 'J', 'vel',
             'badchi', 'basis_const', 'scratch', 'out', 'grad', 'status', 'stream']

    def call(fn=f, **kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return fn(*args)
    assert f(None, 1, 10, 4, a, None, None, 1, a, 1.0, None, a, a, a, a, None) == -1
    assert call(J=0) == -1
    assert call(narm=0) == -1 and call(narm=5) == -1
    assert call(npoly=0) == -1 and call(npoly=11) == -1
    assert call(ntan=3) == -1 and call(ntan=5) == -1
    for k in ('params', 'vel', 'scratch', 'out', 'grad', 'status'):
        assert call(**{k: None}) == -1, k
    arr[0].pt.taps, arr[0].pt.taps_stride = 64, 401 * 35
    for nd in (0, 2, 35):                         # even, too wide
        arr[0].pt.nd = nd
        assert call() == -1, nd
    arr[0].pt.nd, arr[0].pt.taps_stride = 33, 401 * 33
    arr[0].pt.npix = 473                          # 2 npix + nd - 1 > ntp
    assert call() == -1
    arr[0].pt.npix = 401
    arr[0].pt.taps_stride = 401 * 33 - 1          # rows of another spectrum
    assert call() == -1
    arr[0].pt.taps_stride = 401 * 33
    arr[0].pt.fast_interp = 1
    assert call() == -1
    arr[0].pt.fast_interp = 0
    arr[0].pt.G = 2
    assert call() == -1
    arr[0].pt.G = 0
    # the parent refuses the same descriptor for its taps alone
    assert call(fn=L.rvs_objective_grad) == -1
    # the from-template form
    h = L.rvs_objective_grad_from_template_resol
    rows = ctypes.cast((ctypes.c_void_p * 1)(64), ctypes.c_void_p)
    tgood = [arms, 1, 10, 0, rows, rows, None, None, 1, a, 1.0, None, a, rows, a, a, a,
             None]
    assert h(*tgood[:4], None, *tgood[5:]) == -1
    arr[0].pt.nd = 35
    assert h(*tgood) == -1
    arr[0].pt.nd, arr[0].pt.npix = 33, 473
    assert h(*tgood) == -1
    arr[0].pt.npix = 401
    assert L.rvs_objective_grad_from_template(*tgood) == -1     # taps
    assert h(*tgood[:3], 1, *tgood[4:]) == -1                   # vsini_grad without vsini
    # the runs
    b, o, gc = _lib.BfgsState(), _lib.NmObjective(), _lib.GradChain()
    head = [ctypes.addressof(b), ctypes.addressof(o), ctypes.addressof(gc), arms, None, a]
    g = L.rvs_bfgs_run_grad_fused_resol
    assert g(None, None, None, None, None, None, 1, None, None) == -1
    assert g(*head, 1, None, None) == -1              # empty descriptors
    assert L.rvs_bfgs_run_grad_fused_nn_resol(*head, rows, rows, rows, a, 1, None,
                                              None) == -1
    assert L.rvs_bfgs_run_grad_fused_tri_resol(*head, rows, rows, a, 1, None, None) == -1
    b.S, b.n, o.n = 1, 1, 1
    assert g(*head, 0, None, None) == -1              # sync_every < 1


# ---- the scope checks ------------------------------------------------------------------
def _fake(npix=401, ntp=977, kind='regulargrid', ndim=4, resol=None):
    from rvspecfit_amd.library import TemplateLibrary
    lib = TemplateLibrary.__new__(TemplateLibrary)
    lib.name, lib.ndim, lib.kind, lib.ntp = 'gold_b', ndim, kind, ntp
    lib.spline_factors = object()
    arm = types.SimpleNamespace(name='gold_b', G=1, resol=resol, npix=npix)
    return types.SimpleNamespace(arms=[arm]), {'gold_b': lib}


def test_scope_admits_matrices_only_with_both_keys():
    from rvspecfit_amd import engine
    batch, libs = _fake()
    msg = ("config['fused_gradient'] does not go with a resolution matrix (resol_params / "
           "the spectra's own, arm gold_b)")
    for kw in (dict(), dict(resol_gradient=False), dict(vsini_grad=True)):
        with pytest.raises(ValueError) as e:
            engine.check_fused_grad_scope(batch, libs, 5, [dict(nd=3)], **kw)
        assert str(e.value) == msg
    own, _ = _fake(resol=dict(nd=3))              # the spectra's own
    with pytest.raises(ValueError) as e:
        engine.check_fused_grad_scope(own, libs, 5)
    assert str(e.value) == msg
    assert not engine.can_fuse_objective_grad(batch, libs, [dict(nd=3)], npoly=5)
    for vg in (False, True):
        for nd in (1, 3, 11, 33):
            engine.check_fused_grad_scope(batch, libs, 10, [dict(nd=nd)], vsini_grad=vg,
                                          resol_gradient=True)
        engine.check_fused_grad_scope(own, libs, 5, vsini_grad=vg, resol_gradient=True)
    assert engine.can_fuse_objective_grad(batch, libs, [dict(nd=3)], npoly=5,
                                          resol_gradient=True)
    # without a matrix the flag changes nothing
    engine.check_fused_grad_scope(batch, libs, 5, resol_gradient=True)
    # both routes to a matrix together raise as the value does
    with pytest.raises(ValueError, match='not allowed to set resol_param'):
        engine.check_fused_grad_scope(own, libs, 5, [dict(nd=3)], resol_gradient=True)


def test_scope_refuses_by_name_with_both_keys():
    from rvspecfit_amd import engine
    batch, libs = _fake()
    kw = dict(resol_gradient=True)
    for nd in (35, 377, 4):
        with pytest.raises(ValueError) as e:
            engine.check_fused_grad_scope(batch, libs, 5, [dict(nd=nd)], **kw)
        s = str(e.value)
        assert 'fused_gradient' in s and 'resol_gradient' in s and 'gold_b' in s
        assert '%d diagonals' % nd in s and 'at most 33' in s, s
    # an arm outside the geometry: 2 npix + nd - 1 > ntp
    tight, _ = _fake(npix=473)
    engine.check_fused_grad_scope(tight, libs, 5, [dict(nd=31)], **kw)
    with pytest.raises(ValueError) as e:
        engine.check_fused_grad_scope(tight, libs, 5, [dict(nd=33)], **kw)
    s = str(e.value)
    assert 'fused_gradient' in s and 'gold_b' in s and '2 npix + nd - 1 <= ntp' in s
    assert 'npix = 473' in s and 'ntp = 977' in s and 'at most 472 pixels' in s, s
    assert not engine.can_fuse_objective_grad(tight, libs, [dict(nd=33)], npoly=5, **kw)
    # what stays refused beside the two keys
    rs = [dict(nd=3)]
    with pytest.raises(ValueError, match='fused_gradient.*Fisher'):
        engine.check_fused_grad_scope(batch, libs, 5, rs, what='the Fisher matrix', **kw)
    with pytest.raises(ValueError, match='fused_gradient.*fast_interp'):
        engine.check_fused_grad_scope(batch, libs, 5, rs, fast_interp=True, **kw)
    with pytest.raises(ValueError, match='fused_gradient.*npoly'):
        engine.check_fused_grad_scope(batch, libs, 11, rs, **kw)
    batch.arms[0].G = 2
    with pytest.raises(ValueError, match='fused_gradient.*grid set'):
        engine.check_fused_grad_scope(batch, libs, 5, rs, **kw)
    batch.arms[0].G = 1
    # a Delaunay library needs its own key, with or without a matrix
    b2, l2 = _fake(kind='triangulation')
    with pytest.raises(ValueError, match='fused_gradient.*triangulation'):
        engine.check_fused_grad_scope(b2, l2, 5, rs, **kw)
    engine.check_fused_grad_scope(b2, l2, 5, rs, tri_gradient=True, **kw)
    with pytest.raises(ValueError, match='fused_gradient.*resolution matrix'):
        engine.check_fused_grad_scope(b2, l2, 5, rs, tri_gradient=True)
    with pytest.raises(ValueError, match='35 diagonals'):
        engine.check_fused_grad_scope(b2, l2, 5, [dict(nd=35)], tri_gradient=True, **kw)
    # the Fisher kernel has no form for matrices, whatever the gradient's keys
    with pytest.raises(ValueError, match='fused_fisher.*resolution matrix'):
        engine.check_fused_fisher_scope(batch, libs, 5, rs)


# ---- the method ---------------------------------------------------------------------------
def _err(g, ref):
    return float((np.abs(g - ref) / np.maximum(np.abs(ref),
                                                1e-6 * np.abs(ref).max())).max())


def test_band_and_its_transpose(cases):
    """band() reads the matrix as the kernel's taps; band_apply is R @ x and
    band_transposed R^T @ y to rounding, at the matrix's own width and padded to 33
    diagonals"""
    sds = truth.spectra(cases, orc.SpecData)[0]
    rng = np.random.default_rng(11)
    for job in (0, 3):
        for sd, R in zip(sds, rtruth.matrices(sds, job)):
            n = len(sd.lam)
            x, y = rng.standard_normal(n), rng.standard_normal(n)
            for nd in (None, 33):
                taps = radj.band(R, nd)
                assert taps.shape == (n, nd or rtruth.ndiag(R))
                a, b = radj.band_apply(taps, x), radj.band_transposed(taps, y)
                assert np.abs(a - R @ x).max() <= 1e-14 * np.abs(x).max()
                assert np.abs(b - R.T @ y).max() <= 1e-14 * np.abs(y).max()
                assert abs(a @ y - x @ b) <= 1e-13 * np.abs(a).max() * np.abs(y).sum()


@pytest.mark.parametrize('npoly,bound', [(5, 1.3e-12), (10, 2.6e-12)])
def test_restatement_against_the_truth(cases, gold_libs, npoly, bound):
    """value and gradient on the in-cell golden jobs under the matrices of
    chisq_grad_resol_truth, with and without the vsini row, and with a matrix on one arm
    only: the red one, and the blue one arm by arm (see the module's text)"""
    sp = truth.spectra(cases, orc.SpecData)
    worst = dict(plain=0.0, vsini=0.0, one_arm=0.0, blue_only=0.0, blue_only_per_arm=0.0)
    worst_v = 0.0
    for job in truth.INSIDE:
        s, vel, par, vs = truth.JOBS[job]
        mats = rtruth.matrices(sp[s], job)
        for label, mm, fit in (('plain', mats, False), ('vsini', mats, True),
                               ('one_arm', [None, mats[1]], False),
                               ('blue_only', [mats[0], None], False)):
            if fit and not vs:
                continue
            rv, rg = rtruth.chisq_and_grad(sp[s], gold_libs, mm, vel, par, vs,
                                           npoly=npoly, vsini_fit=fit)
            val, g = radj.chisq_and_grad(sp[s], gold_libs, mm, vel, par, vs, npoly=npoly,
                                         vsini_grad=fit)
            assert g.shape == rg.shape == (6 if fit else 5, )
            e = _err(g, rg)
            ev = abs(val - rv) / max(abs(rv), 1e3)
            print('npoly %d job %d %-7s gradient error %.3g value error %.3g'
                  % (npoly, job, label, e, ev))
            worst[label] = max(worst[label], e)
            worst_v = max(worst_v, ev)
            if label == 'blue_only':
                # arm by arm: the truth of each arm alone (no cancellation between arms)
                arms = radj.chisq_and_grad(sp[s], gold_libs, mm, vel, par, vs, npoly=npoly,
                                           details=True)[2]
                for sd, R, a in zip(sp[s], mm, arms):
                    _, ga = rtruth.chisq_and_grad([sd], gold_libs, [R], vel, par, vs,
                                                  npoly=npoly)
                    ea = _err(a['grad'], ga)
                    print('npoly %d job %d blue only, arm %s alone: gradient error %.3g'
                          % (npoly, job, sd.name, ea))
                    worst['blue_only_per_arm'] = max(worst['blue_only_per_arm'], ea)
    print('npoly %d largest gradient errors %s value error %.3g (bounds %.3g, 2.6e-12)'
          % (npoly, worst, worst_v, bound))
    assert max(worst[k] for k in ('plain', 'vsini', 'one_arm', 'blue_only_per_arm')) <= bound
    assert worst_v <= 2.6e-12


# the restatement's adjoint row against autograd with the row as the leaf, relative to the
# absolute sum behind each entry (measured; the device test's bound is built from it)
RESTATED_ROW_ERR = 7.3e-13


def adjoint_row_cases(cases, gold_libs, npoly=10, t_rows=None):
    """[(job, arm number, restated arm, truth (chi, gvel, tbar, terms, cond), change of
    the restated row under one ulp of x)] of the in-cell golden jobs under the matrices of
    spectrum-width 2 s (tests/test_objective_grad_resol_gpu.py's); t_rows[(job, arm)]: the
    template rows to take in place of the restatement's own"""
    import adjoint_row_resol_truth as art
    sp = truth.spectra(cases, orc.SpecData)
    out = []
    for job in truth.INSIDE:
        s, vel, par, vs = truth.JOBS[job]
        mats = rtruth.matrices(sp[s], 2 * s)
        for ia, sd in enumerate(sp[s]):
            lib = gold_libs[sd.name]
            t = None if t_rows is None else t_rows[(job, ia)]
            a = radj.arm(sd, lib, mats[ia], vel, par, vs, npoly, t_row=t)
            b = radj.arm(sd, lib, mats[ia], vel, par, vs, npoly, t_row=t, x_ulps=1.0)
            ref = art.adjoint_row(sd, lib.lam, a['t'], np.asarray(mats[ia].todense()), vel,
                                  vs, npoly)
            out.append((job, ia, a, ref, art.row_error(b['tbar'], a['tbar'], ref[3])))
    return out


def test_restated_adjoint_row_against_autograd(cases, gold_libs):
    import adjoint_row_resol_truth as art
    worst, inf, lo, hi = 0.0, 0.0, 1.0, 0.0
    for job, ia, a, (chi, gv, want, terms, cond), moved in adjoint_row_cases(cases,
                                                                             gold_libs):
        assert cond < 100
        e = art.row_error(a['tbar'], want, terms)
        ei = np.abs(a['tbar'] - want).max() / np.abs(want).max()
        print('job %d arm %d adjoint row: error %.3g of the absolute sums (%.3g of the '
              'largest entry); one ulp of x moves it by %.3g' % (job, ia, e, ei, moved))
        assert abs(a['grad'][0] - gv) <= 2.6e-12 * abs(gv)
        worst, inf = max(worst, e), max(inf, ei)
        lo, hi = min(lo, moved), max(hi, moved)
    print('largest %.3g (%.3g of the largest entry); conditioning %.3g ... %.3g'
          % (worst, inf, lo, hi))
    assert worst <= 10 * RESTATED_ROW_ERR
    # the row moves under one ulp of x by far more than the restatement is off
    assert lo > 10 * RESTATED_ROW_ERR


def test_restatement_without_a_matrix_is_the_parent(cases, gold_libs):
    """mats of None: the numbers of objective_adjoint_restated, bit for bit; an identity
    matrix: the same"""
    import scipy.sparse
    sp = truth.spectra(cases, orc.SpecData)
    s, vel, par, vs = truth.JOBS[3]
    v0, g0 = adj.chisq_and_grad(sp[s], gold_libs, vel, par, vs, npoly=10, vsini_grad=True)
    v1, g1 = radj.chisq_and_grad(sp[s], gold_libs, [None, None], vel, par, vs, npoly=10,
                                 vsini_grad=True)
    eye = [scipy.sparse.identity(len(sd.lam), format='csr') for sd in sp[s]]
    v2, g2 = radj.chisq_and_grad(sp[s], gold_libs, eye, vel, par, vs, npoly=10,
                                 vsini_grad=True)
    assert v0 == v1 == v2 and np.array_equal(g0, g1) and np.array_equal(g0, g2)
