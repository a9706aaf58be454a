"""The fused gradient on MLP libraries without a GPU: the new entry points'
declarations against the binding, what they refuse before any launch, the host
arithmetic of their _ok / work-size functions, the opt-in of the scope check -- and the
yardsticks of the GPU tests: the float32 reverse pass restated in torch (reverse32)
against the float64 truth (vjp64), and the adjoint method's tbar at a GIVEN template row
against autograd with the row as the leaf.

Measured here (B = 27, tbar from template_adjoint_truth on the 129-pixel fixture of
tests/test_nn_vjp_gpu.py; metric |got - want| / sum_n |tbar_n jac64[k, n]|):
    reverse32 against vjp64: 4 -> 64^3 -> 40 -> 333: 2.51e-07; its 39-wide cut: 2.22e-07
    the restatement's tbar against autograd, relative to |tbar|_inf: 1.5e-14 (npoly 5),
    1.6e-14 (npoly 10); with a fixed vsini of 380 km/s 5.3e-15 and 6.5e-15
The GPU bound of rvs_template_nn_vjp is 4 x the first figure at the test's own points
(the rule of DESIGN 4.16)."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import nn_grad_truth as nt
import nn_vjp_truth as vt
import objective_adjoint_restated as adj

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    'rvs_objective_grad_from_template_ok': 'int npoly, int npix, int ntp, int vsini_grad',
    'rvs_objective_grad_from_template_work_size': 'int J, int narm, int vsini_grad',
    'rvs_objective_grad_from_template':
        'const rvs_objective_arm *arms, int narm, int npoly, int vsini_grad, '
        'const double *const *templ, const double *const *outside, const double *vsini, '
        'const int32_t *job_spec, int J, const double *vel, double badchi, '
        'const double *basis_const, void *scratch, double *const *tbar, double *out, '
        'double *grad, int32_t *status, void *stream',
    'rvs_objective_grad_join':
        'int narm, int J, int ndim, int vsini_grad, const void *scratch, '
        'const double *const *gparams, const double *out, const double *grad_vv, '
        'double *grad, void *stream',
    'rvs_template_nn_vjp_work_size': 'int B, int nlayer, const int32_t *dims',
    'rvs_bfgs_run_grad_fused_nn':
        'const rvs_bfgs_state *b, const rvs_nm_objective *o, const rvs_grad_chain *g, '
        'const rvs_objective_arm *garms, const double *basis_const, void *gwork, '
        'double *const *tbar, void *const *vjp_work, double *const *gparams, '
        'double *grad_vv, int sync_every, int64_t *stats, void *stream',
    'rvs_template_nn_vjp':
        'const double *params, int B, int ndim, uint32_t log_mask, const double *M, '
        'const double *S, int nlayer, const float *const *W, const float *const *b, '
        'const int32_t *dims, const double *templ, const double *tbar, void *work, '
        'double *gparams, void *stream',
}
LAM = np.exp(np.linspace(np.log(3950.), np.log(5060.), 333))
NPIX = 129
VEL = [12.5, -83.0, 140.25]


def _norm(decl):
    return ' '.join(decl.replace('*', ' * ').split())


# ---- 1. the boundary ----------------------------------------------------------------------
def test_symbols_and_signatures():
    """declared as DESIGN 4.25 states them, bound with matching ctypes lists, exported;
    the ABI number did not move"""
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
                  'uint32_t': ctypes.c_uint32}[a.split()[0]] for a in got]
        res, args = _lib.SIGNATURES[name]
        assert args == kinds, name
        assert res is (ctypes.c_int64 if m.group(1) == 'int64_t' else ctypes.c_int)
        assert hasattr(L, name)


def test_from_template_ok_is_the_geometry_rule_without_ndim():
    from rvspecfit_amd import _lib
    L = _lib.lib()
    ok, gok = L.rvs_objective_grad_from_template_ok, L.rvs_objective_grad_ok
    for npoly in (0, 1, 5, 10, 11):
        for npix, ntp in [(2751, 6215), (2881, 6449), (129, 333), (1000, 333), (16, 32),
                          (17, 32), (10, 31), (3000, 8000), (0, 333)]:
            for vg in (-1, 0, 1, 2):
                want = int(1 <= npoly <= 10 and npix >= 1 and ntp >= 32 and
                           2 * npix <= ntp and 3 * ntp * 8 + 8192 <= 160 * 1024 and
                           vg in (0, 1))
                assert ok(npoly, npix, ntp, vg) == want, (npoly, npix, ntp, vg)
                for nd in (1, 4):      # rvs_objective_grad_ok inside its ndim bound
                    assert gok(npoly, npix, ntp, nd, vg) == want


def test_work_sizes():
    from rvspecfit_amd import _lib
    L = _lib.lib()
    ws = L.rvs_objective_grad_from_template_work_size
    assert ws(100, 3, 0) == 3 * 100 * 4 * 8 and ws(100, 3, 1) == 3 * 100 * 5 * 8
    for bad in ((0, 1, 0), (10, 0, 0), (10, 5, 0), (10, 1, 2), (10, 1, -1)):
        assert ws(*bad) == 0, bad
    vs = L.rvs_template_nn_vjp_work_size

    def dims(*d):
        return ctypes.cast((ctypes.c_int32 * len(d))(*d), ctypes.c_void_p)
    # the jobs' exponents (int32, padded to 8 bytes), then [B][runs of 256 pixels][K_L]
    assert vs(27, 5, dims(4, 64, 64, 64, 40, 333)) == 8 * 14 + 27 * 2 * 40 * 4
    assert vs(8192, 5, dims(4, 256, 256, 256, 200, 6215)) == 4 * 8192 + 8192 * 25 * 200 * 4
    assert vs(1, 5, dims(4, 64, 64, 64, 39, 256)) == 8 + 39 * 4
    assert vs(0, 5, dims(4, 64, 64, 64, 40, 333)) == 0
    assert vs(27, 5, dims(4, 64, 48, 64, 40, 333)) == 0       # a hidden width of 48
    assert vs(27, 2, dims(4, 64, 333)) == 0                   # two layers
    assert vs(27, 3, dims(7, 64, 64, 333)) == 0               # ndim = 7
    assert vs(27, 5, None) == 0


def _vjp_call(dims, ndim=None, B=3, null=None):
    from rvspecfit_amd import _lib
    L = _lib.lib()
    a = ctypes.c_void_p(64)       # never dereferenced
    nl = len(dims) - 1
    Wp = (ctypes.c_void_p * nl)(*[None if null == 'W' else 64] * nl)
    bp = (ctypes.c_void_p * nl)(*[64] * nl)
    dm = (ctypes.c_int32 * (nl + 1))(*dims)
    args = dict(params=a, M=a, S=a, templ=a, tbar=a, work=a, gparams=a)
    if null in args:
        args[null] = None
    return L.rvs_template_nn_vjp(args['params'], B, dims[0] if ndim is None else ndim, 1,
                                 args['M'], args['S'], nl,
                                 ctypes.cast(Wp, ctypes.c_void_p),
                                 ctypes.cast(bp, ctypes.c_void_p),
                                 ctypes.cast(dm, ctypes.c_void_p), args['templ'],
                                 args['tbar'], args['work'], args['gparams'], None)


def test_vjp_refuses_before_any_launch():
    """RVS_E_ARG (-1) for everything outside rvs_template_nn_grad's scope and for NULL
    arrays: no device is touched (there is none here)"""
    assert _vjp_call([4, 64, 48, 64, 40, 333]) == -1
    assert _vjp_call([4, 48, 64, 40, 333]) == -1
    assert _vjp_call([7, 64, 64, 40, 333]) == -1
    assert _vjp_call([4, 64, 333]) == -1
    assert _vjp_call([4] + [64] * 7 + [333]) == -1
    assert _vjp_call([4, 64, 288, 40, 333]) == -1
    assert _vjp_call([4, 64, 64, 40, 333], ndim=3) == -1
    assert _vjp_call([4, 64, 64, 40, 333], B=0) == -1
    for null in ('W', 'params', 'M', 'S', 'templ', 'tbar', 'work', 'gparams'):
        assert _vjp_call([4, 64, 64, 40, 333], null=null) == -1, null


def test_from_template_and_join_refuse_before_any_launch():
    from rvspecfit_amd import _lib
    L = _lib.lib()
    a = ctypes.c_void_p(64)
    f = L.rvs_objective_grad_from_template
    arr = (_lib.ObjectiveArm * 1)()
    arr[0].ndim, arr[0].ntp = 6, 333            # (ndim is not read: no cell record)
    arr[0].pt.npix, arr[0].pt.ntp = 129, 333
    arr[0].factors = 64
    rows = ctypes.cast((ctypes.c_void_p * 1)(64), ctypes.c_void_p)
    nullrow = ctypes.cast((ctypes.c_void_p * 1)(None), ctypes.c_void_p)
    names = ['arms', 'narm', 'npoly', 'vsini_grad', 'templ', 'outside', 'vsini',
             'job_spec', 'J', 'vel', 'badchi', 'basis_const', 'scratch', 'tbar', 'out',
             'grad', 'status', 'stream']
    good = [ctypes.addressof(arr), 1, 5, 0, rows, rows, None, None, 1, a, 1.0, None, a,
            rows, a, a, a, None]

    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[names.index(k)] = v
        return f(*args)
    assert call(J=0) == -1 and call(arms=None) == -1
    assert call(narm=0) == -1 and call(narm=5) == -1
    assert call(npoly=0) == -1 and call(npoly=11) == -1
    assert call(vsini_grad=2) == -1 and call(vsini_grad=-1) == -1
    assert call(vsini_grad=1) == -1                 # vsini fitted without vsini
    for k in ('templ', 'outside', 'tbar', 'vel', 'scratch', 'out', 'grad', 'status'):
        assert call(**{k: None}) == -1, k
    for k in ('templ', 'outside', 'tbar'):
        assert call(**{k: nullrow}) == -1, k
    arr[0].pt.npix = 1000                           # 2 npix > ntp
    assert call() == -1
    arr[0].pt.npix = 129
    for fld, val, back in (('fast_interp', 1, 0), ('taps', 64, None), ('G', 2, 0)):
        setattr(arr[0].pt, fld, val)
        assert call() == -1, fld
        setattr(arr[0].pt, fld, back)
    arr[0].factors = None
    assert call() == -1
    g = L.rvs_objective_grad_join
    good = [1, 3, 4, 0, a, rows, a, a, a, None]
    assert g(*good[:0] + [0] + good[1:]) == -1 and g(*good[:0] + [5] + good[1:]) == -1
    assert g(1, 0, 4, 0, a, rows, a, a, a, None) == -1
    assert g(1, 3, 0, 0, a, rows, a, a, a, None) == -1
    assert g(1, 3, 9, 0, a, rows, a, a, a, None) == -1
    assert g(1, 3, 4, 2, a, rows, a, a, a, None) == -1
    assert g(1, 3, 4, 0, None, rows, a, a, a, None) == -1
    assert g(1, 3, 4, 0, a, None, a, a, a, None) == -1
    assert g(1, 3, 4, 0, a, nullrow, a, a, a, None) == -1
    for i in (6, 7, 8):
        args = list(good)
        args[i] = None
        assert g(*args) == -1, i


def test_rounds_refuse_before_any_launch():
    """rvs_bfgs_run_grad_fused_nn: NULL and empty descriptors, sync_every < 1, an objective
    without MLP arms -- RVS_E_ARG, as rvs_bfgs_run_grad_fused answers them"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    a = ctypes.c_void_p(64)
    f = L.rvs_bfgs_run_grad_fused_nn
    assert f(None, None, None, None, None, None, None, None, None, None, 1, None,
             None) == -1
    b, o, gc = _lib.BfgsState(), _lib.NmObjective(), _lib.GradChain()
    arr = (_lib.ObjectiveArm * 1)()
    rows = ctypes.cast((ctypes.c_void_p * 1)(64), ctypes.c_void_p)
    args = [ctypes.addressof(b), ctypes.addressof(o), ctypes.addressof(gc),
            ctypes.addressof(arr), None, a, rows, rows, rows, a]
    assert f(*args, 1, None, None) == -1              # empty descriptors
    b.S, b.n, o.n = 1, 1, 1
    assert f(*args, 0, None, None) == -1              # sync_every < 1
    for fld in ('runs', 'x0', 'x', 'fun', 'nit', 'nfev', 'status', 'nreq', 'off', 'list',
                'X', 'F', 'counts'):
        setattr(b, fld, 64)
    gc.njev, gc.chi, gc.grad = 64, 64, 64
    gc.cap, gc.narm, gc.ntan, o.narm, o.ndim = 4, 1, 4, 1, 4
    assert f(*args, 1, None, None) == -1              # no row buffers, no MLP arms (o->nn)


# ---- 2. the opt-in of the scope check ---------------------------------------------------
def _fake(npix=NPIX, ntp=333, dims=(4, 64, 64, 64, 40, 333), kind='nn'):
    from rvspecfit_amd.library import TemplateLibrary
    lib = TemplateLibrary.__new__(TemplateLibrary)
    lib.name, lib.ndim, lib.kind, lib.ntp = 'aat_580v', dims[0], kind, ntp
    lib.nn_dims = np.array(dims, dtype=np.int32)
    lib.spline_factors = object()
    arm = types.SimpleNamespace(name='aat_580v', G=1, resol=None, npix=npix)
    return types.SimpleNamespace(arms=[arm]), {'aat_580v': lib}


def test_scope_check_admits_mlp_libraries_only_with_both_keys():
    from rvspecfit_amd import engine
    batch, libs = _fake()
    # without nn_gradient the refusal stays word for word
    msg = ("config['fused_gradient'] needs regular-grid (polylinear) libraries: "
           'aat_580v is a nn library (interpolation_type)')
    for kw in (dict(), dict(nn_gradient=False), dict(vsini_grad=True)):
        with pytest.raises(ValueError) as e:
            engine.check_fused_grad_scope(batch, libs, 5, **kw)
        assert str(e.value) == msg
    assert not engine.can_fuse_objective_grad(batch, libs, npoly=5)
    for vg in (False, True):
        engine.check_fused_grad_scope(batch, libs, 5, vsini_grad=vg, nn_gradient=True)
        engine.check_fused_grad_scope(batch, libs, 10, vsini_grad=vg, nn_gradient=True)
    # the other refusals stay, with nn_gradient too
    with pytest.raises(ValueError, match='fused_gradient.*Fisher'):
        engine.check_fused_grad_scope(batch, libs, 5, what='the Fisher matrix',
                                      nn_gradient=True)
    with pytest.raises(ValueError, match='fused_gradient.*fast_interp'):
        engine.check_fused_grad_scope(batch, libs, 5, fast_interp=True, nn_gradient=True)
    with pytest.raises(ValueError, match='fused_gradient.*npoly'):
        engine.check_fused_grad_scope(batch, libs, 11, nn_gradient=True)
    with pytest.raises(ValueError, match='fused_gradient.*resolution matrix'):
        engine.check_fused_grad_scope(batch, libs, 5, resols=[dict(nd=3)],
                                      nn_gradient=True)
    batch.arms[0].G = 2
    with pytest.raises(ValueError, match='fused_gradient.*grid set'):
        engine.check_fused_grad_scope(batch, libs, 5, nn_gradient=True)
    batch.arms[0].G = 1
    # a Delaunay library keeps the chain; a network outside rvs_template_nn_grad's scope
    b2, l2 = _fake(kind='triangulation')
    with pytest.raises(ValueError, match='fused_gradient.*triangulation'):
        engine.check_fused_grad_scope(b2, l2, 5, nn_gradient=True)
    b3, l3 = _fake(dims=(4, 64, 48, 64, 40, 333))
    with pytest.raises(ValueError, match='multiple of 32'):
        engine.check_fused_grad_scope(b3, l3, 5, nn_gradient=True)


def test_geometry_refusal_on_an_mlp_arm_names_the_nn_library():
    """npix = 1000 on ntp = 333 (the case tests/test_objective_grad_gpu.py raises on):
    2 npix > ntp"""
    from rvspecfit_amd import engine
    batch, libs = _fake(npix=1000)
    with pytest.raises(ValueError) as e:
        engine.check_fused_grad_scope(batch, libs, 5, nn_gradient=True)
    assert 'fused_gradient' in str(e.value) and 'nn library' in str(e.value)
    assert 'geometry' in str(e.value)


# ---- 3. the yardsticks ---------------------------------------------------------------------
def fixture_spectra(net, S=3, seed=5):
    """S noisy spectra of the network's own templates on 129 pixels (4000-5000 A): the
    fixture of tests/test_nn_grad_gpu.py with 2 npix <= 333; [(wave, spec, espec)]"""
    rng = np.random.RandomState(seed)
    wave = np.linspace(4000., 5000., NPIX)
    par = nt.points(net, S, seed=6)
    t = nt.jacobian64(net, par)[0]
    out = []
    for s in range(S):
        f = np.sqrt((1 - VEL[s] / nt.C_KMS) / (1 + VEL[s] / nt.C_KMS))
        m = np.interp(wave * f, LAM, t[s]) * (1.0 + 0.1 * (wave - 4500.) / 500.)
        e = np.full(NPIX, 0.02)
        out.append((wave, m + e * rng.normal(size=NPIX), e))
    return out


def adjoint_rows(net, p, npoly=5, vsini=None):
    """tbar [B, ntp] from template_adjoint_truth: job j against spectrum j % 3 at the
    float64 network's template of p[j]"""
    sp = fixture_spectra(net)
    t = nt.jacobian64(net, p)[0]
    rows = []
    for j in range(len(p)):
        w, d, e = sp[j % 3]
        rows.append(vt.template_adjoint_truth(w, d, e, LAM, t[j], VEL[j % 3], vsini,
                                              npoly)[2])
    return t, np.array(rows)


def _cut39(net):
    W, b = list(net['W']), list(net['b'])
    W[-2], b[-2], W[-1] = W[-2][:39].copy(), b[-2][:39].copy(), W[-1][:, :39].copy()
    dims = np.array(net['dims'], dtype=np.int32)
    dims[-2] = 39
    return dict(net, W=W, b=b, dims=dims)


@pytest.mark.parametrize('which', ['k40', 'k39'])
def test_reverse32_against_vjp64(which):
    """what float32 arithmetic alone loses in the reverse pass, in the metric the GPU
    test uses; the GPU bound derives from this figure.  The bound here, 1e-6, is the
    float32 unit roundoff 6e-8 times a handful of layers: reasoning, not the measurement."""
    net = nt.network()
    net = _cut39(net) if which == 'k39' else net
    B = 27
    p = nt.points(net, B, seed=B, shrink=0.1)
    _, tbar = adjoint_rows(net, p)
    want, scale = vt.vjp64(net, p, tbar)
    # (the value rows of the float32 network, as the device's are: forward32's)
    t = nt.forward32(net, p)[0]
    got = vt.reverse32(net, p, t, tbar)
    m = vt.vjp_metric(got, want, scale)
    print('%s: reverse32 against vjp64, largest |got - want| / sum |tbar jac| = %.3g '
          '(job %d)' % (which, m.max(), int(m.max(axis=1).argmax())))
    assert got.shape == (B, nt.NDIM) and np.isfinite(got).all()
    assert m.max() <= 1e-6
    # exact properties of the statement itself: the power of two, the flat clip
    g2 = vt.reverse32(net, p, t, np.ldexp(tbar, 100))
    assert np.array_equal(g2, np.ldexp(got, 100))
    tc = t.copy()
    tc[:, 7] = np.exp(300.0)
    tb2 = tbar.copy()
    tb2[:, 7] = 0.0
    assert np.array_equal(vt.reverse32(net, p, tc, tbar), vt.reverse32(net, p, t, tb2))
    assert not vt.reverse32(net, p, t, np.zeros_like(tbar)).any()


@pytest.mark.parametrize('npoly', [5, 10])
@pytest.mark.parametrize('vsini', [None, 380.0])
def test_restatement_tbar_at_a_given_row(npoly, vsini):
    """tests/objective_adjoint_restated.py fed with a GIVEN template row (a library that
    answers with it): its tbar against autograd with the row as the leaf, relative to
    |tbar|_inf; value and velocity component beside it.  Bound 1e-12: float64's 1.1e-16
    times the conditioning of the fixture (cond(A) < 100) times a hundred roundings per
    knot (two tridiagonal sweeps, the FIR, the pixels of two intervals)."""
    net = nt.network()
    p = nt.points(net, 3, seed=6, shrink=0.1)
    t = nt.jacobian64(net, p)[0]
    sp = fixture_spectra(net)
    worst = 0.0
    for s in range(3):
        w, d, e = sp[s]
        lib = types.SimpleNamespace(ndim=0, lam=LAM, log_ids=(),
                                    outside_flag=lambda q: 1.0, eval=lambda q, r=t[s]: r)
        sd = types.SimpleNamespace(lam=w, spec=d, espec=e, name='x')
        a = adj.arm(sd, lib, VEL[s], np.zeros(0), vsini, npoly)
        chi, gvel, tbar, cond = vt.template_adjoint_truth(w, d, e, LAM, t[s], VEL[s],
                                                          vsini, npoly)
        assert cond < 100
        err = np.abs(a['tbar'] - tbar).max() / np.abs(tbar).max()
        worst = max(worst, err)
        assert abs(a['value'] - chi) <= 1e-11 * max(abs(chi), 1e3)
        assert abs(a['grad'][0] - gvel) <= 1e-9 * abs(gvel)
    print('npoly %d vsini %s: restatement tbar against autograd %.3g of |tbar|_inf'
          % (npoly, vsini, worst))
    assert worst <= 1e-12
