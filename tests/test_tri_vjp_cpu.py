"""The fused gradient on Delaunay libraries without a GPU: the two new
entry points' declarations against the binding, what they refuse before any launch, the
opt-in of the scope check (config['tri_gradient'] beside config['fused_gradient']) -- and
the yardstick of the GPU tests: the per-element contraction restated in float64 numpy
against the long-double contraction of tri_grad_truth.template_jacobian
(tests/tri_vjp_truth.py).

Figures (golden libraries, JOBS[0..5], adjoint rows of random sign over 12 decades; metric
|g - truth| / sum_n |tbar_n dt_n/dp_k|): per-element form 1.98e-16 to 6.89e-16, depending
on the order in which numpy adds up, the vertex-dot form 6.71e-15.  The device is held to
VJP_REL_BOUND = 10 x the first figure, computed at the test's own points; 6.6e-16 was
measured on an MI355X."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import tri_vjp_truth as tv

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {
    'rvs_template_tri_vjp':
        'const double *dats, int ntp, const int32_t *simplices, const double *transform, '
        'int nsimplex, int ndim, uint32_t log_mask, int exp_flag, const double *params, '
        'int B, const int32_t *simplex, const double *templ, const double *tbar, '
        'double *gparams, void *stream',
    'rvs_bfgs_run_grad_fused_tri':
        'const rvs_bfgs_state *b, const rvs_nm_objective *o, const rvs_grad_chain *g, '
        'const rvs_objective_arm *garms, const double *basis_const, void *gwork, '
        'double *const *tbar, double *const *gparams, double *grad_vv, int sync_every, '
        'int64_t *stats, void *stream',
}
MSG = ("config['fused_gradient'] needs regular-grid (polylinear) libraries: %s is a "
       'triangulation library (interpolation_type)')


def _norm(decl):
    return ' '.join(decl.replace('*', ' * ').split())


# ---- 1. the boundary ----------------------------------------------------------------------
def test_symbols_and_signatures():
    """declared as DESIGN 4.26 states them, bound with matching ctypes lists, exported; the
    ABI number did not move and the version comment names both"""
    from rvspecfit_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
    head = hdr[:hdr.index('#define RVS_ABI_VERSION')]
    txt = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    L = _lib.lib()
    assert L.rvs_abi_version() == 18
    for name, want in NEW.items():
        assert name in head, name + ' is not in the version comment'
        m = re.search(r'\b(int|int64_t)\s+%s\s*\(([^;]*?)\)\s*;' % name, txt, flags=re.S)
        assert m, name + ' is not declared'
        got = [_norm(a) for a in m.group(2).split(',')]
        assert got == [_norm(a) for a in want.split(',')], name
        kinds = [ctypes.c_void_p if '*' in a else
                 {'int': ctypes.c_int, 'double': ctypes.c_double,
                  'uint32_t': ctypes.c_uint32}[a.split()[0]] for a in got]
        res, args = _lib.SIGNATURES[name]
        assert args == kinds, name
        assert res is ctypes.c_int
        assert hasattr(L, name)


def _vjp_call(ndim=4, ntp=977, nsimplex=10, B=3, null=None):
    from rvspecfit_amd import _lib
    a = ctypes.c_void_p(64)       # never dereferenced
    v = dict(dats=a, simplices=a, transform=a, params=a, simplex=a, templ=a, tbar=a,
             gparams=a)
    if null is not None:
        v[null] = None
    return _lib.lib().rvs_template_tri_vjp(
        v['dats'], ntp, v['simplices'], v['transform'], nsimplex, ndim, 1, 1, v['params'],
        B, v['simplex'], v['templ'], v['tbar'], v['gparams'], None)


def test_vjp_refuses_before_any_launch():
    """RVS_E_ARG (-1) for ndim outside 1..6, ntp < 1, B < 0 and NULL arrays; B == 0 is an
    empty call: no device is touched (there is none here)"""
    for nd in (0, 7, -1):
        assert _vjp_call(ndim=nd) == -1, nd
    assert _vjp_call(ntp=0) == -1 and _vjp_call(B=-1) == -1
    assert _vjp_call(nsimplex=0) == -1
    for null in ('dats', 'simplices', 'transform', 'params', 'simplex', 'templ', 'tbar',
                 'gparams'):
        assert _vjp_call(null=null) == -1, null
        assert _vjp_call(null=null, B=0) == -1, null
    for nd in (1, 6):
        assert _vjp_call(ndim=nd, B=0) == 0


def test_rounds_refuse_before_any_launch():
    """rvs_bfgs_run_grad_fused_tri: NULL and empty descriptors, sync_every < 1, an objective
    without Delaunay arms, arms without row buffers, ndim = 7 -- RVS_E_ARG, as
    rvs_bfgs_run_grad_fused_nn answers them"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    a = ctypes.c_void_p(64)
    f = L.rvs_bfgs_run_grad_fused_tri
    assert f(None, None, None, None, None, None, None, None, None, 1, None, None) == -1
    b, o, gc = _lib.BfgsState(), _lib.NmObjective(), _lib.GradChain()
    arr = (_lib.ObjectiveArm * 1)()
    rows = ctypes.cast((ctypes.c_void_p * 1)(64), ctypes.c_void_p)
    args = [ctypes.addressof(b), ctypes.addressof(o), ctypes.addressof(gc),
            ctypes.addressof(arr), None, a, rows, rows, a]
    assert f(*args, 1, None, None) == -1              # empty descriptors
    b.S, b.n, o.n = 1, 5, 5
    for fld in ('runs', 'x0', 'x', 'fun', 'nit', 'nfev', 'status', 'nreq', 'off', 'list',
                'X', 'F', 'counts'):
        setattr(b, fld, 64)
    gc.njev, gc.chi, gc.grad = 64, 64, 64
    gc.cap, gc.narm, gc.ntan, o.narm, o.ndim, o.npoly = 4, 1, 4, 1, 4, 5
    gc.vsini_mode, o.vsini_col = 0, -1
    for fld in ('vel', 'params', 'extra', 'bad', 'job_spec', 'jstatus', 'status', 'fixed',
                'safe'):
        setattr(o, fld, 64)
    arr[0].ndim, arr[0].ntp, arr[0].pt.npix, arr[0].pt.ntp = 4, 977, 300, 977
    assert f(*args, 0, None, None) == -1              # sync_every < 1
    assert f(*args, 1, None, None) == -1              # no Delaunay arms (o->tri)
    tri = (_lib.NmTriArm * 1)()
    o.tri = ctypes.addressof(tri)
    assert f(*args, 1, None, None) == -1              # an arm without anything
    for fld in ('dats', 'transform', 'extraflags', 'simplices', 'templ', 'outside',
                'simplex'):
        setattr(tri[0], fld, 64)
    tri[0].buckets.cell_start, tri[0].buckets.cell_list = 64, 64
    tri[0].ntp, tri[0].nsimplex = 977, 10
    for fld in ('templ', 'outside', 'simplex'):       # a missing row buffer
        setattr(tri[0], fld, None)
        assert f(*args, 1, None, None) == -1, fld
        setattr(tri[0], fld, 64)
    tri[0].buckets.cell_start = None                  # no bucket grid
    assert f(*args, 1, None, None) == -1
    tri[0].buckets.cell_start = 64
    for fld, val, back in (('fast_interp', 1, 0), ('taps', 64, None), ('G', 2, 0)):
        setattr(arr[0].pt, fld, val)                  # what rvs_internal_arm_plain refuses
        assert f(*args, 1, None, None) == -1, fld
        setattr(arr[0].pt, fld, back)
    arr[0].pt.npix = 1000                             # 2 npix > ntp: the kernel's geometry
    assert f(*args, 1, None, None) == -1
    arr[0].pt.npix = 300
    o.ndim, gc.ntan = 7, 7                            # ndim = 7
    assert f(*args, 1, None, None) == -1
    o.ndim, gc.ntan = 4, 4
    nullrow = ctypes.cast((ctypes.c_void_p * 1)(None), ctypes.c_void_p)
    for i in (6, 7):                                  # tbar[0], gparams[0] NULL
        bad = list(args)
        bad[i] = nullrow
        assert f(*bad, 1, None, None) == -1, i
    for i in (5, 6, 7, 8):                            # gwork, tbar, gparams, grad_vv
        bad = list(args)
        bad[i] = None
        assert f(*bad, 1, None, None) == -1, i


# ---- 2. the opt-in of the scope check ---------------------------------------------------
def _lib_of(kind, name, ndim=4, ntp=977):
    from rvspecfit_amd.library import TemplateLibrary
    lib = TemplateLibrary.__new__(TemplateLibrary)
    lib.name, lib.ndim, lib.kind, lib.ntp = name, ndim, kind, ntp
    lib.nn_dims = np.array((ndim, 64, 64, 64, 40, ntp), dtype=np.int32)
    lib.spline_factors = object()
    return lib


def _fake(kinds=('triangulation', 'triangulation'), npix=300, ndim=4):
    names = ['gold_b', 'gold_r'][:len(kinds)]
    arms = [types.SimpleNamespace(name=n, G=1, resol=None, npix=npix) for n in names]
    return (types.SimpleNamespace(arms=arms),
            {n: _lib_of(k, n, ndim) for n, k in zip(names, kinds)})


def test_scope_check_admits_delaunay_libraries_only_with_both_keys():
    from rvspecfit_amd import engine
    batch, libs = _fake()
    # without tri_gradient the refusal stays word for word, with nn_gradient too
    for kw in (dict(), dict(tri_gradient=False), dict(vsini_grad=True),
               dict(nn_gradient=True), dict(nn_gradient=True, vsini_grad=True)):
        with pytest.raises(ValueError) as e:
            engine.check_fused_grad_scope(batch, libs, 5, **kw)
        assert str(e.value) == MSG % 'gold_b'
        with pytest.raises(ValueError, match='fused_gradient.*triangulation'):
            engine.check_fused_grad_scope(batch, libs, 5, **kw)
    assert not engine.can_fuse_objective_grad(batch, libs, npoly=5)
    assert not engine.can_fuse_objective_grad(batch, libs, npoly=5, nn_gradient=True)
    for vg in (False, True):
        for npoly in (5, 10):
            for nn in (False, True):
                engine.check_fused_grad_scope(batch, libs, npoly, vsini_grad=vg,
                                              tri_gradient=True, nn_gradient=nn)
                assert engine.can_fuse_objective_grad(batch, libs, npoly=npoly,
                                                      vsini_grad=vg, tri_gradient=True)
    # the other refusals stay, in their wording, with tri_gradient too
    with pytest.raises(ValueError) as e:
        engine.check_fused_grad_scope(batch, libs, 5, what='the Fisher matrix',
                                      tri_gradient=True)
    assert str(e.value) == ("config['fused_gradient'] does not go with the Fisher matrix: "
                            'it needs the tangent rows of the gradient chain, which the '
                            'fused kernel never forms')
    with pytest.raises(ValueError, match='fused_gradient.*second_minimizer_lm'):
        engine.check_fused_grad_scope(batch, libs, 5, tri_gradient=True,
                                      what="config['second_minimizer_lm']")
    with pytest.raises(ValueError, match='fused_gradient.*process_epochs'):
        engine.check_fused_grad_scope(batch, libs, 5, tri_gradient=True,
                                      what='the joint fit (process_epochs)')
    with pytest.raises(ValueError, match=r"fused_gradient'\] does not go with fast_interp"):
        engine.check_fused_grad_scope(batch, libs, 5, fast_interp=True, tri_gradient=True)
    with pytest.raises(ValueError, match=r'takes npoly 1\.\.10, not npoly = 11'):
        engine.check_fused_grad_scope(batch, libs, 11, tri_gradient=True)
    with pytest.raises(ValueError, match='fused_gradient.*does not go with a resolution '
                                         'matrix'):
        engine.check_fused_grad_scope(batch, libs, 5, resols=[dict(nd=3), None],
                                      tri_gradient=True)
    batch.arms[1].G = 2
    with pytest.raises(ValueError, match='fused_gradient.*grid set: arm gold_r has 2'):
        engine.check_fused_grad_scope(batch, libs, 5, tri_gradient=True)
    batch.arms[1].G = 1
    libs['gold_r'].spline_factors = None
    with pytest.raises(ValueError, match=r'needs a \(log-\)uniform template grid '
                                         r'\(arm gold_r\)'):
        engine.check_fused_grad_scope(batch, libs, 5, tri_gradient=True)


def test_mixed_kinds_ndim_and_geometry_are_refused():
    from rvspecfit_amd import engine
    for other in ('regulargrid', 'nn'):
        for kinds, arm in ((('triangulation', other), 'gold_r'),
                           ((other, 'triangulation'), 'gold_b')):
            batch, libs = _fake(kinds)
            with pytest.raises(ValueError) as e:
                engine.check_fused_grad_scope(batch, libs, 5, tri_gradient=True,
                                              nn_gradient=True)
            assert 'fused_gradient' in str(e.value) and 'tri_gradient' in str(e.value)
            assert '%s is a %s library' % (arm, other) in str(e.value)
            assert not engine.can_fuse_objective_grad(batch, libs, npoly=5,
                                                      tri_gradient=True, nn_gradient=True)
    batch, libs = _fake(ndim=7)
    with pytest.raises(ValueError, match='fused_gradient.*up to 6 parameters, gold_b has '
                                         'ndim = 7'):
        engine.check_fused_grad_scope(batch, libs, 5, tri_gradient=True)
    batch, libs = _fake(ndim=6)
    engine.check_fused_grad_scope(batch, libs, 5, tri_gradient=True)
    batch, libs = _fake(npix=1000)          # 2 npix > ntp
    with pytest.raises(ValueError) as e:
        engine.check_fused_grad_scope(batch, libs, 5, tri_gradient=True)
    assert 'fused_gradient' in str(e.value) and 'triangulation library' in str(e.value)
    assert 'geometry' in str(e.value)
    # alone the key changes nothing: regular-grid libraries are judged as before
    batch, libs = _fake(('regulargrid', 'regulargrid'))
    engine.check_fused_grad_scope(batch, libs, 5, tri_gradient=True)
    batch, libs = _fake(('regulargrid', 'regulargrid'), ndim=5)
    with pytest.raises(ValueError, match='up to 4 parameters'):
        engine.check_fused_grad_scope(batch, libs, 5, tri_gradient=True)


# ---- 3. the yardstick ------------------------------------------------------------------------
def test_per_element_restatement_against_the_long_double_truth():
    """the per-element contraction in float64 numpy on both golden libraries at
    JOBS[0..5] against the long-double contraction of template_jacobian, relative to
    sum_n |tbar_n dt_n/dp_k|: below 1e-15 (a dozen roundings of 1.1e-16 per knot against
    the absolute sum; the sum over n adds none in this metric beyond its own log2(ntp)
    pairwise levels); the figure is VJP_REL_CPU, which the device's bound derives from.
    The vertex-dot order, beside it, loses more than a digit."""
    fig = tv.golden_figures(tv.per_element)
    dot = tv.golden_figures(tv.vertex_dot)
    assert fig.shape == (12, 4) and np.isfinite(fig).all()
    print('per-element form: largest %.3g (case %d); vertex-dot form: largest %.3g'
          % (fig.max(), int(fig.max(axis=1).argmax()), dot.max()))
    assert fig.max() == tv.vjp_rel_cpu()
    assert tv.vjp_rel_cpu() < 1e-15
    assert tv.vjp_rel_bound() == 10 * tv.vjp_rel_cpu()
    assert dot.max() > 3 * fig.max()
    # the statement's own exact properties: the power of two, the zero row, no simplex
    olibs, cs = tv.golden_cases()
    n, j, p, t, tb, w, s = cs[0]
    g = tv.per_element(olibs[n], p, t, tb)
    assert np.array_equal(tv.per_element(olibs[n], p, t, np.ldexp(tb, 100)),
                          np.ldexp(g, 100))
    assert not tv.per_element(olibs[n], p, t, np.zeros_like(tb)).any()
    import tri_grad_truth as ttruth
    for jj in (ttruth.NO_SIMPLEX, ttruth.NONFINITE):
        assert not tv.per_element(olibs[n], ttruth.JOBS[jj][2], t, tb).any()
