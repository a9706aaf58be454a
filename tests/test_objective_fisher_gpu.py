"""rvs_objective_fisher (csrc/objective_fisher.hip, DESIGN 4.23: value, gradient and
Fisher matrix in one forward-mode kernel per (job, arm)) and the interfaces above it --
against the float64 truths (tests/chisq_fisher_truth.py: autograd Jacobian, QR
projection, with the vsini column of tests/objective_fisher_restated.py;
tests/chisq_grad_truth.py, vsini_grad_truth.py), against the chain
(engine.chisq_point_fisher through spec_fit.chisq_fisher_jobs) and against
rvs_objective_grad.

Bounds, none of them from what this kernel measures: the Fisher matrix within
test_chisq_fisher_gpu.BOUND = 5.84e-12 of sqrt(G_ii G_ll), G = J^T J the truth's
unprojected Gram matrix; the gradient within the same figure in the measure of
test_objective_grad_gpu._rel (|g - ref| / max(|ref_k|, 1e-6 |ref|_inf)).  The numpy
restatement of the method meets both on the CPU (test_objective_fisher_cpu.py: 5.6e-15
and 2.2e-13), so they stand as the project states them.  Between two device paths: the
sum of the two paths' bounds.

Shapes: the 7 JOBS of chisq_grad_truth on the golden arms (ntp 977 and 781, npix 401 and
301), one and two arms, and the cases of tests/objective_grad_shapes.py (groups chunk
geometry, packing, every npoly, dimensions, linear knots, mixed arms; the production
group is the benchmark's size, not a test's).  Every test prints its largest error.

Largest error per group seen on an MI355X on the first run (the whole module: 68 tests in
10.4 s), Fisher matrix / gradient:
    golden arms     9.5e-15 / 2.2e-12     chunk geometry  3.8e-14 / 5.2e-12 (the gradient on
    packing         3.5e-15 / 1.8e-12       chunk-cut860, the alpha component that cancels
    every npoly     9.1e-15 / 1.0e-12       576-fold: rvs_objective_grad measures 3.8e-11
    dimensions      1.9e-15 / 1.3e-13       there; the other eleven cases <= 3.6e-12)
    linear knots    1.2e-15 / 1.3e-13     mixed arms      2.7e-15 / 1.2e-12
Against the chain: Fisher 8.7e-16, gradient 2.2e-13; against rvs_objective_grad: gradient
4.1e-12.  None of these set a bound.  The value is held to the BITS of
rvs_objective_grad: the two kernels share the value phases up to the spline construct and
state the passes over the pixels each in the same words; this is the test
that a change to one of the two statements meets.  (The build before that section already
gave equal bits on every case here.)"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG, gold_lib_dict
from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import vsini_grad_truth as vtruth
import objective_fisher_restated as fwd
import objective_grad_shapes as shapes
from test_chisq_fisher_gpu import BOUND
from test_objective_grad_gpu import _rel

pytestmark = pytest.mark.gpu
J = len(truth.JOBS)
ND = 4
# R (template pixels of gold_b) of the vsini jobs: R < 1, 1 < R < 2, R within 1e-3 of an
# integer, R > 8, vsini = 0 (copy), and two more (test_objective_grad_gpu.test_vsini_row)
RS = [0.4, 1.6, 3 + 5e-4, 9.3, 0.0, 0.7, 2 - 4e-4]
WORST = {}


def _note(group, fe, ge):
    w = WORST.setdefault(group, [0.0, 0.0])
    w[0], w[1] = max(w[0], fe), max(w[1], ge)
    return w


def _make(cases, narm):
    from rvspecfit_amd import _lib, spec_inter, spec_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    cfg = dict(GOLD_CONFIG, template_lib='golden://')
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, gold_lib_dict(n)), 'golden://')
    sds = [sd[:narm] for sd in truth.spectra(cases, spec_fit.SpecData)]
    osds = [sd[:narm] for sd in truth.spectra(cases, orc.SpecData)]
    batch = SpecBatch.from_specdata(sds)
    libs = spec_inter.get_libs(batch.names, cfg)
    dev = batch.device
    f64 = dict(dtype=torch.float64, device=dev)
    lnstep = libs['gold_b'].lnstep
    return dict(cfg=cfg, sds=sds, osds=osds, batch=batch, libs=libs, dev=dev, narm=narm,
                idx=torch.tensor([j[0] for j in truth.JOBS], device=dev),
                vel=torch.tensor([j[1] for j in truth.JOBS], **f64),
                par=torch.tensor([j[2] for j in truth.JOBS], **f64),
                vs=torch.tensor([j[3] or 0.0 for j in truth.JOBS], **f64),
                vsR=torch.tensor([r * vtruth.C_KMS * lnstep for r in RS], **f64))


@pytest.fixture(scope='module')
def setup(cases):
    return _make(cases, 2)


@pytest.fixture(scope='module')
def setup1(cases):
    return _make(cases, 1)


@pytest.fixture(scope='module')
def olibs():
    return {n: orc.Library(gold_lib_dict(n)) for n in ('gold_b', 'gold_r')}


def _fisher(su, npoly, order=None, vsini_grad=False, vs=None, vel=None, work_bytes=None):
    from rvspecfit_amd import engine
    sel = torch.arange(J, device=su['dev']) if order is None else torch.tensor(
        order, device=su['dev'])
    vs = su['vs'] if vs is None else vs
    vel = su['vel'] if vel is None else vel
    return engine.objective_fisher_fused(
        su['batch'], su['libs'], su['par'][sel].contiguous(), vs[sel].contiguous(),
        vel[sel].contiguous(), npoly, True, su['idx'][sel].to(torch.int32).contiguous(),
        vsini_grad, work_bytes=work_bytes)


def _grad(su, npoly, vsini_grad=False, vs=None, vel=None):
    from rvspecfit_amd import engine
    return engine.objective_grad_fused(
        su['batch'], su['libs'], su['par'], su['vs'] if vs is None else vs,
        su['vel'] if vel is None else vel, npoly, True,
        su['idx'].to(torch.int32).contiguous(), vsini_grad)


def _chain(su, npoly, vsini_grad=False, vs=None):
    from rvspecfit_amd import spec_fit
    return spec_fit.chisq_fisher_jobs(
        su['batch'], su['idx'], su['vel'], su['par'], su['vs'] if vs is None else vs,
        dict(npoly=npoly), su['cfg'], vsini_grad=vsini_grad)


def _truths(su, olibs, j, npoly, vsini_grad, vs):
    """(value, gradient, F, G, cond) of job j on the setup's arms"""
    s, vel, par, _ = truth.JOBS[j]
    sds = su['osds'][s]
    if vsini_grad:
        val, g = vtruth.chisq_and_grad_vsini(sds, olibs, vel, par, vs or 0.0, npoly=npoly)
    else:
        val, g = truth.chisq_and_grad(sds, olibs, vel, par, vs, npoly=npoly)
    Ft, G, cond = fwd.fisher_truth(sds, olibs, vel, par, vs, npoly=npoly,
                                   vsini_grad=vsini_grad)
    return val, g, Ft, G, cond


# ---- 1. against the truths -----------------------------------------------------------
@pytest.mark.parametrize('narm', [1, 2])
@pytest.mark.parametrize('vsini_grad', [False, True])
@pytest.mark.parametrize('npoly', [1, 5, 10])
def test_against_the_truths(setup, setup1, olibs, npoly, vsini_grad, narm):
    """F and g on the in-cell JOBS; with the vsini column the jobs are broadened at RS
    (job 4: vsini = 0, the copy branch), without it job 3 alone is (30 km/s)"""
    su = setup if narm == 2 else setup1
    vs = su['vsR'] if vsini_grad else su['vs']
    chi, grad, F, st = _fisher(su, npoly, vsini_grad=vsini_grad, vs=vs)
    K = 1 + ND + int(vsini_grad)
    assert grad.shape == (J, K) and F.shape == (J, K, K)
    grad, F = grad.cpu().numpy(), F.cpu().numpy()
    wf = wg = 0.0
    for j in truth.INSIDE:
        v = float(vs[j].item()) or None
        val, g, Ft, G, cond = _truths(su, olibs, j, npoly, vsini_grad, v)
        assert int(st[j].item()) == 0
        assert abs(chi[j].item() - val) <= 1e-7 * abs(val)
        ef, eg = float(fwd.rel_fisher(F[j], Ft, G).max()), float(_rel(grad[j], g).max())
        print('npoly %d vsini %d narm %d job %d cond(A) %.3g Fisher error %.3g of '
              'sqrt(G_ii G_ll) gradient error %.3g' % (npoly, vsini_grad, narm, j, cond,
                                                       ef, eg))
        wf, wg = max(wf, ef), max(wg, eg)
    w = _note('golden', wf, wg)
    print('npoly %d vsini %d narm %d largest Fisher error %.3g gradient %.3g (bound %.3g;'
          ' so far %.3g, %.3g)' % (npoly, vsini_grad, narm, wf, wg, BOUND, w[0], w[1]))
    assert wf <= BOUND
    assert wg <= BOUND


# ---- 2. the other paths -----------------------------------------------------------------
@pytest.mark.parametrize('vsini_grad', [False, True])
@pytest.mark.parametrize('npoly', [5, 10])
def test_agreement_with_the_chain_and_the_gradient_kernel(setup, olibs, npoly, vsini_grad):
    su = setup
    vs = su['vsR'] if vsini_grad else su['vs']
    chi, grad, F, st = _fisher(su, npoly, vsini_grad=vsini_grad, vs=vs)
    cchi, cgrad, cF, cst = _chain(su, npoly, vsini_grad, vs)
    gchi, ggrad, gst = _grad(su, npoly, vsini_grad, vs)
    assert torch.equal(st, gst), (st, gst)
    assert torch.equal(st, cst), (st, cst)
    # the same value phases in both kernels: the bits
    assert torch.equal(torch.isnan(chi), torch.isnan(gchi))
    assert torch.equal(torch.nan_to_num(chi), torch.nan_to_num(gchi)), (chi, gchi)
    grad, F, cgrad, cF = (x.cpu().numpy() for x in (grad, F, cgrad, cF))
    ggrad = ggrad.cpu().numpy()
    wf = wg = wgg = 0.0
    for j in range(6):     # in-cell jobs and job 5, outside the grid
        v = float(vs[j].item()) or None
        s, vel, par, _ = truth.JOBS[j]
        _, G, _ = fwd.fisher_truth(su['osds'][s], olibs, vel, par, v, npoly=npoly,
                                   vsini_grad=vsini_grad)
        ef = float(fwd.rel_fisher(F[j], cF[j], G).max())
        eg, egg = float(_rel(grad[j], cgrad[j]).max()), float(_rel(grad[j], ggrad[j]).max())
        print('npoly %d vsini %d job %d against the chain: Fisher %.3g gradient %.3g; '
              'against rvs_objective_grad: gradient %.3g' % (npoly, vsini_grad, j, ef, eg,
                                                            egg))
        wf, wg, wgg = max(wf, ef), max(wg, eg), max(wgg, egg)
    print('npoly %d vsini %d largest: chain Fisher %.3g gradient %.3g, gradient kernel '
          '%.3g' % (npoly, vsini_grad, wf, wg, wgg))
    # the sum of the two paths' bounds: the chain's are BOUND for both (test_chisq_fisher_
    # gpu.py, test_chisq_grad_gpu.py), the adjoint kernel's 4.72e-11
    from test_objective_grad_gpu import REL_ERR_BOUND
    assert wf <= 2 * BOUND and wg <= 2 * BOUND
    assert wgg <= BOUND + REL_ERR_BOUND
    # job 6, a non-finite mapped parameter: the penalty, no gradient, no matrix
    assert chi[6].item() == 2 * 1000.0 * su['batch'].badchi == cchi[6].item()
    assert not grad[6].any() and not F[6].any()


# ---- 3. exactness ------------------------------------------------------------------------
def test_exactness_properties(setup):
    su = setup
    for npoly in (1, 5, 10):
        chi, grad, F, st = _fisher(su, npoly)
        assert torch.equal(F, F.transpose(-1, -2))
        chiv, gradv, Fv, stv = _fisher(su, npoly, vsini_grad=True)
        assert Fv.shape == (J, 2 + ND, 2 + ND)
        assert torch.equal(Fv, Fv.transpose(-1, -2))
        # the leading block and the value do not know of the vsini row
        assert torch.equal(Fv[:, :1 + ND, :1 + ND], F) and torch.equal(chiv, chi)
        assert torch.equal(gradv[:, :1 + ND], grad) and torch.equal(stv, st)
        # vsini <= 0, the FIR's copy branch: row and column exactly 0
        for j in range(J):
            if truth.JOBS[j][3] is None:
                assert not Fv[j, 1 + ND].any() and not Fv[j, :, 1 + ND].any()
                assert gradv[j, 1 + ND].item() == 0.0
        assert Fv[3, 1 + ND, 1 + ND].item() > 0
        Fn = F.cpu().numpy()
        for j in truth.INSIDE:
            d = np.sqrt(np.diag(Fn[j]))
            assert (d > 0).all()
            ev = np.linalg.eigvalsh(Fn[j] / (d[:, None] * d[None, :]))
            print('npoly %d job %d smallest scaled eigenvalue %.3g' % (npoly, j, ev.min()))
            assert ev.min() >= -1e-11
        # job 5, outside the grid: the nearest node's template, parameter rows exactly 0
        assert Fn[5][0, 0] > 0 and not Fn[5][1:].any() and not Fn[5][:, 1:].any()
        assert not grad[5, 1:].any() and grad[5, 0].item() != 0.0
        # ... but vsini does not drop out there
        _, gR, FR, _ = _fisher(su, npoly, vsini_grad=True, vs=su['vsR'])
        assert FR[5, 5, 5].item() > 0 and not FR[5, 1:5].any() and not FR[5, :, 1:5].any()
        # job 6, a non-finite outside flag on both arms: 1000 badchi each, nothing else
        assert chi[6].item() == 2 * 1000.0 * su['batch'].badchi
        assert not Fn[6].any() and not Fv[6].any() and not grad[6].any()


def test_nan_where_the_value_is(setup):
    """a velocity that puts the pixels beyond the knots: RVS_ST_SPLINE_RANGE, the value
    NaN -- and with it g and F, under the status bits of rvs_objective_grad"""
    from rvspecfit_amd import _lib
    su = setup
    vel = su['vel'].clone()
    vel[1] = -30000.0
    chi, grad, F, st = _fisher(su, 10, vel=vel)
    gchi, ggrad, gst = _grad(su, 10, vel=vel)
    assert torch.equal(st, gst)
    assert int(st[1].item()) & _lib.ST_SPLINE_RANGE and int(st[1].item()) & _lib.ST_NONFINITE
    assert torch.isnan(chi[1]) and torch.isnan(grad[1]).all() and torch.isnan(F[1]).all()
    keep = [0, 2, 3, 4, 5, 6]
    ref = _fisher(su, 10)
    for a, b in zip((chi, grad, F, st), ref):
        assert torch.equal(a[keep], b[keep])


# ---- 4. determinism ----------------------------------------------------------------------
def test_determinism(setup):
    from rvspecfit_amd import _lib
    su = setup
    ws = _lib.lib().rvs_objective_fisher_work_size
    for vg in (False, True):
        vs = su['vsR'] if vg else su['vs']
        a = _fisher(su, 10, vsini_grad=vg, vs=vs)
        b = _fisher(su, 10, vsini_grad=vg, vs=vs)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        perm = [4, 2, 6, 0, 5, 1, 3]
        c = _fisher(su, 10, perm, vsini_grad=vg, vs=vs)
        sel = torch.tensor(perm, device=su['dev'])
        for x, y in zip(a, c):
            assert torch.equal(x[sel], y)
        # the work buffer of ONE job (seven launches), of three (3 + 3 + 1) and of all
        ntan = ND + int(vg)
        one = ws(1, 2, ntan, 401)
        assert ws(J, 2, ntan, 401) == J * one
        for nb in (one, 3 * one + 8):
            d = _fisher(su, 10, vsini_grad=vg, vs=vs, work_bytes=nb)
            for x, y in zip(a, d):
                assert torch.equal(x, y)


def test_default_work_budget(setup, monkeypatch):
    """engine.objective_fisher_fused bounds its own work buffer: with a budget of two jobs
    the seven jobs go in four launches, with the bits of one launch"""
    from rvspecfit_amd import _lib, engine
    su = setup
    a = _fisher(su, 10, vsini_grad=True, vs=su['vsR'])
    one = _lib.lib().rvs_objective_fisher_work_size(1, 2, ND + 1, 401)
    monkeypatch.setattr(engine, 'FISHER_FUSED_WORK_BUDGET', 2 * one + 100)
    b = _fisher(su, 10, vsini_grad=True, vs=su['vsR'])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    monkeypatch.setattr(engine, 'FISHER_FUSED_WORK_BUDGET', 1)     # below one job: one job
    c = _fisher(su, 10, vsini_grad=True, vs=su['vsR'])
    for x, y in zip(a, c):
        assert torch.equal(x, y)


# ---- 5. shapes ----------------------------------------------------------------------------
_dev = {}
_registered = set()


def _device(c):
    if c.name in _dev:
        return _dev[c.name]
    from rvspecfit_amd import _lib, spec_fit, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    for n, _ in c.arms:
        if n not in _registered:
            spec_inter.register_library(TemplateLibrary(n, shapes.lib_dict(n)),
                                        shapes.ROOT)
            _registered.add(n)
    batch = SpecBatch.from_specdata(shapes.specdata(c, spec_fit.SpecData))
    libs = spec_inter.get_libs(batch.names, shapes.config())
    f64 = dict(dtype=torch.float64, device=batch.device)
    vs = None
    if any(j[3] is not None for j in c.jobs):
        vs = torch.tensor([j[3] or 0.0 for j in c.jobs], **f64)
    d = dict(batch=batch, libs=libs, vs=vs,
             idx=torch.tensor([j[0] for j in c.jobs], dtype=torch.int32,
                              device=batch.device),
             vel=torch.tensor([j[1] for j in c.jobs], **f64),
             par=torch.tensor([list(j[2]) for j in c.jobs], **f64))
    _dev.clear()
    _dev[c.name] = d
    return d


def _check_shape(name):
    """an in-cell case of tests/objective_grad_shapes.py: status 0, the value within 1e-7
    |truth|, g and F within the bound; status and value (bit for bit) those of
    rvs_objective_grad"""
    from rvspecfit_amd import engine
    c = shapes.case(name)
    d = _device(c)
    args = (d['batch'], d['libs'], d['par'], d['vs'], d['vel'], c.npoly, c.rbf, d['idx'],
            c.vsini_grad)
    chi, grad, F, st = engine.objective_fisher_fused(*args)
    gchi, ggrad, gst = engine.objective_grad_fused(*args)
    K = 1 + c.ndim + (1 if c.vsini_grad else 0)
    assert grad.shape == (len(c.jobs), K) and F.shape == (len(c.jobs), K, K)
    assert torch.equal(st, gst) and not st.any()
    # the same value phases in both kernels: the bits
    assert torch.equal(torch.isnan(chi), torch.isnan(gchi))
    assert torch.equal(torch.nan_to_num(chi), torch.nan_to_num(gchi)), (name, chi, gchi)
    assert torch.equal(F, F.transpose(-1, -2))
    grad, F = grad.cpu().numpy(), F.cpu().numpy()
    wf = wg = 0.0
    for j, (s, vel, par, vs) in enumerate(c.jobs):
        val, g = shapes.truth_job(c, j)
        sds = shapes.specdata(c, orc.SpecData)[s]
        with truth.banded_spline(shapes.BANDED_ABOVE):
            Ft, G, cond = fwd.fisher_truth_columns(sds, shapes.olibs(c), vel, par, vs,
                                                   npoly=c.npoly, rbf=c.rbf,
                                                   vsini_grad=c.vsini_grad)
        assert abs(chi[j].item() - val) <= 1e-7 * abs(val), (name, j)
        wf = max(wf, float(fwd.rel_fisher(F[j], Ft, G).max()))
        wg = max(wg, float(shapes.rel_err(grad[j], g).max()))
    w = _note(c.group, wf, wg)
    print('%s largest Fisher error %.3g of sqrt(G_ii G_ll), gradient %.3g (bound %.3g; '
          'group %s so far %.3g, %.3g)' % (name, wf, wg, BOUND, c.group, w[0], w[1]))
    assert wf <= BOUND
    assert wg <= BOUND


@pytest.mark.parametrize('name', shapes.names('chunk'))
def test_chunk_geometry(name):
    _check_shape(name)


@pytest.mark.parametrize('name', shapes.names('packing'))
def test_packing(name):
    """R = 9.3 and 11.5 on 64, 65, 33 and 32 knots: the taps and their derivatives (2 kmax
    + 2 doubles) and the primitives' stage (2 (kmax + 3)) in buffers of ntp doubles"""
    _check_shape(name)


@pytest.mark.parametrize('name', shapes.names('every_p'))
def test_every_npoly(name):
    _check_shape(name)


@pytest.mark.parametrize('name', shapes.names('dims'))
def test_lower_dimensional_grids(name):
    _check_shape(name)


@pytest.mark.parametrize('name', shapes.names('linear'))
def test_linear_knots(name):
    _check_shape(name)


@pytest.mark.parametrize('name', shapes.names('mixed'))
def test_mixed_arms(name):
    _check_shape(name)


@pytest.mark.parametrize('name', ['chunk-cut835', 'mixed-cut32-fine6485'])
def test_shapes_determinism(name):
    """twice, permuted, and with the work buffer of one job: the same bits"""
    from rvspecfit_amd import _lib, engine
    c = shapes.case(name)
    d = _device(c)

    def run(order=None, nb=None):
        sel = torch.arange(len(c.jobs), device=d['vel'].device) if order is None else \
            torch.tensor(order, device=d['vel'].device)
        return engine.objective_fisher_fused(
            d['batch'], d['libs'], d['par'][sel].contiguous(),
            None if d['vs'] is None else d['vs'][sel].contiguous(),
            d['vel'][sel].contiguous(), c.npoly, c.rbf, d['idx'][sel].contiguous(),
            c.vsini_grad, work_bytes=nb)
    a = run()
    for x, y in zip(a, run()):
        assert torch.equal(x, y)
    perm = [2, 0, 3, 1]
    sel = torch.tensor(perm, device=d['vel'].device)
    for x, y in zip(a, run(perm)):
        assert torch.equal(x[sel], y)
    one = _lib.lib().rvs_objective_fisher_work_size(
        1, len(c.arms), c.ndim, max(n for _, n in c.arms))
    for x, y in zip(a, run(nb=one)):
        assert torch.equal(x, y)


# ---- 8. refusals at the C entry -----------------------------------------------------------
def test_c_entry_refusals(setup):
    """RVS_E_ARG, before any launch, for a work buffer below the one-job size and for
    what the kernel does not cover: a resolution matrix, fast_interp, npoly 11, a grid set"""
    from rvspecfit_amd import _lib, engine
    su = setup
    L = _lib.lib()
    batch, libs = su['batch'], su['libs']
    arr = (_lib.ObjectiveArm * 2)()
    bconst = (ctypes.c_double * 2)()
    keep = engine.fill_objective_grad_arms(arr, bconst, batch, libs, 10, True)
    dev = su['dev']
    one = L.rvs_objective_fisher_work_size(1, 2, ND, 401)
    work = torch.empty(one // 8, dtype=torch.float64, device=dev)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    grad = torch.zeros((1, 5), dtype=torch.float64, device=dev)
    F = torch.zeros((1, 5, 5), dtype=torch.float64, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    par, vel = su['par'][:1].contiguous(), su['vel'][:1].contiguous()

    def call(npoly=10, nb=one):
        rc = L.rvs_objective_fisher(ctypes.addressof(arr), 2, npoly, ND, _lib.ptr(par),
                                    None, None, 1, _lib.ptr(vel), float(batch.badchi),
                                    ctypes.addressof(bconst), _lib.ptr(work), nb,
                                    _lib.ptr(out), _lib.ptr(grad), _lib.ptr(F),
                                    _lib.ptr(st), _lib.stream())
        torch.cuda.synchronize()
        return rc
    assert call() == 0
    ref = _fisher(su, 10, order=[0])
    assert torch.equal(out, ref[0]) and torch.equal(F, ref[2])
    assert call(nb=one - 8) == -1
    assert call(npoly=11) == -1
    arr[0].pt.fast_interp = 1
    assert call() == -1
    arr[0].pt.fast_interp = 0
    taps = arr[1].pt.taps
    arr[1].pt.taps = _lib.ptr(work)
    assert call() == -1
    arr[1].pt.taps = taps
    arr[0].pt.G = 2
    assert call() == -1
    arr[0].pt.G = 0
    assert call() == 0
    del keep


# ---- 6. the LM rounds ----------------------------------------------------------------------
from test_bfgs_jac_gpu import (NPOLY, _fake_stars, _objective, _x0,  # noqa: E402, F401
                               nm_optimum, setups)

LM_KEYS = ('x', 'fun', 'grad', 'hess', 'mu', 'nit', 'nfev', 'status')


def _lm_pair(su, S, x0, cap=None, **kw):
    """rvs_lm_run_fused against lm.minimize_lockstep_native fed by the same fused rows"""
    from rvspecfit_amd import lm, optimizer
    pobj, args = _objective(su, S, **kw)
    chain = optimizer.GradChain(pobj, cap=cap, fused_fisher=True)
    assert chain.fisher and chain.fused_fisher and not chain.fused
    for k in ('arms', 'point', 'point_work', 'fisher_work', 'fisher_buf'):
        assert not hasattr(chain, k), k              # no row buffers
    dev_r = lm.minimize_lockstep_device(pobj, x0, chain=chain)
    host = lm.minimize_lockstep_native(chain.rows, x0.cpu().numpy())
    d = {k: dev_r[k].cpu().numpy() for k in LM_KEYS}
    print('device nit', d['nit'], 'nfev', d['nfev'], 'status', d['status'], 'rounds',
          dev_r['rounds'], 'calls', dev_r['calls'])
    print('host   nit', host['nit'], 'nfev', host['nfev'], 'status', host['status'],
          'rounds', host['rounds'])
    for k in LM_KEYS:
        assert np.array_equal(d[k], host[k]), k
    assert host['rounds'] <= dev_r['rounds'] < host['rounds'] + 4
    f0 = chain.rows(np.arange(S), x0.cpu().numpy())[:, 0]
    assert (d['fun'] <= f0).all(), (d['fun'], f0)
    return pobj, chain, dev_r, d


def test_lm_run_fused_equals_host_machine(setups, nm_optimum):   # noqa: F811
    """S = 8, n = 6, bit for bit; twice; and under permuted spectra"""
    from rvspecfit_amd import lm, optimizer
    su = setups['grid']
    S = 8
    cols = ['vel', 'vsini'] + su['names']
    x0 = _x0(nm_optimum, su['names'], S, cols)
    pobj, chain, dev_r, d = _lm_pair(su, S, x0)
    assert d['nfev'].max() > 2 and (d['nfev'] >= d['nit'] + 1).all()
    again = lm.minimize_lockstep_device(pobj, x0, chain=chain)
    for k in LM_KEYS:
        assert np.array_equal(again[k].cpu().numpy(), d[k]), k
    # the fused rows against the chain's: value within 1e-11 max(|f|, 1e3)
    pobj_c, _ = _objective(su, S)
    rows_c = optimizer.GradChain(pobj_c, fisher=True).rows(np.arange(S), x0.cpu().numpy())
    rows_f = chain.rows(np.arange(S), x0.cpu().numpy())
    assert rows_f.shape == rows_c.shape == (S, lm.npack(6))
    assert (np.abs(rows_f[:, 0] - rows_c[:, 0]) <=
            1e-11 * np.maximum(np.abs(rows_c[:, 0]), 1e3)).all()
    perm = [4, 2, 6, 0, 7, 5, 1, 3]
    sub = dict(su, batch=su['batch'].subset(torch.tensor(perm, device='cuda')),
               sds=[su['sds'][i] for i in perm])
    pobj2, _ = _objective(sub, S)
    r2 = lm.minimize_lockstep_device(
        pobj2, x0[perm].contiguous(),
        chain=optimizer.GradChain(pobj2, fused_fisher=True))
    for k in LM_KEYS:
        assert np.array_equal(r2[k].cpu().numpy(), d[k][perm]), k


def test_lm_run_fused_in_chunks(setups, nm_optimum):   # noqa: F811
    """S = 5 in chunks of 3: the results of one chunk"""
    from rvspecfit_amd import lm, optimizer
    su = setups['grid']
    S = 5
    cols = ['vel', 'vsini'] + su['names']
    x0 = _x0(nm_optimum, su['names'], S, cols)
    pobj, chain, dev_r, d = _lm_pair(su, S, x0, cap=3)
    assert chain.cap == 3
    assert dev_r['calls'] >= 2 * min(dev_r['rounds'], 2)
    pobj1, _ = _objective(su, S)
    one = lm.minimize_lockstep_device(
        pobj1, x0, chain=optimizer.GradChain(pobj1, fused_fisher=True))
    for k in LM_KEYS:
        assert np.array_equal(one[k].cpu().numpy(), d[k]), k


def test_lm_run_fused_one_run_one_dimension(setups, nm_optimum):   # noqa: F811
    """S = 1, n = 1: the velocity alone"""
    su = setups['grid']
    fix = tuple(su['names']) + ('vsini', )
    x0 = _x0(nm_optimum, su['names'], 1, ['vel']) + 3.0
    pobj, chain, dev_r, d = _lm_pair(su, 1, x0, fix=fix)
    assert pobj.n == 1 and d['nit'][0] >= 1


def test_grad_chain_refusals(setups):   # noqa: F811
    """GradChain(fused=True, fisher=True) keeps its refusal, with and without the new
    keyword; rvs_lm_run_fused refuses a work buffer below the matrices plus one job"""
    from rvspecfit_amd import _lib, lm, optimizer
    su = setups['grid']
    pobj, _ = _objective(su, 2)
    for kw in (dict(), dict(fused_fisher=True)):
        with pytest.raises(ValueError, match=r'(?s)fused_gradient.*fisher=True'):
            optimizer.GradChain(pobj, fused=True, fisher=True, **kw)
    chain = optimizer.GradChain(pobj, fused_fisher=True)
    one = _lib.lib().rvs_objective_fisher_work_size(
        1, len(su['batch'].arms), chain.ntan, max(a.npix for a in su['batch'].arms))
    chain.nbytes = chain.cap * (1 + chain.ntan)**2 * 8 + one - 8
    x0 = torch.zeros((2, pobj.n), dtype=torch.float64, device='cuda')
    with pytest.raises(Exception, match='rvs_lm_run_fused'):
        lm.minimize_lockstep_device(pobj, x0, chain=chain)


# ---- 7. process ------------------------------------------------------------------------------
PD0_STARS = dict(teff=5200., logg=2.3, feh=-0.8, alpha=0.2, vsini=5.0)


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, torch.Tensor):
        return torch.equal(a, b) or bool(
            (torch.isnan(a) == torch.isnan(b)).all() and
            torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b, equal_nan=a.dtype.kind == 'f')
    return a == b or (isinstance(a, float) and a != a and b != b)


def test_process_with_fused_fisher(cases, setups):   # noqa: F811
    """8 fake stars, config['second_minimizer_lm'] with and without the key: finite
    records, a finite status of every run, chisq no worse than the chain's LM polish from
    the same simplex optimum + 1e-6 |chisq| (the comparison of
    test_process_with_fused_gradient); config['fisher_uncertainties'] with the key:
    covar_fisher within the Fisher bound of the chain's; without the key, and with an
    unrelated false key, the parent's bits"""
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.engine import SpecBatch
    su = setups['grid']
    S = 8
    batch = SpecBatch.from_specdata(_fake_stars(cases, S))
    pd0 = {k: np.full(S, v) for k, v in PD0_STARS.items()}
    out = {}
    for tag, extra in (('chain', {}), ('fused', dict(fused_fisher=True)),
                       ('false', dict(fused_fisher=False, some_unrelated_key=False))):
        cfg = dict(su['cfg'], second_minimizer=True, second_minimizer_lm=True,
                   fisher_uncertainties=True, **extra)
        out[tag] = vel_fit.process(batch, dict(pd0), options=dict(npoly=NPOLY), config=cfg)
    a, b, c = out['fused'], out['chain'], out['false']
    # without the key (absent, or false beside an unrelated key): the same bits
    assert set(b) == set(c)
    for k in b:
        assert _same(b[k], c[k]), k
    assert 'fused' not in b['lm'] and a['lm']['fused'] is True
    assert a['lm']['device'] is True and 'bfgs' not in a
    assert np.isin(a['lm']['status'], (0, 1, 2)).all()
    assert (a['lm']['nfev'] >= 1).all()
    for k in ('vel', 'vel_err', 'chisq', 'vsini'):
        assert torch.isfinite(a[k]).all(), k
    for k in su['names']:
        assert torch.isfinite(a['param'][k]).all(), k
    ca, cb = a['chisq'].cpu().numpy(), b['chisq'].cpu().numpy()
    print('chisq fused', ca, 'chain', cb, 'fused - chain', ca - cb, 'nit', a['lm']['nit'],
          b['lm']['nit'], 'nfev', a['lm']['nfev'], b['lm']['nfev'], 'status',
          a['lm']['status'], b['lm']['status'])
    assert (ca <= cb + 1e-6 * np.abs(cb)).all(), ca - cb
    # covar_fisher: at ONE point both forms -- the chain's optimum -- through
    # fisher_uncertainties with and without the key
    names = su['names']
    par = torch.stack([b['param'][k] for k in names], dim=1)
    fu = {}
    for key in (False, True):
        fu[key] = vel_fit.fisher_uncertainties(
            batch, b['vel'], par, vsini=b['vsini'], options=dict(npoly=NPOLY),
            config=dict(su['cfg'], fused_fisher=key), vsini_grad=True)
    assert fu[False]['covar'].shape == np.asarray(b['covar_fisher']).shape
    Fa, Fb = fu[True]['fisher'], fu[False]['fisher']
    worst = 0.0
    for s in range(S):
        g = np.sqrt(np.diag(Fb[s]))        # F_ii <= G_ii: no wider than sqrt(G_ii G_ll)
        ok = g > 0
        rel = np.abs(Fa[s] - Fb[s])[np.ix_(ok, ok)] / (g[ok][:, None] * g[ok][None, :])
        worst = max(worst, float(rel.max()))
        assert np.array_equal(Fa[s][~ok], Fb[s][~ok])
    print('fisher_uncertainties: largest |F_fused - F_chain| / sqrt(F_ii F_ll) %.3g '
          '(bound %.3g)' % (worst, 2 * BOUND))
    assert worst <= 2 * BOUND
    # ... and the covariance: the inversion's conditioning times that (the argument of
    # test_chisq_fisher_gpu.test_fisher_uncertainties: 1e-8 of sqrt(C_ii C_ll))
    Ca, Cb = fu[True]['covar'], fu[False]['covar']
    for s in range(S):
        if fu[False]['bad_fisher'][s]:
            continue
        sc = np.sqrt(np.diag(Cb[s]))
        assert (np.abs(Ca[s] - Cb[s]) / (sc[:, None] * sc[None, :])).max() <= 1e-8
    assert set(a) == set(b) and a['names_fisher'] == b['names_fisher']
    assert np.isfinite(np.asarray(a['vel_err_fisher'].cpu())).all()


def test_public_calls_with_the_key(setup):
    """get_chisq_fisher, chisq_fisher_jobs, chisq_func_fisher through the key are the
    engine call's bits; without it the chain's"""
    from rvspecfit_amd import spec_fit
    su = setup
    cfgk = dict(su['cfg'], fused_fisher=True)
    ref = _fisher(su, 10)
    got = spec_fit.chisq_fisher_jobs(su['batch'], su['idx'], su['vel'], su['par'],
                                     su['vs'], dict(npoly=10), cfgk)
    for x, y in zip(ref, got):
        assert torch.equal(x, y)
    chain = _chain(su, 10)
    off = spec_fit.chisq_fisher_jobs(su['batch'], su['idx'], su['vel'], su['par'],
                                     su['vs'], dict(npoly=10),
                                     dict(su['cfg'], fused_fisher=False))
    for x, y in zip(chain, off):
        assert torch.equal(x, y) or (x.dtype.is_floating_point and torch.equal(
            torch.nan_to_num(x), torch.nan_to_num(y)))
    _, vel, par, _ = truth.JOBS[0]
    c1, g1, F1 = spec_fit.get_chisq_fisher(su['sds'][0], vel, par, options=dict(npoly=10),
                                           config=cfgk)
    assert c1 == ref[0][0].item() and (F1 == ref[2][0].cpu().numpy()).all()
    assert (g1 == ref[1][0].cpu().numpy()).all()


# ---- 8. refusals -------------------------------------------------------------------------------
def test_refusals(cases, setup, setups):   # noqa: F811
    """each option the kernel does not cover raises ValueError naming it and the key,
    from get_chisq_fisher and from process (second_minimizer_lm and
    fisher_uncertainties)"""
    import os
    from conftest import GOLD
    from rvspecfit_amd import engine, spec_fit, spec_inter, vel_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    import tri_grad_truth as ttruth
    su = setup
    _, vel, par, _ = truth.JOBS[0]
    sd = su['sds'][0]
    cfg = dict(su['cfg'], fused_fisher=True)
    pcfgs = [dict(cfg, second_minimizer=True, second_minimizer_lm=True),
             dict(cfg, fisher_uncertainties=True)]
    S = 2
    pbatch = SpecBatch.from_specdata(_fake_stars(cases, S))
    pd0 = dict(teff=np.full(S, 5200.), logg=np.full(S, 2.3), feh=np.full(S, -0.8),
               alpha=np.full(S, 0.2), vsini=np.full(S, 5.0))
    opt = dict(npoly=10)

    def both(match, g_kw=None, p_kw=None, g_sd=sd, p_batch=pbatch, g_cfg=cfg,
             p_over=None, g_opt=opt, p_opt=opt, g_vel=vel, g_par=par):
        pat = r'(?s)fused_fisher.*%s|%s.*fused_fisher' % (match, match)
        with pytest.raises(ValueError, match=pat):
            spec_fit.get_chisq_fisher(g_sd, g_vel, g_par, options=g_opt, config=g_cfg,
                                      **(g_kw or {}))
        for pc in pcfgs:
            with pytest.raises(ValueError, match=pat):
                vel_fit.process(p_batch, dict(pd0), options=p_opt,
                                config=dict(pc, **(p_over or {})), **(p_kw or {}))
    rp = {x.name: spec_fit.construct_resol_mat(x.lam, width=0.5) for x in sd}
    prp = {a.name: spec_fit.construct_resol_mat(a.lam_host, 2500.) for a in pbatch.arms}
    both('resolution matrix', dict(resol_params=rp), dict(resolParams=prp))
    both('fast_interp', dict(fast_interp=True), None, p_opt=dict(npoly=10,
                                                                 fast_interp=True))
    both('npoly', g_opt=dict(npoly=11), p_opt=dict(npoly=11))
    other = [spec_fit.SpecData(x.name, x.lam[:-3], x.spec[:-3], x.espec[:-3],
                               badmask=x.badmask[:-3]) for x in su['sds'][1]]
    gs = SpecBatch.from_specdata([sd, other])
    stars = _fake_stars(cases, 2)
    lam = stars[0][0].lam
    gset = SpecBatch([engine.ArmData(
        'gold_b', [lam, lam[:-7]], np.stack([stars[0][0].spec, stars[1][0].spec]),
        np.stack([stars[0][0].espec, stars[1][0].espec]), device='cuda',
        grid_id=np.arange(2, dtype=np.int32))])
    both('grid set', g_sd=gs, g_vel=[vel, vel], p_batch=gset)
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, ttruth.tri_lib_dict(n)),
                                    'golden-tri://')
    both('triangulation', g_cfg=dict(cfg, template_lib='golden-tri://'),
         p_over=dict(template_lib='golden-tri://'))
    d = dict(np.load(os.path.join(GOLD, 'nn_case.npz')))
    dd = dict(lam=np.exp(np.linspace(np.log(3950.), np.log(5060.), int(d['dims'][-1]))),
              log_step=np.array(True), log_ids=np.array([0]),
              parnames=np.array(['teff', 'logg', 'feh', 'alpha']),
              nn_dims=d['dims'], nn_M=d['M'], nn_S=d['S'])
    for i in range(len(d['dims']) - 1):
        dd['nn_W%d' % i], dd['nn_b%d' % i] = d['W%d' % i], d['b%d' % i]
    spec_inter.register_library(TemplateLibrary('aat_580v', dd), 'golden-nn://')
    wave = np.linspace(4000, 5000, 1000)
    rng = np.random.RandomState(3)
    nn_sds = [[spec_fit.SpecData('aat_580v', wave, rng.normal(1, 0.1, 1000),
                                 np.full(1000, 0.1))] for _ in range(2)]
    both('nn library', g_sd=nn_sds[0], p_batch=SpecBatch.from_specdata(nn_sds),
         g_cfg=dict(GOLD_CONFIG, template_lib='golden-nn://', fused_fisher=True,
                    nn_gradient=True),
         p_over=dict(template_lib='golden-nn://', nn_gradient=True),
         g_opt=dict(npoly=5), p_opt=dict(npoly=5))
    with pytest.raises(ValueError, match=r'(?s)fused_fisher.*epochs'):
        vel_fit.process_epochs(pbatch, np.array([0, 0]),
                               {k: v[:1] for k, v in pd0.items()}, np.zeros(2),
                               options=opt, config=cfg)
    # the other key keeps its refusals beside this one
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*Fisher'):
        spec_fit.get_chisq_fisher(sd, vel, par, options=opt,
                                  config=dict(cfg, fused_gradient=True))
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*second_minimizer_lm'):
        vel_fit.process(pbatch, dict(pd0), options=opt,
                        config=dict(pcfgs[0], fused_gradient=True))
