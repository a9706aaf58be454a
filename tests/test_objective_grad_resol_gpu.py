"""rvs_objective_grad_resol / rvs_objective_grad_from_template_resol (csrc/objective_grad.hip,
the RESOL form: value and gradient in one kernel per (job, arm) under banded resolution
matrices, the band's transpose applied to the one adjoint row) and the
interfaces above them -- config['fused_gradient'] beside config['resol_gradient'] --
against the float64 autograd truth under dense matrices (tests/chisq_grad_resol_truth.py),
against the value kernel under the same matrices (engine.objective_fused), against the
calls without matrices (identity bands), and through optimizer.GradChain(fused=True),
rvs_bfgs_run_grad_fused_resol and vel_fit.process.

Shapes: the 7 JOBS of chisq_grad_truth on the golden arms (401 and 301 pixels, ntp 977 and
781) under the matrices of chisq_grad_resol_truth (9 ... 25 diagonals), and one arm of
1100 pixels on objective_grad_shapes.fine(2600) under 17 and 25 diagonals: a thread owns
up to three pixels there and the band crosses the thread stride at pixels 512 and 1024.

Bounds.  Value: 1e-11 max(|v|, 1e3), as everywhere.  Gradient: relative to
max(|g_k|, 1e-6 |g|_inf), 10 x MEASURED_REL_ERR, the largest error of this file's tests on
an MI355X; that is below REL_ERR_BOUND of tests/test_objective_grad_gpu.py (10 x 4.72e-12,
the kernel without a band -- the band adds at most 33 fused multiply-adds per pixel to
sums of hundreds of terms), and DEFECT of that file (5e-10) is the hard ceiling.
Adjoint row: relative to the absolute sum behind each entry, against float64 autograd with
the template row as the leaf through the dense matrix (tests/adjoint_row_resol_truth.py);
the bound is 10 x the numpy restatement's own error in that measure
(tests/test_objective_grad_resol_cpu.py: RESTATED_ROW_ERR) plus what one unit in the last
place of the pixels' coordinates x = lam f moves the row by -- the kernel forms
lam f - knot as a fused multiply-add behind its own rounding of f, the truth and the
restatement round the product, and the row is that sensitive (ulp(x) / h: 9e-13 A on
knots 0.4 A apart; on the 3.3-A knots of tests/test_nn_vjp_gpu.py the same comparison
measures ten times less, 1.94e-13 of the largest entry).

Largest errors seen on an MI355X, DESIGN 4.27:
  gradient   golden jobs 2.87e-13 (npoly 5), 6.59e-13 (npoly 10); the long arm 2.61e-13 /
             3.38e-13; padded to 33 diagonals 6.59e-13; the vsini row 1.86e-13
  adjoint row of the from-template form against autograd: 7.8e-12 ... 1.15e-10 of the
             absolute sums, at most 0.88 of the pair's bound (0.8 ... 2.1e-12 of the
             largest entry); contracted on the host with the tangent rows against the grid form's parameter components: 3.96e-15
  identity bands (nd = 1, nd = 3 with zero side taps): every output bit-equal to the call
             without matrices on regular-grid, Delaunay and MLP libraries
  value      within 1e-11 of engine.objective_fused under the same matrices (the bits on
             1 job of 7: the two kernels sum the normal equations in different orders,
             as they do without a band)
  rvs_bfgs_run_grad_fused_resol: the host machine's bits on 5 runs (up to 78 gradient rows)"""
import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG, gold_lib_dict
from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import chisq_grad_resol_truth as rtruth
import adjoint_row_resol_truth as art
import objective_adjoint_resol_restated as radj
import objective_grad_shapes as shapes
import test_bfgs_jac_gpu as tj
from test_bfgs_jac_gpu import setups   # noqa: F401 (fixture)
from test_nn_vjp_gpu import nets, libs, chain as nn_chain   # noqa: F401 (fixtures)
from test_nn_vjp_gpu import NAME as NN_NAME, TWIN_CONTRACTION_BOUND
from test_objective_grad_gpu import REL_ERR_BOUND, DEFECT
from test_objective_grad_resol_cpu import RESTATED_ROW_ERR, adjoint_row_cases

pytestmark = pytest.mark.gpu
J = len(truth.JOBS)
MEASURED_REL_ERR = 6.59e-13
GRAD_BOUND = 10 * MEASURED_REL_ERR
assert GRAD_BOUND <= REL_ERR_BOUND <= DEFECT
KEYS = dict(fused_gradient=True, resol_gradient=True)


def _rel(g, ref):
    return np.abs(g - ref) / np.maximum(np.abs(ref), 1e-6 * np.abs(ref).max())


def _job_of_spectrum(s):
    """the `job` of chisq_grad_resol_truth.width for spectrum s: widths 0.5 ... 1.9"""
    return 2 * s


def _batch(sds, mats=None, arms=(0, 1)):
    """SpecBatch of the spectra `sds` with mats[s][ia] (ResolMatrix or None) as
    SpecData.resolution"""
    from rvspecfit_amd import spec_fit
    from rvspecfit_amd.engine import SpecBatch
    return SpecBatch.from_specdata([
        [spec_fit.SpecData(x.name, x.lam, x.spec, x.espec, badmask=x.badmask,
                           resolution=None if mats is None else mats[s][ia])
         for ia, x in enumerate(sp) if ia in arms] for s, sp in enumerate(sds)])


@pytest.fixture(scope='module')
def setup(cases):
    from rvspecfit_amd import _lib, spec_inter, spec_fit
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    cfg = dict(GOLD_CONFIG, template_lib='golden://', **KEYS)
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, gold_lib_dict(n)), 'golden://')
    sds = truth.spectra(cases, spec_fit.SpecData)
    osds = truth.spectra(cases, orc.SpecData)
    mats = [rtruth.matrices(sp, _job_of_spectrum(s), spec_fit) for s, sp in enumerate(sds)]
    omats = [[R.mat for R in m] for m in mats]
    batch = _batch(sds, mats)
    plain = _batch(sds)
    libs = spec_inter.get_libs(batch.names, cfg)
    dev = batch.device
    f64 = dict(dtype=torch.float64, device=dev)
    return dict(cfg=cfg, sds=sds, osds=osds, mats=mats, omats=omats, batch=batch,
                plain=plain, libs=libs, dev=dev,
                idx=torch.tensor([j[0] for j in truth.JOBS], device=dev),
                vel=torch.tensor([j[1] for j in truth.JOBS], **f64),
                par=torch.tensor([j[2] for j in truth.JOBS], **f64),
                vs=torch.tensor([j[3] or 0.0 for j in truth.JOBS], **f64))


@pytest.fixture(scope='module')
def olibs():
    return {n: orc.Library(gold_lib_dict(n)) for n in ('gold_b', 'gold_r')}


def _fused(su, npoly, batch=None, resols=None, order=None, vsini_grad=False, vs=None,
           libs=None, resol_gradient=True, **kw):
    from rvspecfit_amd import engine
    sel = torch.arange(J, device=su['dev']) if order is None else torch.tensor(
        order, device=su['dev'])
    vs = su['vs'] if vs is None else vs
    return engine.objective_grad_fused(
        su['batch'] if batch is None else batch, su['libs'] if libs is None else libs,
        su['par'][sel].contiguous(), vs[sel].contiguous(), su['vel'][sel].contiguous(),
        npoly, True, su['idx'][sel].to(torch.int32).contiguous(), vsini_grad,
        resols=resols, resol_gradient=resol_gradient, **kw)


_truths = {}


def _truth(su, olibs, npoly, vsini_fit=False):
    """[(value, grad)] of JOBS under the spectra's own matrices, once"""
    key = (npoly, vsini_fit)
    if key not in _truths:
        # (vsini_fit: the jobs with rotation only)
        _truths[key] = [None if vsini_fit and not vs else
                        rtruth.chisq_and_grad(su['osds'][s], olibs, su['omats'][s], v, p,
                                              vs, npoly=npoly, vsini_fit=vsini_fit)
                        for s, v, p, vs in truth.JOBS]
    return _truths[key]


def _against(label, chi, grad, st, want, jobs, bound=None):
    bound = GRAD_BOUND if bound is None else bound
    worst = 0.0
    for j in jobs:
        val, g = want[j]
        assert int(st[j].item()) == 0
        e = _rel(grad[j], g)
        for k in range(len(g)):
            print('%s job %d comp %d truth %.12g fused %.12g rel err %.3g'
                  % (label, j, k, g[k], grad[j, k], e[k]))
        ev = abs(chi[j].item() - val) / max(abs(val), 1e3)
        print('%s job %d value %.15g truth %.15g (%.3g)' % (label, j, chi[j].item(), val, ev))
        assert ev <= 1e-11
        worst = max(worst, float(e.max()))
    print('%s largest relative gradient error %.3g (bound %.3g)' % (label, worst, bound))
    assert worst <= DEFECT, 'a defect to find, not a bound to set'
    assert worst <= bound
    return worst


# ---- 1. gradient and value against the truth ------------------------------------------------
@pytest.mark.parametrize('npoly', [5, 10])
def test_gradient_and_value_against_the_truth(setup, olibs, npoly):
    """the golden jobs under every spectrum's own matrices"""
    want = _truth(setup, olibs, npoly)
    chi, grad, st = _fused(setup, npoly)
    assert grad.shape == (J, 5)
    _against('npoly %d' % npoly, chi, grad.cpu().numpy(), st, want, truth.INSIDE)


LONG = dict(widths=(0.5, 0.8), nds=(17, 25))
_long = {}


def _long_case(npoly):
    """one arm of 1100 pixels on 2600 knots, two spectra under 17 and 25 diagonals, four
    jobs (two of them rotationally broadened): the device side and the truth, once"""
    if npoly in _long:
        return _long[npoly]
    from rvspecfit_amd import spec_fit
    import test_objective_grad_shapes_gpu as tg
    c = shapes.Case('resol-fine2600-p%d' % npoly, 'side', [(shapes.fine(2600), 1100)], npoly,
                    Rs=(None, 1.6), in_cell=False, seed=81)
    d = dict(tg._device(c))
    sds = shapes.specdata(c, spec_fit.SpecData)
    osds = shapes.specdata(c, orc.SpecData)
    mats = [[spec_fit.construct_resol_mat(sp[0].lam, width=w)]
            for sp, w in zip(sds, LONG['widths'])]
    assert tuple(rtruth.ndiag(m[0].mat) for m in mats) == LONG['nds']
    d['batch'] = _batch(sds, mats, arms=(0, ))
    d['plain'] = _batch(sds, None, arms=(0, ))
    with truth.banded_spline(shapes.BANDED_ABOVE):
        want = [rtruth.chisq_and_grad(osds[s], shapes.olibs(c), [mats[s][0].mat], vel, par,
                                      vs, npoly=npoly) for s, vel, par, vs in c.jobs]
    _long[npoly] = (c, d, want)
    return _long[npoly]


def _fused_case(c, d, batch=None, order=None, resols=None, **kw):
    from rvspecfit_amd import engine
    sel = torch.arange(len(c.jobs), device=d['vel'].device) if order is None else \
        torch.tensor(order, device=d['vel'].device)
    return engine.objective_grad_fused(
        d['batch'] if batch is None else batch, d['libs'], d['par'][sel].contiguous(),
        d['vs'][sel].contiguous(), d['vel'][sel].contiguous(), c.npoly, c.rbf,
        d['idx'][sel].contiguous(), c.vsini_grad, resols=resols, resol_gradient=True, **kw)


@pytest.mark.parametrize('npoly', [5, 10])
def test_long_arm_against_the_truth(npoly):
    """more than one pixel per thread, the band across the thread stride"""
    c, d, want = _long_case(npoly)
    assert d['batch'].arms[0].npix == 1100 > 2 * 512
    chi, grad, st = _fused_case(c, d)
    _against('long arm npoly %d' % npoly, chi, grad.cpu().numpy(), st, want,
             range(len(c.jobs)))


# ---- 2. the value is the value kernel's ---------------------------------------------------------
@pytest.mark.parametrize('npoly', [5, 10])
def test_value_is_the_value_kernels(setup, npoly):
    from rvspecfit_amd import engine
    su = setup
    chi, grad, st = _fused(su, npoly)
    ref, rst = engine.objective_fused(su['batch'], su['libs'], su['par'], su['vs'],
                                      su['vel'], npoly, True,
                                      su['idx'].to(torch.int32).contiguous())
    assert torch.equal(st, rst), (st, rst)
    same = 0
    for j in range(J):
        a, b = chi[j].item(), ref[j].item()
        same += a == b
        print('npoly %d job %d value %.17g objective_fused %.17g' % (npoly, j, a, b))
        assert abs(a - b) <= 1e-11 * max(abs(b), 1e3), (j, a, b)
    print('npoly %d: %d of %d values bit-equal' % (npoly, same, J))
    # the outside flag: job 5 outside the grid, job 6 a non-finite parameter
    assert chi[6].item() == 2 * 1000.0 * su['batch'].badchi == ref[6].item()
    assert not grad[6].any() and not grad[5, 1:].any()
    c, d, _ = _long_case(npoly)
    chi, grad, st = _fused_case(c, d)
    ref, rst = engine.objective_fused(d['batch'], d['libs'], d['par'], d['vs'], d['vel'],
                                      npoly, True, d['idx'])
    assert torch.equal(st, rst)
    assert ((chi - ref).abs() <= 1e-11 * ref.abs().clamp(min=1e3)).all(), (chi, ref)


# ---- 3. identity matrices ---------------------------------------------------------------------------
def _identity(batch, nd):
    """resols of identity bands of nd diagonals (zero side taps), one per spectrum"""
    from rvspecfit_amd import engine
    out = []
    for arm in batch.arms:
        taps = np.zeros((batch.S, arm.npix, nd))
        taps[:, :, (nd - 1) // 2] = 1.0
        out.append(engine.make_resol(taps, nd, batch.S, batch.device))
    return out


@pytest.mark.parametrize('npoly', [5, 10])
def test_identity_on_regular_grids(setup, npoly):
    """nd = 1 and nd = 3 with zero side taps: every output the bits of the call without
    matrices, with and without the vsini row; on the long arm too"""
    su = setup
    for vg in (False, True):
        ref = _fused(su, npoly, batch=su['plain'], vsini_grad=vg)
        for nd in (1, 3):
            got = _fused(su, npoly, batch=su['plain'], resols=_identity(su['plain'], nd),
                         vsini_grad=vg)
            for a, b, what in zip(got, ref, ('value', 'gradient', 'status')):
                assert torch.equal(a, b), (npoly, vg, nd, what, a, b)
    c, d, _ = _long_case(npoly)
    ref = _fused_case(c, d, batch=d['plain'])
    for nd in (1, 3):
        got = _fused_case(c, d, batch=d['plain'], resols=_identity(d['plain'], nd))
        for a, b in zip(got, ref):
            assert torch.equal(a, b), (npoly, nd)


def test_identity_on_delaunay_libraries(setup, setups):   # noqa: F811
    from rvspecfit_amd import spec_inter
    su = setup
    libs = spec_inter.get_libs(su['plain'].names, setups['tri']['cfg'])
    assert libs['gold_b'].kind == 'triangulation'
    kw = dict(batch=su['plain'], libs=libs, tri_gradient=True)
    ref = _fused(su, 10, vsini_grad=True, **kw)
    assert ref[1].abs().sum().item() > 0
    for nd in (1, 3):
        got = _fused(su, 10, vsini_grad=True, resols=_identity(su['plain'], nd), **kw)
        for a, b in zip(got, ref):
            assert torch.equal(a, b), nd


def test_identity_on_mlp_libraries(nn_chain):   # noqa: F811
    from rvspecfit_amd import engine
    su = nn_chain
    call = lambda rs: engine.objective_grad_fused(      # noqa: E731
        su['batch'], {NN_NAME: su['lib']}, su['P'], su['rot'], su['vel'], 5, True, None,
        True, nn_gradient=True, resols=rs, resol_gradient=True)
    ref = call(None)
    assert ref[1].abs().sum().item() > 0
    for nd in (1, 3):
        got = call(_identity(su['batch'], nd))
        for a, b in zip(got, ref):
            assert torch.equal(a, b), nd


# ---- 4. the widest band, and what is refused -----------------------------------------------------------
def test_33_diagonals_pass_the_truth_and_35_are_refused(setup, olibs):
    """the golden matrices padded with zero diagonals to nd = 33 (the kernel then runs 33
    products per pixel): the truth of test 1; nd = 35 and an arm one double beyond the
    LDS limit raise and return RVS_E_ARG"""
    from rvspecfit_amd import _lib, engine
    su = setup
    b = su['plain']

    def padded(nd):
        return [engine.make_resol(np.stack([radj.band(su['omats'][s][ia], nd)
                                            for s in range(b.S)]), nd, b.S, b.device)
                for ia in range(len(b.arms))]
    chi, grad, st = _fused(su, 10, batch=b, resols=padded(33))
    _against('nd 33', chi, grad.cpu().numpy(), st, _truth(su, olibs, 10), truth.INSIDE)
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*gold_b.*35 diagonals.*33'):
        _fused(su, 10, batch=b, resols=padded(35))
    # 2 npix + nd - 1 <= ntp: 131 pixels on 263 knots take one diagonal, not three
    import test_objective_grad_shapes_gpu as tg
    c = shapes.case('p10-cut263')
    d = tg._device(c)
    ok = _lib.lib().rvs_objective_grad_resol_ok
    assert ok(10, 131, 263, 4, 1, 0) == 1 and ok(10, 131, 263, 4, 3, 0) == 0
    _fused_case(c, d, resols=_identity(d['batch'], 1))
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*2 npix \+ nd - 1 <= ntp'):
        _fused_case(c, d, resols=_identity(d['batch'], 3))


# ---- 5. the transposed band alone: the adjoint row of the from-template form ----------------------------
def test_adjoint_row_under_a_matrix(cases, setup, olibs):
    """rvs_objective_grad_from_template_resol on the rows rvs_template_polylinear writes
    for the golden jobs: value, velocity and vsini components the bits of
    rvs_objective_grad_resol (everything behind the row is one text); tbar contracted on
    the host with the tangent rows against the kernel's parameter components, within the
    bound test_nn_vjp_gpu.py holds the same comparison to without matrices; and tbar
    itself against float64 autograd with the device's own template row as the leaf
    through the dense matrix, relative to the absolute sum behind each entry, within
    10 x the restatement's own error plus the row's change under one ulp of x (see the
    module's text)"""
    from rvspecfit_amd import engine
    su = setup
    jobs = list(truth.INSIDE)
    sel = torch.tensor(jobs, device=su['dev'])
    par, vs, vel = (su[k][sel].contiguous() for k in ('par', 'vs', 'vel'))
    js = su['idx'][sel].to(torch.int32).contiguous()
    chi, grad, st = engine.objective_grad_fused(su['batch'], su['libs'], par, vs, vel, 10,
                                                True, js, True, resol_gradient=True)
    ls = [su['libs'][arm.name] for arm in su['batch'].arms]
    rows = [lib.eval_batch_grad(par) for lib in ls]
    o, gvv, st2, tbars, _ = engine.objective_grad_from_template(
        su['batch'], su['libs'], [r[0][:, 0].contiguous() for r in rows],
        [r[1] for r in rows], vs, vel, 10, True, js, True, resol_gradient=True)
    assert torch.equal(st, st2)
    assert torch.equal(o, chi) and torch.equal(gvv, grad[:, [0, 5]])
    host = sum(torch.einsum('jn,jkn->jk', tb, r[0][:, 1:]) for tb, r in zip(tbars, rows))
    ec = shapes.rel_err(host.cpu().numpy(), grad[:, 1:5].cpu().numpy()).max()
    print('tbar contracted on the host against the parameter components: %.3g' % ec)
    assert ec <= TWIN_CONTRACTION_BOUND
    t_rows = {(j, ia): rows[ia][0][i, 0].cpu().numpy()
              for i, j in enumerate(jobs) for ia in range(len(ls))}
    pos = {j: i for i, j in enumerate(jobs)}
    bad = []
    for j, ia, a, (c, gv, want, terms, cond), moved in adjoint_row_cases(
            cases, olibs, 10, t_rows):
        assert cond < 100
        tb = tbars[ia][pos[j]].cpu().numpy()
        e = art.row_error(tb, want, terms)
        bound = 10 * RESTATED_ROW_ERR + moved
        print('job %d arm %d adjoint row: error %.3g of the absolute sums (%.3g of the '
              'largest entry %.3g); bound %.3g = 10 x %.3g + %.3g for one ulp of x; the '
              'restatement on the same row %.3g'
              % (j, ia, e, np.abs(tb - want).max() / np.abs(want).max(),
                 np.abs(want).max(), bound, RESTATED_ROW_ERR, moved,
                 art.row_error(a['tbar'], want, terms)))
        if not e <= bound:
            bad.append((j, ia, e, bound))
    assert not bad, bad


# ---- 6. mixed arms, per-spectrum matrices, determinism ----------------------------------------------------
def test_mixed_arms_permutation_and_repeats(setup):
    """a matrix on the blue arm only beside an arm without one; a job alone, in the batch
    and in a permuted batch has the same bits; two runs are bit-equal"""
    su = setup
    one = _batch(su['sds'], [[m[0], None] for m in su['mats']])
    lnstep = su['libs']['gold_b'].lnstep
    vs = torch.tensor([r * truth.C_KMS * lnstep for r in
                       (0.4, 1.6, 3.0005, 9.3, 0.0, 0.7, 1.9996)], dtype=torch.float64,
                      device=su['dev'])
    perm = [4, 2, 6, 0, 5, 1, 3]
    sel = torch.tensor(perm, device=su['dev'])
    for batch in (su['batch'], one):
        chi, grad, st = _fused(su, 10, batch=batch, vsini_grad=True, vs=vs)
        chi2, grad2, st2 = _fused(su, 10, batch=batch, vsini_grad=True, vs=vs)
        assert torch.equal(grad, grad2) and torch.equal(chi, chi2) and torch.equal(st, st2)
        chi3, grad3, st3 = _fused(su, 10, batch=batch, order=perm, vsini_grad=True, vs=vs)
        assert torch.equal(grad3, grad[sel]) and torch.equal(chi3, chi[sel])
        assert torch.equal(st3, st[sel])
        for j in (0, 3, 5):
            c1, g1, s1 = _fused(su, 10, batch=batch, order=[j], vsini_grad=True, vs=vs)
            assert torch.equal(c1[0], chi[j]) and torch.equal(g1[0], grad[j])
            assert torch.equal(s1[0], st[j])
    # the red arm of `one` is a band of one diagonal: its matrix-free bits, so the call
    # differs from the call under both matrices and from the one under none
    a = _fused(su, 10, batch=one)[0]
    assert not torch.equal(a[:5], _fused(su, 10)[0][:5])
    assert not torch.equal(a[:5], _fused(su, 10, batch=su['plain'])[0][:5])


# ---- 7. the vsini row under a matrix --------------------------------------------------------------------------
def test_vsini_row_against_the_truth(setup, olibs):
    su = setup
    jobs = [j for j in truth.INSIDE if truth.JOBS[j][3]]
    assert jobs
    want = _truth(su, olibs, 10, vsini_fit=True)
    chi, grad, st = _fused(su, 10, vsini_grad=True)
    assert grad.shape == (J, 6)
    grad = grad.cpu().numpy()
    _against('vsini row', chi, grad, st, want, jobs)
    assert all(grad[j, 5] != 0.0 for j in jobs)
    # without rotation the component is exactly 0
    assert all(grad[j, 5] == 0.0 for j in truth.INSIDE if not truth.JOBS[j][3])


# ---- 8. the rounds in the library ---------------------------------------------------------------------------------
def _stars(cases, S, width=0.9):
    """S fake stars on the blue golden arm, each under a matrix of its own width"""
    from rvspecfit_amd import spec_fit
    return [[spec_fit.SpecData(sd.name, sd.lam, sd.spec, sd.espec,
                               resolution=spec_fit.construct_resol_mat(
                                   sd.lam, width=width + 0.1 * s))
             for sd in sp] for s, sp in enumerate(tj._fake_stars(cases, S))]


def test_run_grad_fused_resol_equals_host_machine(cases, setup, setups):   # noqa: F811
    """S = 5, n = 6, rows in chunks of 3: rvs_bfgs_run_grad_fused_resol against
    minimize_lockstep_native(jac=True) over GradChain(fused=True).rows, bit for bit"""
    from rvspecfit_amd import bfgs, optimizer, vel_fit
    from rvspecfit_amd.engine import SpecBatch
    S = 5
    su = dict(setups['grid'], batch=SpecBatch.from_specdata(_stars(cases, S)),
              cfg=dict(setups['grid']['cfg'], **KEYS))
    assert all(a.resol is not None and a.resol['nd'] <= 33 for a in su['batch'].arms)
    pobj, _ = tj._objective(su, S, pd0=dict(teff=5200., logg=2.3, feh=-0.8, alpha=0.2,
                                            vsini=5.0))
    assert pobj.native and pobj.resol_gradient
    cols = ['vel', 'vsini'] + su['names']
    x0 = torch.tensor([[30.0 - 20 * s, 5.0, 5200., 2.3, -0.8, 0.2] for s in range(S)],
                      dtype=torch.float64, device=su['batch'].device)
    H0 = vel_fit.get_hess_inv(cols)
    chain = optimizer.GradChain(pobj, cap=3, fused=True)
    assert chain.fused_resol and chain.cap == 3
    assert not hasattr(chain, 'arms') and not hasattr(chain, 'point_work')
    dev_r = bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=H0, jac=True, chain=chain)
    host = bfgs.minimize_lockstep_native(chain.rows, x0.cpu().numpy(), hess_inv0=H0,
                                         jac=True)
    keys = ('x', 'fun', 'nit', 'nfev', 'njev', 'status')
    d = {k: dev_r[k].cpu().numpy() for k in keys}
    print('device nit', d['nit'], 'nfev', d['nfev'], 'njev', d['njev'], 'status',
          d['status'], 'rounds', dev_r['rounds'], 'calls', dev_r['calls'])
    print('host   nit', host['nit'], 'nfev', host['nfev'], 'njev', host['njev'], 'status',
          host['status'])
    for k in keys:
        assert np.array_equal(d[k], np.asarray(host[k])), k
    assert d['njev'].max() > 3
    f0 = chain.rows(np.arange(S), x0.cpu().numpy())[:, 0]
    assert (d['fun'] <= f0).all()
    # the rows are the chain's rows under the same matrices, to the bound
    # tests/test_objective_grad_gpu.py holds the fused rows and the chain's to
    ref = optimizer.GradChain(pobj, cap=3).rows(np.arange(S), x0.cpu().numpy())
    got = chain.rows(np.arange(S), x0.cpu().numpy())
    for s in range(S):
        assert abs(got[s, 0] - ref[s, 0]) <= 1e-11 * max(abs(ref[s, 0]), 1e3)
        e = _rel(got[s, 1:], ref[s, 1:]).max()
        print('run %d rows: fused against the chain %.3g' % (s, e))
        assert e <= REL_ERR_BOUND, (s, got[s], ref[s])


def test_process_with_both_keys(cases, setups):   # noqa: F811
    """8 fake stars under resolParams: finite records, chisq no higher than the chain's
    polish from the same simplex optimum + 1e-6 |chisq|"""
    from rvspecfit_amd import spec_fit, vel_fit
    from rvspecfit_amd.engine import SpecBatch
    su = setups['grid']
    S = 8
    batch = SpecBatch.from_specdata(tj._fake_stars(cases, S))
    rp = {a.name: spec_fit.construct_resol_mat(a.lam_host, width=1.0) for a in batch.arms}
    pd0 = dict(teff=np.full(S, 5200.), logg=np.full(S, 2.3), feh=np.full(S, -0.8),
               alpha=np.full(S, 0.2), vsini=np.full(S, 5.0))
    out = {}
    for fused in (False, True):
        cfg = dict(su['cfg'], second_minimizer=True, second_minimizer_jac=True,
                   resol_gradient=True, fused_gradient=fused)
        out[fused] = vel_fit.process(batch, dict(pd0), options=dict(npoly=tj.NPOLY),
                                     config=cfg, resolParams=rp)
    a, b = out[True], out[False]
    assert a['bfgs']['jac'] is True and a['bfgs']['fused'] is True
    assert b['bfgs']['jac'] is True and b['bfgs']['fused'] is False
    assert (a['bfgs']['njev'] >= 1).all()
    for k in ('vel', 'vel_err', 'chisq', 'vsini'):
        assert torch.isfinite(a[k]).all(), k
    for k in su['names']:
        assert torch.isfinite(a['param'][k]).all(), k
    ca, cb = a['chisq'].cpu().numpy(), b['chisq'].cpu().numpy()
    print('chisq fused', ca, 'chain', cb, 'fused - chain', ca - cb, 'nit',
          a['bfgs']['nit'], b['bfgs']['nit'], 'status', a['bfgs']['status'],
          b['bfgs']['status'])
    assert (ca <= cb + 1e-6 * np.abs(cb)).all(), ca - cb


# ---- 9. refusals with both keys set -----------------------------------------------------------------------------------
def test_refusals_with_both_keys(cases, setup):
    """from get_chisq_grad and from process: a band wider than 33 diagonals names the key,
    the arm and the limit; the Fisher matrix, the Levenberg-Marquardt polish, the
    joint-epoch fit, fast_interp and a grid set stay refused"""
    from rvspecfit_amd import engine, spec_fit, vel_fit
    from rvspecfit_amd.engine import SpecBatch
    su = setup
    _, vel, par, _ = truth.JOBS[0]
    sd = su['sds'][0]
    cfg = dict(su['cfg'])
    pcfg = dict(cfg, second_minimizer=True, second_minimizer_jac=True)
    S = 2
    stars = tj._fake_stars(cases, S)
    pbatch = SpecBatch.from_specdata(stars)
    pd0 = dict(teff=np.full(S, 5200.), logg=np.full(S, 2.3), feh=np.full(S, -0.8),
               alpha=np.full(S, 0.2), vsini=np.full(S, 5.0))
    opt = dict(npoly=10)
    wide = {x.name: spec_fit.construct_resol_mat(x.lam, width=4.0) for x in sd}
    assert all(rtruth.ndiag(R.mat) > 33 for R in wide.values())
    pwide = {a.name: spec_fit.construct_resol_mat(a.lam_host, width=4.0)
             for a in pbatch.arms}
    rp = {x.name: spec_fit.construct_resol_mat(x.lam, width=0.5) for x in sd}
    prp = {a.name: spec_fit.construct_resol_mat(a.lam_host, width=0.5)
           for a in pbatch.arms}
    pat = r'(?s)fused_gradient.*resol_gradient.*gold_b.*diagonals.*at most 33'
    with pytest.raises(ValueError, match=pat):
        spec_fit.get_chisq_grad(sd, vel, par, options=opt, config=cfg, resol_params=wide)
    with pytest.raises(ValueError, match=pat):
        vel_fit.process(pbatch, dict(pd0), options=opt, config=pcfg, resolParams=pwide)
    # the narrow band goes through both
    spec_fit.get_chisq_grad(sd, vel, par, options=opt, config=cfg, resol_params=rp)
    # without resol_gradient the old refusal, word for word
    old = dict(cfg, resol_gradient=False)
    with pytest.raises(ValueError) as e:
        spec_fit.get_chisq_grad(sd, vel, par, options=opt, config=old, resol_params=rp)
    assert str(e.value) == ("config['fused_gradient'] does not go with a resolution matrix "
                            "(resol_params / the spectra's own, arm gold_b)")
    with pytest.raises(ValueError, match='fused_gradient.*resolution matrix'):
        vel_fit.process(pbatch, dict(pd0), options=opt,
                        config=dict(pcfg, resol_gradient=False), resolParams=prp)
    # what needs tangent rows, and what the kernel has no form for
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*Fisher'):
        spec_fit.get_chisq_fisher(sd, vel, par, options=opt, config=cfg, resol_params=rp)
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*second_minimizer_lm'):
        vel_fit.process(pbatch, dict(pd0), options=opt, resolParams=prp,
                        config=dict(cfg, second_minimizer=True, second_minimizer_lm=True))
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*epochs'):
        vel_fit.process_epochs(pbatch, np.array([0, 0]),
                               {k: v[:1] for k, v in pd0.items()}, np.zeros(2),
                               options=opt, config=cfg, resolParams=prp)
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*fast_interp'):
        spec_fit.get_chisq_grad(sd, vel, par, options=opt, config=cfg, resol_params=rp,
                                fast_interp=True)
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*fast_interp'):
        vel_fit.process(pbatch, dict(pd0), options=dict(npoly=10, fast_interp=True),
                        config=pcfg, resolParams=prp)
    lam = stars[0][0].lam
    gset = SpecBatch([engine.ArmData(
        'gold_b', [lam, lam[:-7]], np.stack([stars[0][0].spec, stars[1][0].spec]),
        np.stack([stars[0][0].espec, stars[1][0].espec]), device='cuda',
        grid_id=np.arange(2, dtype=np.int32))])
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*grid set'):
        vel_fit.process(gset, dict(pd0), options=opt, config=pcfg)
