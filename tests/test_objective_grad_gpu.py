"""rvs_objective_grad (csrc/objective_grad.hip: value and gradient in one kernel per
(job, arm), by the adjoint method) and the interfaces above it -- against the float64
autograd truth of tests/chisq_grad_truth.py, against the gradient chain
(engine.chisq_point_grad, spec_fit.chisq_grad_jobs) and the value kernel
(engine.objective_fused), and through optimizer.GradChain(fused=True),
rvs_bfgs_run_grad_fused and vel_fit.process with config['fused_gradient'].

Shapes: the 7 JOBS of chisq_grad_truth on the golden arms (ntp 977 and 781, both odd;
npix 401 and 301; 16 vertices), and small spectra built from them.

Largest error of the fused gradient against the truth seen on an MI355X on the first
run, over the in-cell jobs, relative to max(|g_k|, 1e-6 |g|_inf):
    3.9e-12 (npoly 5), 4.72e-12 (npoly 10); npoly 16 is refused by the kernel
Both on job 1 (S/N 10, a gradient near its zero: value -315, components -0.04, 9e-4,
-0.55, 4.8, -0.68), on d/dalpha: the contraction sum_n tbar_n t_n g_dn over ~1000
knots cancels there more than the chain's sum over the pixels; the other jobs are at
1e-13.  Against the chain the same job measures 4.1e-12, the others <= 2.1e-13.
The bound is 10 x that: the sums have a fixed order, the factor covers another
machine's exp / log and the host BLAS under the truth, as test_chisq_grad_gpu.py
argues.  (A measured error above 5e-10, the best case of the forward difference this
replaces, would be a defect, not a bound.)  The chain measures 5.8e-13."""
import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG, gold_lib_dict
from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import vsini_grad_truth as vtruth
import test_bfgs_jac_gpu as tj
from test_bfgs_jac_gpu import setups   # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
J = len(truth.JOBS)
MEASURED_REL_ERR = 4.72e-12
REL_ERR_BOUND = 10 * MEASURED_REL_ERR
DEFECT = 5e-10


def _rel(g, ref):
    return np.abs(g - ref) / np.maximum(np.abs(ref), 1e-6 * np.abs(ref).max())


@pytest.fixture(scope='module')
def setup(cases):
    from rvspecfit_amd import _lib, spec_inter, spec_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    cfg = dict(GOLD_CONFIG, template_lib='golden://')
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, gold_lib_dict(n)), 'golden://')
    sds = truth.spectra(cases, spec_fit.SpecData)
    batch = SpecBatch.from_specdata(sds)
    libs = spec_inter.get_libs(batch.names, cfg)
    dev = batch.device
    f64 = dict(dtype=torch.float64, device=dev)
    return dict(cfg=cfg, sds=sds, batch=batch, libs=libs, dev=dev,
                idx=torch.tensor([j[0] for j in truth.JOBS], device=dev),
                vel=torch.tensor([j[1] for j in truth.JOBS], **f64),
                par=torch.tensor([j[2] for j in truth.JOBS], **f64),
                vs=torch.tensor([j[3] or 0.0 for j in truth.JOBS], **f64))


@pytest.fixture(scope='module')
def olibs():
    return {n: orc.Library(gold_lib_dict(n)) for n in ('gold_b', 'gold_r')}


def _fused(su, npoly, order=None, vsini_grad=False, vs=None):
    from rvspecfit_amd import engine
    sel = torch.arange(J, device=su['dev']) if order is None else torch.tensor(
        order, device=su['dev'])
    vs = su['vs'] if vs is None else vs
    return engine.objective_grad_fused(
        su['batch'], su['libs'], su['par'][sel].contiguous(), vs[sel].contiguous(),
        su['vel'][sel].contiguous(), npoly, True,
        su['idx'][sel].to(torch.int32).contiguous(), vsini_grad)


def _chain(su, npoly, vsini_grad=False, vs=None, vel=None, par=None, idx=None):
    from rvspecfit_amd import spec_fit
    return spec_fit.chisq_grad_jobs(
        su['batch'], su['idx'] if idx is None else idx,
        su['vel'] if vel is None else vel, su['par'] if par is None else par,
        su['vs'] if vs is None else vs, dict(npoly=npoly), su['cfg'],
        vsini_grad=vsini_grad)


# ---- 1. the gradient against the truth ----------------------------------------------
@pytest.mark.parametrize('npoly', [5, 10])
def test_gradient_against_the_truth(cases, setup, olibs, npoly):
    want = truth.truth_jobs(cases, olibs, npoly)
    chi, grad, st = _fused(setup, npoly)
    grad = grad.cpu().numpy()
    assert grad.shape == (J, 5)
    worst = 0.0
    for j in truth.INSIDE:
        val, g = want[j]
        assert int(st[j].item()) == 0
        e = _rel(grad[j], g)
        for k in range(5):
            print('npoly %d job %d comp %d truth %.12g fused %.12g rel err %.3g'
                  % (npoly, j, k, g[k], grad[j, k], e[k]))
        print('npoly %d job %d value %.12g truth %.12g' % (npoly, j, chi[j].item(), val))
        assert abs(chi[j].item() - val) <= 1e-7 * abs(val)
        worst = max(worst, float(e.max()))
    print('npoly %d largest relative error %.3g (bound %.3g)'
          % (npoly, worst, REL_ERR_BOUND))
    assert worst <= DEFECT, 'a defect to find, not a bound to set'
    assert worst <= REL_ERR_BOUND


def test_npoly_16_is_refused(setup):
    """the kernel covers npoly 1..10: beyond, ValueError naming the option and the key,
    and RVS_E_ARG from the library"""
    from rvspecfit_amd import _lib
    with pytest.raises(ValueError, match=r'fused_gradient.*npoly'):
        _fused(setup, 16)
    assert _lib.lib().rvs_objective_grad_ok(16, 401, 977, 4, 0) == 0


# ---- 2. agreement with the existing paths ---------------------------------------------
@pytest.mark.parametrize('npoly', [5, 10])
def test_agreement_with_chain_and_value_kernel(setup, npoly):
    from rvspecfit_amd import engine
    su = setup
    chi, grad, st = _fused(su, npoly)
    cchi, cgrad, cst = _chain(su, npoly)
    assert torch.equal(st, cst), (st, cst)
    grad, cgrad = grad.cpu().numpy(), cgrad.cpu().numpy()
    for j in range(5):
        e = _rel(grad[j], cgrad[j])
        print('npoly %d job %d max rel err against the chain %.3g' % (npoly, j, e.max()))
        assert e.max() <= REL_ERR_BOUND
    # job 5, outside the grid: no parameter component, the chain's velocity component
    assert not grad[5, 1:].any() and not cgrad[5, 1:].any()
    print('outside job d/dvel fused %.12g chain %.12g' % (grad[5, 0], cgrad[5, 0]))
    assert abs(grad[5, 0] - cgrad[5, 0]) <= REL_ERR_BOUND * abs(cgrad[5, 0])
    # job 6, a non-finite mapped parameter: the penalty and no gradient
    assert chi[6].item() == 2 * 1000.0 * su['batch'].badchi == cchi[6].item()
    assert not grad[6].any()
    ref, rst = engine.objective_fused(su['batch'], su['libs'], su['par'], su['vs'],
                                      su['vel'], npoly, True,
                                      su['idx'].to(torch.int32).contiguous())
    assert torch.equal(st, rst)
    for j in range(J):
        a, b = chi[j].item(), ref[j].item()
        print('npoly %d job %d value %.12g objective_fused %.12g chain %.12g'
              % (npoly, j, a, b, cchi[j].item()))
        assert abs(a - b) <= 1e-11 * max(abs(b), 1e3), (j, a, b)


# ---- 3. the vsini row -------------------------------------------------------------------
def test_vsini_row(setup):
    """all components against chisq_grad_jobs(vsini_grad=True) on the chain: R < 1,
    1 < R < 2, R within 1e-3 of an integer, R > 8 (wider than the value kernel's
    register-window FIR), and vsini = 0, where the component is exactly 0"""
    su = setup
    lnstep = su['libs']['gold_b'].lnstep
    Rs = [0.4, 1.6, 3 + 5e-4, 9.3, 0.0, 0.7, 2 - 4e-4]
    vs = torch.tensor([r * vtruth.C_KMS * lnstep for r in Rs], dtype=torch.float64,
                      device=su['dev'])
    chi, grad, st = _fused(su, 10, vsini_grad=True, vs=vs)
    cchi, cgrad, cst = _chain(su, 10, vsini_grad=True, vs=vs)
    assert grad.shape == (J, 6) and torch.equal(st, cst)
    grad, cgrad = grad.cpu().numpy(), cgrad.cpu().numpy()
    for j in range(5):
        e = _rel(grad[j], cgrad[j])
        print('R %.4f job %d d/dvsini fused %.12g chain %.12g max rel err %.3g'
              % (Rs[j], j, grad[j, 5], cgrad[j, 5], e.max()))
        assert abs(chi[j].item() - cchi[j].item()) <= 1e-11 * max(abs(cchi[j].item()), 1e3)
        assert e.max() <= REL_ERR_BOUND
    assert grad[4, 5] == 0.0 and cgrad[4, 5] == 0.0
    assert grad[0, 5] != 0.0 and grad[3, 5] != 0.0
    # outside the grid the parameters drop out, vsini does not
    assert not grad[5, 1:5].any()
    print('outside job d/dvsini fused %.12g chain %.12g' % (grad[5, 5], cgrad[5, 5]))
    assert abs(grad[5, 5] - cgrad[5, 5]) <= REL_ERR_BOUND * max(
        abs(cgrad[5, 5]), 1e-6 * np.abs(cgrad[5]).max())
    assert not grad[6].any()


# ---- 4. the transposed resampling ---------------------------------------------------------
def test_transposed_resampling(cases, olibs):
    """a spectrum whose pixels come in close pairs and triples (several pixels in one
    knot interval, runs of empty intervals between them) and whose first / last pixel
    falls, at the job's velocity, into the template's first / last knot interval"""
    from rvspecfit_amd import engine, spec_fit, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    vel, par = 37.3, (5000.0, 2.2, -1.0, 0.2)
    f = np.sqrt((1 - vel / truth.C_KMS) / (1 + vel / truth.C_KMS))
    sds, osds = [], []
    for name, tag in (('gold_b', 'c0'), ('gold_r', 'c2')):
        kn = olibs[name].lam
        lam0 = cases['%s/%s/lam' % (tag, name)]
        # clusters of 2 or 3 pixels 0.02 knot intervals apart, every 7th interval
        x = [(kn[0] + 0.3 * (kn[1] - kn[0])) / f]
        for i in range(3, len(kn) - 3, 7):
            h = kn[i + 1] - kn[i]
            for c in range(2 + (i // 7) % 2):
                x.append((kn[i] + (0.4 + 0.02 * c) * h) / f)
        x.append((kn[-2] + 0.6 * (kn[-1] - kn[-2])) / f)
        x = np.array(x)
        assert 2 * len(x) <= len(kn)
        spec = np.interp(x, lam0, cases['%s/%s/spec' % (tag, name)])
        espec = np.interp(x, lam0, cases['%s/%s/espec' % (tag, name)])
        sds.append(spec_fit.SpecData(name, x, spec, espec))
        osds.append(orc.SpecData(name, x, spec, espec))
        pos = np.searchsorted(kn, x * f, 'right') - 1
        assert pos[0] == 0 and pos[-1] == len(kn) - 2
        assert np.bincount(pos).max() == 3 and (np.diff(pos) >= 4).any()
    batch = SpecBatch.from_specdata([sds])
    cfg = dict(GOLD_CONFIG, template_lib='golden://')
    libs = spec_inter.get_libs(batch.names, cfg)
    f64 = dict(dtype=torch.float64, device=batch.device)
    chi, grad, st = engine.objective_grad_fused(
        batch, libs, torch.tensor([par], **f64), None, torch.tensor([vel], **f64), 10)
    val, g = truth.chisq_and_grad(osds, olibs, vel, par, None, npoly=10)
    e = _rel(grad[0].cpu().numpy(), g)
    print('clustered pixels: value %.12g truth %.12g gradient %s truth %s rel err %s'
          % (chi[0].item(), val, grad[0].cpu().numpy(), g, e))
    assert int(st[0].item()) == 0
    assert abs(chi[0].item() - val) <= 1e-7 * abs(val)
    assert e.max() <= REL_ERR_BOUND


# ---- 5. determinism -------------------------------------------------------------------------
def test_determinism(setup):
    lnstep = setup['libs']['gold_b'].lnstep
    vs = torch.tensor([r * vtruth.C_KMS * lnstep for r in
                       (0.4, 1.6, 3.0005, 9.3, 0.0, 0.7, 1.9996)], dtype=torch.float64,
                      device=setup['dev'])
    chi, grad, st = _fused(setup, 10, vsini_grad=True, vs=vs)
    chi2, grad2, st2 = _fused(setup, 10, vsini_grad=True, vs=vs)
    assert torch.equal(grad, grad2) and torch.equal(chi, chi2) and torch.equal(st, st2)
    perm = [4, 2, 6, 0, 5, 1, 3]
    chi3, grad3, st3 = _fused(setup, 10, perm, vsini_grad=True, vs=vs)
    sel = torch.tensor(perm, device=setup['dev'])
    assert torch.equal(grad3, grad[sel]) and torch.equal(chi3, chi[sel])
    assert torch.equal(st3, st[sel])


# ---- 6. the optimiser ------------------------------------------------------------------------
def test_fused_rows_against_the_chains(setups):   # noqa: F811
    """GradChain(fused=True).rows against the chain's rows on the row cases of
    test_bfgs_jac_gpu.py (free and fixed parameters, priors, vsini clamps): value within
    1e-11 max(|f|, 1e3), gradient within the bound of test 1"""
    from rvspecfit_amd import optimizer
    su = setups['grid']
    for kw, rows in tj._row_cases(su):
        pobj, _ = tj._objective(su, 3, **kw)
        fused = optimizer.GradChain(pobj, fused=True)
        chain = optimizer.GradChain(pobj)
        assert not hasattr(fused, 'arms') and not hasattr(fused, 'point_work')
        idx = np.array([r[1] for r in rows], dtype=np.int64)
        X = np.array([r[2] for r in rows], dtype=np.float64)
        F, C = fused.rows(idx, X), chain.rows(idx, X)
        assert F.shape == C.shape == (len(rows), X.shape[1] + 1)
        for j, (label, s, x, loose) in enumerate(rows):
            print(label, 'fused', F[j], 'chain', C[j])
            if 'out of range' in label or 'non-finite' in label:
                assert F[j, 0] == 1e30 and not F[j, 1:].any()
                continue
            assert abs(F[j, 0] - C[j, 0]) <= 1e-11 * max(abs(C[j, 0]), 1e3)
            assert _rel(F[j, 1:], C[j, 1:]).max() <= REL_ERR_BOUND, label


@pytest.fixture(scope='module')
def nm_optimum(setups):   # noqa: F811
    return tj._start(setups['grid'], 8)


def _fused_pair(su, S, x0, H0, cap=None, **kw):
    from rvspecfit_amd import bfgs, optimizer
    pobj, args = tj._objective(su, S, **kw)
    chain = optimizer.GradChain(pobj, cap=cap, fused=True)
    dev_r = bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=H0, jac=True, chain=chain)
    host = bfgs.minimize_lockstep_native(chain.rows, x0.cpu().numpy(), hess_inv0=H0,
                                         jac=True)
    return pobj, chain, dev_r, host


KEYS = ('x', 'fun', 'nit', 'nfev', 'njev', 'status')


def _bit_equal(dev_r, host):
    d = {k: dev_r[k].cpu().numpy() for k in KEYS}
    print('device nit', d['nit'], 'nfev', d['nfev'], 'njev', d['njev'], 'status',
          d['status'], 'rounds', dev_r['rounds'], 'calls', dev_r['calls'])
    print('host   nit', host['nit'], 'nfev', host['nfev'], 'njev', host['njev'],
          'status', host['status'])
    for k in KEYS:
        assert np.array_equal(d[k], np.asarray(host[k])), k
    return d


def test_run_grad_fused_equals_host_machine(setups, nm_optimum):   # noqa: F811
    """S = 8, n = 6: rvs_bfgs_run_grad_fused against minimize_lockstep_native(jac=True)
    over the same fused rows, bit for bit, also under permuted spectra"""
    from rvspecfit_amd import bfgs, vel_fit
    su = setups['grid']
    S = 8
    cols = ['vel', 'vsini'] + su['names']
    x0 = tj._x0(nm_optimum, su['names'], S, cols)
    H0 = vel_fit.get_hess_inv(cols)
    pobj, chain, dev_r, host = _fused_pair(su, S, x0, H0)
    d = _bit_equal(dev_r, host)
    assert d['njev'].max() > 3
    f0 = chain.rows(np.arange(S), x0.cpu().numpy())[:, 0]
    assert (d['fun'] <= f0).all()
    perm = [4, 2, 6, 0, 7, 5, 1, 3]
    sub = dict(su, batch=su['batch'].subset(torch.tensor(perm, device='cuda')),
               sds=[su['sds'][i] for i in perm])
    pobj2, _ = tj._objective(sub, S)
    from rvspecfit_amd import optimizer
    r2 = bfgs.minimize_lockstep_device(pobj2, x0[perm].contiguous(), hess_inv0=H0,
                                       jac=True,
                                       chain=optimizer.GradChain(pobj2, fused=True))
    for k in KEYS:
        assert np.array_equal(r2[k].cpu().numpy(), d[k][perm]), k


def test_run_grad_fused_in_chunks(setups, nm_optimum):   # noqa: F811
    """S = 5 with cap = 3"""
    from rvspecfit_amd import vel_fit
    su = setups['grid']
    S = 5
    cols = ['vel', 'vsini'] + su['names']
    x0 = tj._x0(nm_optimum, su['names'], S, cols)
    H0 = vel_fit.get_hess_inv(cols)
    pobj, chain, dev_r, host = _fused_pair(su, S, x0, H0, cap=3)
    assert chain.cap == 3
    _bit_equal(dev_r, host)
    assert dev_r['calls'] >= 2 * min(dev_r['rounds'], 2)


def test_run_grad_fused_one_run_one_dimension(setups, nm_optimum):   # noqa: F811
    """S = 1, n = 1: the velocity alone"""
    su = setups['grid']
    fix = tuple(su['names']) + ('vsini', )
    x0 = tj._x0(nm_optimum, su['names'], 1, ['vel']) + 3.0
    pobj, chain, dev_r, host = _fused_pair(su, 1, x0, np.array([[1.0]]), fix=fix)
    assert pobj.n == 1
    d = _bit_equal(dev_r, host)
    assert d['nit'][0] >= 1


# ---- 7. process ----------------------------------------------------------------------------------
def test_process_with_fused_gradient(cases, setups):   # noqa: F811
    """8 fake stars: finite records, chisq no worse than the differenced polish from the
    same simplex optimum + 1e-6 |chisq| (test_process_with_second_minimizer_jac)"""
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.engine import SpecBatch
    su = setups['grid']
    S = 8
    batch = SpecBatch.from_specdata(tj._fake_stars(cases, S))
    pd0 = dict(teff=np.full(S, 5200.), logg=np.full(S, 2.3), feh=np.full(S, -0.8),
               alpha=np.full(S, 0.2), vsini=np.full(S, 5.0))
    out = {}
    for fused in (False, True):
        cfg = dict(su['cfg'], second_minimizer=True, second_minimizer_jac=fused,
                   fused_gradient=fused)
        out[fused] = vel_fit.process(batch, dict(pd0), options=dict(npoly=tj.NPOLY),
                                     config=cfg)
    a, b = out[True], out[False]
    assert a['bfgs']['jac'] is True and a['bfgs']['fused'] is True
    assert (a['bfgs']['njev'] >= 1).all()
    for k in ('vel', 'vel_err', 'chisq', 'vsini'):
        assert torch.isfinite(a[k]).all(), k
    for k in su['names']:
        assert torch.isfinite(a['param'][k]).all(), k
    ca, cb = a['chisq'].cpu().numpy(), b['chisq'].cpu().numpy()
    print('chisq fused', ca, 'fd', cb, 'fused - fd', ca - cb, 'nit', a['bfgs']['nit'],
          b['bfgs']['nit'], 'status', a['bfgs']['status'], b['bfgs']['status'])
    assert (ca <= cb + 1e-6 * np.abs(cb)).all(), ca - cb


# ---- 8. refusals -----------------------------------------------------------------------------------
def test_refusals(cases, setup, setups):   # noqa: F811
    """each option the kernel does not cover raises ValueError naming it and the key,
    from get_chisq_grad and from process"""
    import os
    from conftest import GOLD
    from rvspecfit_amd import engine, spec_fit, spec_inter, vel_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    import tri_grad_truth as ttruth
    su = setup
    _, vel, par, _ = truth.JOBS[0]
    sd = su['sds'][0]
    cfg = dict(su['cfg'], fused_gradient=True)
    pcfg = dict(cfg, second_minimizer=True, second_minimizer_jac=True)
    S = 2
    pbatch = SpecBatch.from_specdata(tj._fake_stars(cases, S))
    pd0 = dict(teff=np.full(S, 5200.), logg=np.full(S, 2.3), feh=np.full(S, -0.8),
               alpha=np.full(S, 0.2), vsini=np.full(S, 5.0))
    opt = dict(npoly=10)

    def both(match, g_kw=None, p_kw=None, g_sd=sd, p_batch=pbatch, g_cfg=cfg,
             p_cfg=pcfg, g_opt=opt, p_opt=opt, g_vel=vel, g_par=par, p_pd0=pd0):
        pat = r'(?s)fused_gradient.*%s|%s.*fused_gradient' % (match, match)
        with pytest.raises(ValueError, match=pat):
            spec_fit.get_chisq_grad(g_sd, g_vel, g_par, options=g_opt, config=g_cfg,
                                    **(g_kw or {}))
        with pytest.raises(ValueError, match=pat):
            vel_fit.process(p_batch, dict(p_pd0), options=p_opt, config=p_cfg,
                            **(p_kw or {}))
    # a resolution matrix
    rp = {x.name: spec_fit.construct_resol_mat(x.lam, width=0.5) for x in sd}
    prp = {a.name: spec_fit.construct_resol_mat(a.lam_host, 2500.) for a in pbatch.arms}
    both('resolution matrix', dict(resol_params=rp), dict(resolParams=prp))
    # fast_interp
    both('fast_interp', dict(fast_interp=True), None, p_opt=dict(npoly=10,
                                                                 fast_interp=True))
    # an npoly the kernel refuses
    both('npoly', g_opt=dict(npoly=11), p_opt=dict(npoly=11))
    # a grid set
    other = [spec_fit.SpecData(x.name, x.lam[:-3], x.spec[:-3], x.espec[:-3],
                               badmask=x.badmask[:-3]) for x in su['sds'][1]]
    gs = SpecBatch.from_specdata([sd, other])
    stars = tj._fake_stars(cases, 2)
    lam = stars[0][0].lam
    gset = SpecBatch([engine.ArmData(
        'gold_b', [lam, lam[:-7]], np.stack([stars[0][0].spec, stars[1][0].spec]),
        np.stack([stars[0][0].espec, stars[1][0].espec]), device='cuda',
        grid_id=np.arange(2, dtype=np.int32))])
    both('grid set', g_sd=gs, g_vel=[vel, vel], p_batch=gset)
    # a Delaunay library
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, ttruth.tri_lib_dict(n)),
                                    'golden-tri://')
    both('triangulation', g_cfg=dict(cfg, template_lib='golden-tri://'),
         p_cfg=dict(pcfg, template_lib='golden-tri://'))
    # an MLP library (the network of nn_case.npz)
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
    nncfg = dict(GOLD_CONFIG, template_lib='golden-nn://', fused_gradient=True,
                 nn_gradient=True)
    both('nn library', g_sd=nn_sds[0], p_batch=SpecBatch.from_specdata(nn_sds),
         g_cfg=nncfg, p_cfg=dict(nncfg, second_minimizer=True,
                                 second_minimizer_jac=True),
         g_opt=dict(npoly=5), p_opt=dict(npoly=5))
    # the key beside what needs tangent rows
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*second_minimizer_lm'):
        vel_fit.process(pbatch, dict(pd0), options=opt,
                        config=dict(cfg, second_minimizer=True, second_minimizer_lm=True))
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*Fisher'):
        spec_fit.get_chisq_fisher(sd, vel, par, options=opt, config=cfg)
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*epochs'):
        vel_fit.process_epochs(pbatch, np.array([0, 0]),
                               {k: v[:1] for k, v in pd0.items()}, np.zeros(2),
                               options=opt, config=cfg)
