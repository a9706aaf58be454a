"""The BFGS polish on the analytic gradient, on the device: rvs_proc_finish_grad and the
gradient chain against vel_fit.chisq_func_grad row by row; rvs_bfgs_run_grad against
the same machine on the host (bfgs.minimize_lockstep_native(jac=True)) around the same
chain driven from Python; what holds by construction; scipy itself; vel_fit.process
with config['second_minimizer_jac'].  Golden regular-grid arms (lib_gold_*) and golden
Delaunay arms (lib_tri_gold_*), npoly 10, 1 to 8 spectra.

Against scipy itself the trajectories may part at rounding, so f_end is compared:
  MI355X figure, first device run: |f_device - f_scipy| / |f_scipy| = 0, 0 and
  1.21e-16 on the three spectra (|d| = 2.27e-13 on f = -1881.7; nit 17 / 17, 0 / 0 and
  20 / 20, status 0 / 0, 2 / 2, 0 / 0: the runs did not part).
The bound is 10 x the largest figure of that run; the test prints every figure before
it asserts."""
import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG, gold_lib_dict, gold_specdata

import tri_grad_truth as ttruth

pytestmark = pytest.mark.gpu
NPOLY = 10
C_KMS = 299792.458
F_SCIPY_REL_MEASURED = 1.21e-16
F_SCIPY_REL_BOUND = 10 * F_SCIPY_REL_MEASURED


def _ulps(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid='ignore'):
        u = np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))
    return np.where(both_nan | (a == b), 0.0, u)


@pytest.fixture(scope='module')
def setups(cases):
    """per library kind: config, the spectra (lists of SpecData), their batch"""
    from rvspecfit_amd import _lib, spec_inter, spec_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    out = {}
    for kind, url, mk in (('grid', 'golden://', gold_lib_dict),
                          ('tri', 'golden-tri://', ttruth.tri_lib_dict)):
        for n in ('gold_b', 'gold_r'):
            spec_inter.register_library(TemplateLibrary(n, mk(n)), url)
        cfg = dict(GOLD_CONFIG, template_lib=url)
        rng = np.random.RandomState(21)
        sds = []
        for i in range(8):   # different noise per spectrum: different paths
            sds.append([spec_fit.SpecData(
                sd.name, sd.lam, sd.spec * (1 + 0.02 * rng.normal(size=len(sd.spec))),
                sd.espec, badmask=sd.badmask)
                for sd in gold_specdata(cases, ('c1', 'c3')[i % 2],
                                        spec_fit.SpecData)])
        batch = SpecBatch.from_specdata(sds)
        libs = spec_inter.get_libs(batch.names, cfg)
        names = list(spec_inter.getSpecParams('gold_b', cfg))
        out[kind] = dict(cfg=cfg, sds=sds, batch=batch, libs=libs, names=names)
    return out


# (stellar parameters of the rows: points tri_grad_truth.JOBS places inside a simplex of
# the golden triangulation, all of them inside the regular grid too)
PD0 = dict(teff=6000.0, logg=2.5, feh=-0.4, alpha=0.1, vsini=30.0)


def _objective(su, S, fix=(), priors=None, pd0=None, with_vsini=True):
    """optimizer.ProcessObjective of the first S spectra and the single-spectrum
    arguments of vel_fit.chisq_func_grad for each of them"""
    from rvspecfit_amd import optimizer, vel_fit
    batch = su['batch'].subset(torch.arange(S, device=su['batch'].device))
    names, cfg = su['names'], su['cfg']
    pd0 = dict(PD0 if pd0 is None else pd0)
    if not with_vsini:
        pd0.pop('vsini')
    fit = with_vsini and 'vsini' not in fix
    dev = batch.device
    pdt = {k: torch.full((S, ), float(v), dtype=torch.float64, device=dev)
           for k, v in pd0.items()}
    prb = None if priors is None else {
        k: (torch.full((S, ), float(m), dtype=torch.float64, device=dev),
            torch.full((S, ), float(sg), dtype=torch.float64, device=dev))
        for k, (m, sg) in priors.items()}
    safe = torch.stack([pdt[k] for k in names], dim=1).contiguous()
    pobj = optimizer.ProcessObjective(batch, su['libs'], names, pdt, list(fix), fit,
                                      cfg, dict(npoly=NPOLY), prb, safe)
    args = []
    for s in range(S):
        mapper = vel_fit.ParamMapper(names, dict(pd0), list(fix),
                                     vel_fit.VSiniMapper(cfg['max_vsini']),
                                     fitVsini=fit)
        args.append(dict(specdata=su['sds'][s], paramMapper=mapper,
                         options=dict(npoly=NPOLY), config=cfg, priors=priors,
                         min_vel=cfg['min_vel'], max_vel=cfg['max_vel']))
    return pobj, args


# ---- 1. rows against vel_fit.chisq_func_grad ------------------------------------------
def _row_cases(su):
    """(label, objective keywords, rows [(spectrum, x)], columns that carry a prior or
    penalty term per row)"""
    lnstep = su['libs']['gold_b'].lnstep
    near_int = (3 + 5e-4) * C_KMS * lnstep      # R = vsini / (c lnstep) near 3
    free = [
        ('inside', 0, [12.0, 30.0, 6000., 2.5, -0.4, 0.1], ()),
        ('x_vsini < 0', 1, [-20.0, -3.0, 6500., 3.6, -0.3, 0.12], (0, 2)),
        ('x_vsini > max', 2, [5.0, 520.0, 6200., 2.9, -0.9, 0.22], (0, 2)),
        ('R near an integer', 0, [12.0, near_int, 5000., 2.2, -1.0, 0.2], ()),
        ('vel out of range', 1, [1500.0, 30.0, 6000., 2.5, -0.4, 0.1], ()),
        ('non-finite parameter', 2, [12.0, 30.0, np.nan, 2.5, -0.4, 0.1], ()),
    ]
    fixed_prior = [   # alpha fixed (no column), Normal prior on teff (column 2)
        ('fixed alpha, prior on teff', 0, [12.0, 30.0, 6123., 2.5, -0.4], (0, 3)),
        ('the same, vsini below 0', 1, [-8.0, -1.0, 6000., 2.5, -0.4], (0, 2, 3)),
    ]
    vs_fixed = [      # vsini given and fixed: no column
        ('vsini fixed', 0, [12.0, 6000., 2.5, -0.4, 0.1], ()),
        ('vsini fixed, another spectrum', 2, [-15.0, 6200., 2.9, -0.9, 0.22], ()),
    ]
    return [(dict(), free), (dict(fix=('alpha', ), priors={'teff': (5800.0, 150.0)}),
                             fixed_prior), (dict(fix=('vsini', )), vs_fixed)]


@pytest.mark.parametrize('kind', ['grid', 'tri'])
def test_rows_against_chisq_func_grad(setups, kind):
    """rvs_proc_map + the gradient chain + rvs_proc_finish_grad against
    vel_fit.chisq_func_grad, row by row.  Both sides run the same kernels: the value
    and every component without a prior or penalty term are equal; a value or component
    with one is within 4 ulp (two additions in another order / 2 (p - mu) isig^2 against
    2 (p - mu) / sig^2: derived, nothing to measure)."""
    from rvspecfit_amd import optimizer, vel_fit
    su = setups[kind]
    for kw, rows in _row_cases(su):
        pobj, args = _objective(su, 3, **kw)
        chain = optimizer.GradChain(pobj)
        idx = np.array([r[1] for r in rows], dtype=np.int64)
        X = np.array([r[2] for r in rows], dtype=np.float64)
        F = chain.rows(idx, X)
        assert F.shape == (len(rows), X.shape[1] + 1)
        for j, (label, s, x, loose) in enumerate(rows):
            with np.errstate(all='ignore'):
                f, g = vel_fit.chisq_func_grad(np.array(x), args[s])
            want = np.concatenate([[f], g])
            u = _ulps(F[j], want)
            print(kind, label, 'F', F[j], 'want', want, 'ulps', u)
            if 'out of range' in label or 'non-finite' in label:
                assert f == 1e30 and not g.any()
            else:
                assert np.isfinite(F[j]).all() and g[0] != 0
            for c in range(len(want)):
                if c in loose:
                    assert u[c] <= 4, (label, c, F[j, c], want[c])
                else:
                    assert u[c] == 0, (label, c, F[j, c], want[c])


def test_finish_grad_refuses_bad_arguments(setups):
    from rvspecfit_amd import _lib
    import ctypes
    L = _lib.lib()
    t = torch.zeros(64, dtype=torch.float64, device='cuda')
    i = torch.zeros(64, dtype=torch.int32, device='cuda')
    p = _lib.ptr
    src = (ctypes.c_int32 * 4)(2, 3, 4, 5)

    def call(J=2, n=6, ndim=4, ntan=5, src=src, vcol=1, chi=t):
        return L.rvs_proc_finish_grad(J, n, ndim, ntan, None, 0, p(chi), p(t), p(t),
                                      p(t), p(t), p(i), p(i), p(i), src, vcol, None,
                                      None, 500.0, p(t), p(i), _lib.stream())
    assert call() == 0
    assert call(J=0) == -1 and call(n=9) == -1 and call(ndim=7) == -1
    assert call(ntan=4) == -1 and call(chi=None) == -1 and call(src=None) == -1
    assert call(vcol=6) == -1
    assert call(src=(ctypes.c_int32 * 4)(0, 3, 4, 5)) == -1    # the velocity's column
    assert call(src=(ctypes.c_int32 * 4)(1, 3, 4, 5)) == -1    # the vsini column
    assert call(src=(ctypes.c_int32 * 4)(2, 3, 4, -1)) == -1   # a column without source
    ntp = (ctypes.c_int32 * 2)(977, 781)
    assert L.rvs_grad_chain_work_size(0, 2, 5, ntp, 2) == 0
    assert L.rvs_grad_chain_work_size(4, 2, 7, ntp, 2) == 0
    assert L.rvs_grad_chain_work_size(4, 2, 5, None, 2) == 0
    assert L.rvs_grad_chain_work_size(4, 2, 5, ntp, 2) > 4 * 6 * (977 + 781) * 48
    assert L.rvs_bfgs_run_grad(None, None, None, 4, None, None) == -1
    torch.cuda.synchronize()


# ---- 2. rvs_bfgs_run_grad against the host machine around the same chain ----------------
def _start(su, S, n_free=True):
    """the simplex optimum of the first S spectra, as vel_fit.process reaches it"""
    from rvspecfit_amd import vel_fit
    batch = su['batch'].subset(torch.arange(S, device=su['batch'].device))
    pd0 = {k: np.full(S, v) for k, v in PD0.items()}
    r = vel_fit.process(batch, pd0, options=dict(npoly=NPOLY), config=dict(su['cfg']))
    return r


@pytest.fixture(scope='module')
def nm_optimum(setups):
    return _start(setups['grid'], 8)


def _x0(r, names, S, cols):
    v = dict(vel=r['nm_vel'][:S], vsini=r['vsini'][:S])
    v.update({k: r['param'][k][:S] for k in names})
    return torch.stack([v[c].double() for c in cols], dim=1).contiguous()


def _run_pair(su, S, x0, hess_inv0, cap=None, **kw):
    from rvspecfit_amd import bfgs, optimizer
    pobj, args = _objective(su, S, **kw)
    chain = optimizer.GradChain(pobj, cap=cap)
    dev_r = bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=hess_inv0, jac=True,
                                          chain=chain)
    host = bfgs.minimize_lockstep_native(chain.rows, x0.cpu().numpy(),
                                         hess_inv0=hess_inv0, jac=True)
    return pobj, chain, args, dev_r, host


def _compare(dev_r, host, S):
    d = {k: dev_r[k].cpu().numpy() for k in ('x', 'fun', 'nit', 'nfev', 'njev',
                                             'status')}
    print('device nit', d['nit'], 'nfev', d['nfev'], 'njev', d['njev'], 'status',
          d['status'], 'rounds', dev_r['rounds'], 'calls', dev_r['calls'])
    print('host   nit', host['nit'], 'nfev', host['nfev'], 'njev', host['njev'],
          'status', host['status'], 'rounds', host['rounds'])
    print('max |dfun|', np.abs(d['fun'] - host['fun']).max())
    # (the criteria of test_gpu_parity.py::test_process_bfgs_device_equals_host: the
    # machines differ in pow() of _cubicmin, a run whose zoom step falls on that last
    # bit may part ways)
    same = np.ones(S, dtype=bool)
    for k in ('nit', 'nfev', 'njev', 'status'):
        same &= d[k] == host[k]
    assert same.mean() > 0.9, same
    assert np.array_equal(d['x'][same], host['x'][same])
    assert np.array_equal(d['fun'][same], host['fun'][same])
    assert np.abs(d['fun'] - host['fun']).max() < 2e-3
    return d


def test_run_grad_equals_host_machine(setups, nm_optimum):
    """S = 8 golden spectra, n = 6 (vel, vsini, four parameters); two calls and a call
    on permuted spectra agree bit for bit; every run that ends with status 0 has
    max |g| <= gtol through vel_fit.chisq_func_grad; f_end <= f(x0)"""
    from rvspecfit_amd import bfgs, optimizer, vel_fit
    su = setups['grid']
    S = 8
    cols = ['vel', 'vsini'] + su['names']
    x0 = _x0(nm_optimum, su['names'], S, cols)
    H0 = vel_fit.get_hess_inv(cols)
    pobj, chain, args, dev_r, host = _run_pair(su, S, x0, H0)
    d = _compare(dev_r, host, S)
    assert d['njev'].max() > 3
    # by construction
    f0 = chain.rows(np.arange(S), x0.cpu().numpy())[:, 0]
    assert (d['fun'] <= f0).all(), (d['fun'], f0)
    for s in range(S):
        if d['status'][s] == 0:
            f, g = vel_fit.chisq_func_grad(d['x'][s], args[s])
            print('run', s, 'status 0: max |g|', np.abs(g).max())
            assert np.abs(g).max() <= 1e-5
    # twice the same bits
    again = bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=H0, jac=True, chain=chain)
    for k in ('x', 'fun', 'nit', 'nfev', 'njev', 'status'):
        assert np.array_equal(again[k].cpu().numpy(), d[k]), k
    # permuted spectra: the permuted runs
    perm = [4, 2, 6, 0, 7, 5, 1, 3]
    sub = dict(su, batch=su['batch'].subset(torch.tensor(perm, device='cuda')),
               sds=[su['sds'][i] for i in perm])
    pobj2, _ = _objective(sub, S)
    r2 = bfgs.minimize_lockstep_device(pobj2, x0[perm].contiguous(), hess_inv0=H0,
                                       jac=True)
    for k in ('x', 'fun', 'nit', 'nfev', 'njev', 'status'):
        assert np.array_equal(r2[k].cpu().numpy(), d[k][perm]), k


def test_run_grad_in_chunks(setups, nm_optimum):
    """S = 5 with cap = 3: two chunks per round, a run count that is no multiple of
    the advance kernel's block; the same results as with one chunk"""
    from rvspecfit_amd import bfgs, vel_fit
    su = setups['grid']
    S = 5
    cols = ['vel', 'vsini'] + su['names']
    x0 = _x0(nm_optimum, su['names'], S, cols)
    H0 = vel_fit.get_hess_inv(cols)
    pobj, chain, args, dev_r, host = _run_pair(su, S, x0, H0, cap=3)
    assert chain.cap == 3
    d = _compare(dev_r, host, S)
    assert dev_r['calls'] >= 2 * min(dev_r['rounds'], 2)
    pobj1, _ = _objective(su, S)
    one = bfgs.minimize_lockstep_device(pobj1, x0, hess_inv0=H0, jac=True)
    for k in ('x', 'fun', 'nit', 'nfev', 'njev', 'status'):
        assert np.array_equal(one[k].cpu().numpy(), d[k]), k


def test_run_grad_one_run_one_dimension(setups, nm_optimum):
    """S = 1, n = 1: every stellar parameter and vsini fixed, the velocity alone"""
    su = setups['grid']
    fix = tuple(su['names']) + ('vsini', )
    x0 = _x0(nm_optimum, su['names'], 1, ['vel']) + 3.0
    H0 = np.array([[1.0]])     # get_hess_inv's entry of the velocity
    pobj, chain, args, dev_r, host = _run_pair(su, 1, x0, H0, fix=fix)
    assert pobj.n == 1
    d = _compare(dev_r, host, 1)
    assert d['nit'][0] >= 1


def test_run_grad_delaunay(setups):
    """the Delaunay arms (rvs_template_tri_buckets_grad in the chain): S = 4"""
    from rvspecfit_amd import vel_fit
    su = setups['tri']
    S = 4
    cols = ['vel', 'vsini'] + su['names']
    x0 = _x0(_start(su, S), su['names'], S, cols)
    H0 = vel_fit.get_hess_inv(cols)
    pobj, chain, args, dev_r, host = _run_pair(su, S, x0, H0)
    _compare(dev_r, host, S)


# ---- 3. scipy itself ----------------------------------------------------------------
def test_f_end_against_scipy(setups, nm_optimum):
    """three spectra through scipy.optimize.minimize(vel_fit.chisq_func_grad, x0,
    jac=True, method='BFGS', hess_inv0=...): f_end (see the file header)"""
    import warnings
    import scipy.optimize as so
    from rvspecfit_amd import bfgs, vel_fit
    su = setups['grid']
    S = 3
    cols = ['vel', 'vsini'] + su['names']
    x0 = _x0(nm_optimum, su['names'], S, cols)
    H0 = vel_fit.get_hess_inv(cols)
    pobj, args = _objective(su, S)
    r = bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=H0, jac=True)
    fun = r['fun'].cpu().numpy()
    worst = 0.0
    for s in range(S):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            q = so.minimize(vel_fit.chisq_func_grad, x0[s].cpu().numpy(),
                            args=(args[s], ), jac=True, method='BFGS',
                            options=dict(hess_inv0=H0))
        rel = abs(fun[s] - q.fun) / abs(q.fun)
        print('spectrum %d f_device %.12g f_scipy %.12g |d| %.3g rel %.3g nit %d / %d '
              'status %d / %d' % (s, fun[s], q.fun, abs(fun[s] - q.fun), rel,
                                  int(r['nit'][s]), q.nit, int(r['status'][s]),
                                  q.status))
        worst = max(worst, rel)
    print('largest |f_device - f_scipy| / |f_scipy| %.3g (bound %.3g)'
          % (worst, F_SCIPY_REL_BOUND))
    assert worst <= F_SCIPY_REL_BOUND


# ---- 4. vel_fit.process -------------------------------------------------------------
def _fake_stars(cases, S=8):
    from rvspecfit_amd import spec_fit, synth
    lam = cases['c0/gold_b/lam']
    sds = []
    for seed in range(S):
        rng = np.random.RandomState(100 + seed)
        spec, espec = synth.fake_observation(lam, 5000. + 60 * seed, 2., -1., 0.2,
                                             rng.normal(0, 100), 80., rng,
                                             wresol=4700. / 2000 / 2.35)
        sds.append([spec_fit.SpecData('gold_b', lam, spec, espec)])
    return sds


@pytest.mark.parametrize('kind', ['grid', 'tri'])
def test_process_with_second_minimizer_jac(cases, setups, kind):
    """8 fake stars: finite records, bfgs info says jac, chisq no worse than the
    differenced polish from the same simplex optimum (+ 1e-6 |chisq| for the later
    velocity refinement)"""
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.engine import SpecBatch
    su = setups[kind]
    S = 8
    batch = SpecBatch.from_specdata(_fake_stars(cases, S))
    pd0 = dict(teff=np.full(S, 5200.), logg=np.full(S, 2.3), feh=np.full(S, -0.8),
               alpha=np.full(S, 0.2), vsini=np.full(S, 5.0))
    out = {}
    for jac in (False, True):
        cfg = dict(su['cfg'], second_minimizer=True, second_minimizer_jac=jac)
        out[jac] = vel_fit.process(batch, dict(pd0), options=dict(npoly=NPOLY),
                                   config=cfg)
    a, b = out[True], out[False]
    assert a['bfgs']['jac'] is True and 'jac' not in b['bfgs']
    assert a['bfgs']['njev'].shape == (S, ) and (a['bfgs']['njev'] >= 1).all()
    for k in ('vel', 'vel_err', 'chisq', 'vsini'):
        assert torch.isfinite(a[k]).all(), k
    for k in su['names']:
        assert torch.isfinite(a['param'][k]).all(), k
    ca, cb = a['chisq'].cpu().numpy(), b['chisq'].cpu().numpy()
    print(kind, 'chisq jac', ca, 'fd', cb, 'jac - fd', ca - cb, 'nit', a['bfgs']['nit'],
          b['bfgs']['nit'], 'nfev', a['bfgs']['nfev'], b['bfgs']['nfev'], 'status',
          a['bfgs']['status'], b['bfgs']['status'])
    assert (ca <= cb + 1e-6 * np.abs(cb)).all(), ca - cb


def test_process_jac_refuses_what_the_gradient_does_not_cover(cases, setups,
                                                               monkeypatch):
    """every option outside the gradient's scope raises ValueError naming it, from
    process itself and before anything is built: npoly > 16, a resolution matrix,
    fast_interp, an MLP library, a grid set, vsini beside six parameters; and a batch
    the chain's chunks do not hold"""
    import itertools
    import os
    from conftest import GOLD
    from rvspecfit_amd import engine, optimizer, spec_fit, spec_inter, vel_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    su = setups['grid']
    stars = _fake_stars(cases, 2)
    batch = SpecBatch.from_specdata(stars)
    pd0 = dict(teff=np.full(2, 5200.), logg=np.full(2, 2.3), feh=np.full(2, -0.8),
               alpha=np.full(2, 0.2), vsini=np.full(2, 5.0))
    jac = dict(second_minimizer=True, second_minimizer_jac=True)
    cfg = dict(su['cfg'], **jac)

    def never(*a, **k):
        raise AssertionError('something was built before the scope was checked')
    monkeypatch.setattr(optimizer, 'ProcessObjective', never)
    monkeypatch.setattr(spec_fit, 'chisq_grid_jobs', never)
    with pytest.raises(ValueError, match='npoly'):
        vel_fit.process(batch, dict(pd0), options=dict(npoly=17), config=cfg)
    rp = {a.name: spec_fit.construct_resol_mat(a.lam_host, 2500.) for a in batch.arms}
    with pytest.raises(ValueError, match='resolution matrix'):
        vel_fit.process(batch, dict(pd0), options=dict(npoly=NPOLY), config=cfg,
                        resolParams=rp)
    with pytest.raises(ValueError, match='fast_interp'):
        vel_fit.process(batch, dict(pd0), options=dict(npoly=NPOLY, fast_interp=True),
                        config=cfg)
    # a grid set: the two spectra on wavelength grids of their own
    lam = stars[0][0].lam
    grids = [lam, lam[:-7]]
    sp = np.stack([stars[0][0].spec, stars[1][0].spec])
    es = np.stack([stars[0][0].espec, stars[1][0].espec])
    gset = SpecBatch([engine.ArmData('gold_b', grids, sp, es, device='cuda',
                                     grid_id=np.arange(2, dtype=np.int32))])
    with pytest.raises(ValueError, match='grid set'):
        vel_fit.process(gset, dict(pd0), options=dict(npoly=NPOLY), config=cfg)
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
    nnb = SpecBatch.from_specdata([[spec_fit.SpecData(
        'aat_580v', wave, rng.normal(1, 0.1, 1000), np.full(1000, 0.1))]
        for _ in range(2)])
    with pytest.raises(ValueError, match='nn library'):
        vel_fit.process(nnb, dict(pd0), options=dict(npoly=5),
                        config=dict(GOLD_CONFIG, template_lib='golden-nn://', **jac))
    # six stellar parameters and a fitted vsini: seven tangents
    nd = 6
    pts = np.array(list(itertools.product([0., 1.], repeat=nd)))
    tl = np.exp(np.linspace(np.log(lam[0] - 30), np.log(lam[-1] + 30), 1500))
    six = dict(lam=tl, log_step=np.array(True), log_ids=np.array([], dtype=int),
               parnames=np.array(['p%d' % i for i in range(nd)]),
               dats=np.zeros((2**nd, len(tl)), dtype=np.float32),
               idgrid=np.arange(2**nd).reshape((2, ) * nd), vec=pts.T.copy())
    for i in range(nd):
        six['uvec%d' % i] = np.array([0., 1.])
    spec_inter.register_library(TemplateLibrary('gold_b', six), 'golden-six://')
    pd6 = {'p%d' % i: np.full(2, 0.5) for i in range(nd)}
    pd6['vsini'] = np.full(2, 5.0)
    with pytest.raises(ValueError, match='vsini'):
        vel_fit.process(batch, pd6, options=dict(npoly=NPOLY),
                        config=dict(GOLD_CONFIG, template_lib='golden-six://', **jac))
    # more spectra than 24 chunks of the budget's rows
    monkeypatch.setattr(optimizer, "GRAD_CHAIN_BUDGET", 1 << 19)   # one row per chunk
    big = SpecBatch.from_specdata(_fake_stars(cases, 2) * 13)
    pdb = {k: np.full(26, v[0]) for k, v in pd0.items()}
    with pytest.raises(ValueError, match='GRAD_CHAIN_BUDGET'):
        vel_fit.process(big, pdb, options=dict(npoly=NPOLY), config=cfg)


def test_process_jac_host_machine_equals_device(cases, setups, monkeypatch):
    """RVS_BFGS_ON_DEVICE=0 (vel_fit.BFGS_ON_DEVICE False): process runs
    minimize_lockstep_native(jac=True) around GradChain.rows -- the same machine on
    the same kernels as the device loop, held to it under the criteria of
    test_gpu_parity.py::test_process_bfgs_device_equals_host"""
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.engine import SpecBatch
    su = setups['grid']
    S = 8
    batch = SpecBatch.from_specdata(_fake_stars(cases, S))
    pd0 = dict(teff=np.full(S, 5200.), logg=np.full(S, 2.3), feh=np.full(S, -0.8),
               alpha=np.full(S, 0.2), vsini=np.full(S, 5.0))
    cfg = dict(su['cfg'], second_minimizer=True, second_minimizer_jac=True)
    out = {}
    for name, flag in (('device', True), ('host', False)):
        monkeypatch.setattr(vel_fit, 'BFGS_ON_DEVICE', flag)
        out[name] = vel_fit.process(batch, dict(pd0), options=dict(npoly=NPOLY),
                                    config=cfg)
    a, b = out['device'], out['host']
    assert a['bfgs']['device'] and not b['bfgs']['device']
    assert a['bfgs']['jac'] and b['bfgs']['jac']
    assert torch.equal(a['nm_nit'], b['nm_nit'])
    print('device', a['bfgs'], 'host', b['bfgs'], 'evals', a['objective_evals'],
          b['objective_evals'])
    same = np.ones(S, dtype=bool)
    for k in ('nit', 'nfev', 'njev', 'status'):
        same &= np.asarray(a['bfgs'][k]) == np.asarray(b['bfgs'][k])
    assert same.mean() > 0.9, same
    sm = torch.as_tensor(same).to(a['vel'].device)
    for k in ('vel', 'chisq'):
        assert torch.equal(a[k][sm], b[k][sm]), k
    for k in su['names']:
        assert torch.equal(a['param'][k][sm], b['param'][k][sm]), k
    assert (a['chisq'] - b['chisq']).abs().max().item() < 2e-3
    # the device counts the rows it launched, the rows behind the counters included
    assert a['objective_evals'] >= b['objective_evals'] > 0


def test_run_grad_delaunay_scan_form(setups, monkeypatch):
    """library.TRI_BUCKETS False: the chain takes rvs_template_tri_grad (the exhaustive
    find_simplex) as TemplateLibrary._tri_call does; the same simplices, so the same
    bits as through the bucket grid"""
    from rvspecfit_amd import bfgs, library, vel_fit
    su = setups['tri']
    S = 3
    cols = ['vel', 'vsini'] + su['names']
    H0 = vel_fit.get_hess_inv(cols)
    x0 = torch.tensor([[12.0, 30.0, 6000., 2.5, -0.4, 0.1],
                       [-20.0, 20.0, 6500., 3.6, -0.3, 0.12],
                       [5.0, 40.0, 6200., 2.9, -0.9, 0.22]], dtype=torch.float64,
                      device='cuda')
    out = {}
    for flag in (True, False):
        monkeypatch.setattr(library, 'TRI_BUCKETS', flag)
        pobj, _ = _objective(su, S)
        out[flag] = bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=H0, jac=True,
                                                  maxiter=12)
    print('buckets', out[True]['nit'], out[True]['status'], 'scan', out[False]['nit'],
          out[False]['status'])
    assert int(out[True]['njev'].min()) >= 1
    for k in ('x', 'fun', 'nit', 'nfev', 'njev', 'status'):
        assert torch.equal(out[True][k], out[False][k]), k
