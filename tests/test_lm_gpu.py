"""The Levenberg-Marquardt polish on the device: rvs_proc_finish_fisher against the numpy
statement of its mapping (tests/lm_truth.py); the rows of the Fisher form of the gradient
chain against vel_fit.chisq_func_fisher and the CPU truth of the Fisher matrix;
rvs_lm_run against the same machine on the host around the same chain; vel_fit.process
with config['second_minimizer_lm'].  Golden regular-grid arms (lib_gold_*) and golden
Delaunay arms (lib_tri_gold_*), npoly 10, 1 to 8 spectra -- the set-ups, row kinds and
fake stars of tests/test_bfgs_jac_gpu.py.

Value and gradient of a row.  The Fisher form's (f, g) are held bit for bit against the
gradient chain's (GradChain().rows: the same kernels' first two passes and the same
statements of the finish kernel), and vel_fit.chisq_func_fisher's against
vel_fit.chisq_func_grad's.  Against the host function a device row carries what
test_bfgs_jac_gpu.py::test_rows_against_chisq_func_grad derives: 0 ulp, and 4 ulp on the
value and the components with a prior or penalty term (two additions in another order,
2 (p - mu) isig^2 against 2 (p - mu) / sig^2).

rvs_lm_run against the host machine: every run the same path and the same bits, on every
shape (see test_lm_run_equals_host_machine).

MI355X figures of the first device run (every test prints its own before it asserts):
rvs_proc_finish_fisher's H 0 ulp from the numpy mapping on all three configurations; a
row's H 0 - 1 ulp from chisq_func_fisher, its (vel, parameters) block at most 1.12e-14 of
sqrt(G_ii G_ll) from 2 F_truth (bound 5.84e-12); rvs_lm_run and the host machine: max |dx|
= max |dfun| = 0 on the four shapes (nit 3 - 34, nfev 4 - 81 per run); process on the fake
stars: chisq_lm - chisq_differenced in [-4.6e-5, -3.2e-10] (regular grid, 2 - 5 rows per
spectrum against 70 - 713) and [-0.61, +1.3e-4] (Delaunay; the margin is 2.9e-3)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG, gold_lib_dict, gold_specdata
from oracle import rvs_oracle as orc

import chisq_fisher_truth as ftruth
import lm_truth
import tri_grad_truth as ttruth
from test_bfgs_jac_gpu import (NPOLY, _fake_stars, _objective, _row_cases,  # noqa: F401
                               _start, _ulps, _x0, nm_optimum, setups)
from test_chisq_fisher_gpu import BOUND

pytestmark = pytest.mark.gpu


# ---- 1. rvs_proc_finish_fisher against the numpy mapping ------------------------------
FINISH = {
    # name: (n, src [ndim = 4], vsini_col, priors)
    'n6': (6, [2, 3, 4, 5], 1, True),
    'n3_two_fixed_one_prior': (3, [-1, 1, -1, 2], -1, True),
    'n1': (1, [-1, -1, -1, -1], -1, False),
}


def _finish_inputs(name):
    n, src, vcol, prior = FINISH[name]
    J, ndim = 37, len(src)
    fisher, X, isig = lm_truth.seeded_rows(31, J, n, src, vcol, prior=prior)
    K = fisher.shape[1]
    rng = np.random.RandomState(32)
    d = dict(chi=rng.normal(size=J) * 1e3, grad=rng.normal(size=(J, K)) * 10,
             fisher=fisher, X=X, params=rng.normal(size=(J, ndim)),
             extra=np.abs(rng.normal(size=J)), bad=np.zeros(J, dtype=np.int32),
             job_spec=rng.permutation(J).astype(np.int32),
             job_status=np.zeros(J, dtype=np.int32))
    d['bad'][[5, 36]] = 1
    if prior:
        # (per spectrum r = job_spec[j]: isig of row j is prior_isig[job_spec[j]])
        d['prior_isig'] = isig
        d['prior_mean'] = rng.normal(size=(J, ndim))
        d['isig_rows'] = isig[d['job_spec']]
    else:
        d['prior_isig'] = d['prior_mean'] = d['isig_rows'] = None
    return d


@pytest.mark.parametrize('name', list(FINISH))
def test_finish_fisher_against_numpy_mapping(name):
    from rvspecfit_amd import _lib, lm
    _lib.require_gpu()
    L = _lib.lib()
    n, src, vcol, prior = FINISH[name]
    d = _finish_inputs(name)
    J, ndim = 37, len(src)
    ntan = ndim + (1 if vcol >= 0 else 0)
    t = {k: (None if v is None else torch.as_tensor(v).cuda().contiguous())
         for k, v in d.items()}
    p = _lib.ptr
    csrc = (ctypes.c_int32 * ndim)(*src)
    status = torch.zeros(J, dtype=torch.int32, device='cuda')
    Fg = torch.full((J, n + 1), np.nan, dtype=torch.float64, device='cuda')
    Ff = torch.full((J, lm.npack(n)), np.nan, dtype=torch.float64, device='cuda')
    head = (J, n, ndim, ntan, None, 0, p(t['chi']), p(t['grad']))
    tail = (p(t['X']), p(t['params']), p(t['extra']), p(t['bad']), p(t['job_spec']),
            p(t['job_status']), csrc, vcol, p(t['prior_mean']), p(t['prior_isig']),
            500.0)
    assert L.rvs_proc_finish_grad(*head, *tail, p(Fg), p(status), _lib.stream()) == 0
    assert L.rvs_proc_finish_fisher(*head, p(t['fisher']), *tail, p(Ff), p(status),
                                    _lib.stream()) == 0
    torch.cuda.synchronize()
    Fg, Ff = Fg.cpu().numpy(), Ff.cpu().numpy()
    # f and the gradient: the bits of rvs_proc_finish_grad
    assert np.array_equal(Ff[:, :n + 1], Fg)
    f, g, H = lm.unpack_rows(Ff, n)
    want = lm_truth.hess_from_fisher(d['fisher'], d['X'], src, vcol, d['isig_rows'],
                                     500.0)
    bad = d['bad'] != 0
    assert (f[bad] == 1e30).all() and not g[bad].any() and not H[bad].any()
    u = _ulps(H[~bad], want[~bad])
    print(name, 'largest H error', u.max(), 'ulp')
    assert u.max() <= 4
    if vcol >= 0:
        x = d['X'][:, vcol]
        for kind in (x < 0, x == 0, (0 < x) & (x < 500), x > 500):
            assert (kind & ~bad).any()
    # bad arguments: refused as by rvs_proc_finish_grad

    def call(J=J, n=n, ndim=ndim, ntan=ntan, src=csrc, vcol=vcol, chi=t['chi'],
             fisher=t['fisher']):
        return L.rvs_proc_finish_fisher(
            J, n, ndim, ntan, None, 0, p(chi), p(t['grad']), p(fisher), *tail[:6], src,
            vcol, *tail[8:], p(Ff_dev), p(status), _lib.stream())
    Ff_dev = torch.empty((J, lm.npack(n)), dtype=torch.float64, device='cuda')
    assert call() == 0
    assert call(J=0) == -1 and call(n=9) == -1 and call(ndim=7) == -1
    assert call(ntan=ntan + 1) == -1 and call(chi=None) == -1 and call(src=None) == -1
    assert call(fisher=None) == -1 and call(vcol=n) == -1
    assert call(src=(ctypes.c_int32 * 4)(0, 3, 4, 5)) == -1    # the velocity's column
    torch.cuda.synchronize()


# ---- 2. rows against vel_fit.chisq_func_fisher and the truth ----------------------------
def _oracle_spectra(cases):
    """the spectra of test_bfgs_jac_gpu.setups (the same seeded noise) as the oracle's
    SpecData, for tests/chisq_fisher_truth.py"""
    rng = np.random.RandomState(21)
    out = []
    for i in range(8):
        out.append([orc.SpecData(
            sd.name, sd.lam, sd.spec * (1 + 0.02 * rng.normal(size=len(sd.spec))),
            sd.espec, badmask=sd.badmask)
            for sd in gold_specdata(cases, ('c1', 'c3')[i % 2], orc.SpecData)])
    return out


@pytest.mark.parametrize('kind', ['grid', 'tri'])
def test_rows_against_chisq_func_fisher(cases, setups, kind):
    """GradChain(fisher=True).rows on the ten row kinds: (f, g) the bits of the gradient
    chain's rows and within the derived ulps of vel_fit.chisq_func_grad (file header); H
    exactly symmetric by its packed form, the bits of vel_fit.chisq_func_fisher's up to
    the 4 ulp of a prior term, and its (vel, stellar parameters) block within the
    project's bound for this chain of sums of 2 F_truth + the analytic prior term --
    tests/chisq_fisher_truth.py holds vsini fixed, so the vsini row and column have no
    truth there and are held by the mapping's properties (zero where the mapper clamps,
    2 on the diagonal beyond the clamp) and by chisq_func_fisher."""
    from rvspecfit_amd import lm, optimizer, vel_fit
    su = setups[kind]
    osds = _oracle_spectra(cases)
    if kind == 'grid':
        olibs = {n: orc.Library(gold_lib_dict(n)) for n in ('gold_b', 'gold_r')}
        tfn = ftruth.regular_template
    else:
        olibs, tfn = ttruth.oracle_libs(), ftruth.tri_template
    max_vsini = su['cfg']['max_vsini']
    worst = 0.0
    for kw, rows in _row_cases(su):
        pobj, args = _objective(su, 3, **kw)
        idx = np.array([r[1] for r in rows], dtype=np.int64)
        X = np.array([r[2] for r in rows], dtype=np.float64)
        n = X.shape[1]
        Fg = optimizer.GradChain(pobj).rows(idx, X)
        F = optimizer.GradChain(pobj, fisher=True).rows(idx, X)
        assert F.shape == (len(rows), lm.npack(n))
        assert np.array_equal(F[:, :n + 1], Fg, equal_nan=True)
        fr, gr, Hr = lm.unpack_rows(F, n)
        for j, (label, s, x, loose) in enumerate(rows):
            mapper = args[s]['paramMapper']
            fitted = mapper.get_fitted_params()
            with np.errstate(all='ignore'):
                f, g, H = vel_fit.chisq_func_fisher(np.array(x), args[s])
                f2, g2 = vel_fit.chisq_func_grad(np.array(x), args[s])
            assert f == f2 and np.array_equal(g, g2)
            assert H.shape == (n, n) and np.array_equal(H, H.T)
            u = _ulps(np.concatenate([[fr[j]], gr[j]]), np.concatenate([[f], g]))
            for c in range(n + 1):
                assert u[c] <= (4 if c in loose else 0), (label, c, u[c])
            uh = _ulps(Hr[j], H)
            print(kind, label, 'H ulps against chisq_func_fisher', uh.max())
            assert uh.max() <= 4
            if 'out of range' in label or 'non-finite' in label:
                assert f == 1e30 and not g.any() and not H.any()
                assert fr[j] == 1e30 and not gr[j].any() and not Hr[j].any()
                continue
            assert np.isfinite(F[j]).all()
            if 'vsini' in fitted:
                v = fitted.index('vsini')
                if not 0 < x[v] < max_vsini:
                    assert Hr[j, v, v] == 2.0
                    assert not np.delete(Hr[j, v], v).any()
                else:
                    assert Hr[j, v, v] > 0
            # the (vel, stellar parameters) block against the truth
            pd = mapper.forward(np.array(x))
            Ft, G, cond = ftruth.fisher(osds[s], olibs, pd['vel'], tuple(pd['params']),
                                        pd['vsini'], npoly=NPOLY, template_fn=tfn)
            names = list(mapper.specParams)
            cols = [a for a, k in enumerate(fitted) if k != 'vsini']
            tan = [0 if fitted[a] == 'vel' else 1 + names.index(fitted[a])
                   for a in cols]
            want = 2.0 * Ft[np.ix_(tan, tan)]
            pri = args[s]['priors'] or {}
            for q, a in enumerate(cols):
                if fitted[a] in pri:
                    want[q, q] += 2.0 / pri[fitted[a]][1]**2
            gs = np.sqrt(np.diag(G))[tan]
            rel = np.abs(Hr[j][np.ix_(cols, cols)] - want) / (2.0 * gs[:, None] * gs)
            print(kind, label, 'cond(A) %.3g largest error %.3g of sqrt(G_ii G_ll) '
                  '(bound %.3g)' % (cond, rel.max(), BOUND))
            worst = max(worst, float(rel.max()))
    assert worst <= BOUND


# ---- 3. rvs_lm_run against the host machine around the same chain -----------------------
KEYS = ('x', 'fun', 'grad', 'hess', 'mu', 'nit', 'nfev', 'status')


def _lm_pair(su, S, x0, cap=None, **kw):
    from rvspecfit_amd import lm, optimizer
    pobj, args = _objective(su, S, **kw)
    chain = optimizer.GradChain(pobj, cap=cap, fisher=True)
    dev_r = lm.minimize_lockstep_device(pobj, x0, chain=chain)
    host = lm.minimize_lockstep_native(chain.rows, x0.cpu().numpy())
    d = {k: dev_r[k].cpu().numpy() for k in KEYS}
    print('device nit', d['nit'], 'nfev', d['nfev'], 'status', d['status'], 'rounds',
          dev_r['rounds'], 'calls', dev_r['calls'])
    print('host   nit', host['nit'], 'nfev', host['nfev'], 'status', host['status'],
          'rounds', host['rounds'])
    print('max |dx|', np.abs(d['x'] - host['x']).max(), 'max |dfun|',
          np.abs(d['fun'] - host['fun']).max())
    # every run the same path and the same bits
    for k in KEYS:
        assert np.array_equal(d[k], host[k]), k
    # (the device counts the rounds it launched: it looks at the counters every
    # sync_every = 4 rounds in the tail, so up to 3 rounds behind the last run's end)
    assert host['rounds'] <= dev_r['rounds'] < host['rounds'] + 4
    f0 = chain.rows(np.arange(S), x0.cpu().numpy())[:, 0]
    assert (d['fun'] <= f0).all(), (d['fun'], f0)
    assert np.array_equal(d['hess'], d['hess'].transpose(0, 2, 1))
    return pobj, chain, args, dev_r, d


def test_lm_run_equals_host_machine(setups, nm_optimum):
    """S = 8 golden spectra, n = 6; two calls in a row agree bit for bit; a run that ends
    with status 0 on the gradient has max |g| <= gtol"""
    from rvspecfit_amd import lm
    su = setups['grid']
    S = 8
    cols = ['vel', 'vsini'] + su['names']
    x0 = _x0(nm_optimum, su['names'], S, cols)
    pobj, chain, args, dev_r, d = _lm_pair(su, S, x0)
    assert d['nfev'].max() > 2 and (d['nfev'] >= d['nit'] + 1).all()
    assert dev_r['rows_launched'] >= d['nfev'].sum()
    again = lm.minimize_lockstep_device(pobj, x0, chain=chain)
    for k in KEYS:
        assert np.array_equal(again[k].cpu().numpy(), d[k]), k


def test_lm_run_in_chunks(setups, nm_optimum):
    """S = 5 with cap = 3: two chunks per round; the results of one chunk"""
    from rvspecfit_amd import lm
    su = setups['grid']
    S = 5
    cols = ['vel', 'vsini'] + su['names']
    x0 = _x0(nm_optimum, su['names'], S, cols)
    pobj, chain, args, dev_r, d = _lm_pair(su, S, x0, cap=3)
    assert chain.cap == 3
    assert dev_r['calls'] >= 2 * min(dev_r['rounds'], 2)
    pobj1, _ = _objective(su, S)
    one = lm.minimize_lockstep_device(pobj1, x0)
    for k in KEYS:
        assert np.array_equal(one[k].cpu().numpy(), d[k]), k


def test_lm_run_one_run_one_dimension(setups, nm_optimum):
    """S = 1, n = 1: every stellar parameter and vsini fixed, the velocity alone"""
    su = setups['grid']
    fix = tuple(su['names']) + ('vsini', )
    x0 = _x0(nm_optimum, su['names'], 1, ['vel']) + 3.0
    pobj, chain, args, dev_r, d = _lm_pair(su, 1, x0, fix=fix)
    assert pobj.n == 1 and d['nit'][0] >= 1


def test_lm_run_delaunay(setups):
    """the Delaunay arms: S = 4"""
    su = setups['tri']
    S = 4
    cols = ['vel', 'vsini'] + su['names']
    x0 = _x0(_start(su, S), su['names'], S, cols)
    _lm_pair(su, S, x0)


# ---- 4. vel_fit.process ------------------------------------------------------------------
PD0_STARS = dict(teff=5200., logg=2.3, feh=-0.8, alpha=0.2, vsini=5.0)


@pytest.mark.parametrize('kind', ['grid', 'tri'])
def test_process_with_second_minimizer_lm(cases, setups, kind):
    """8 fake stars: finite records, ret['lm'] with device=True and no 'bfgs' key, chisq
    no worse than the differenced polish from the same simplex optimum (+ 1e-6 |chisq|,
    the margin of the jac polish's test), every run's fun at or below the objective at
    its start (the simplex optimum of a call without a second minimiser; the value of
    vel_fit.chisq_func_grad there, which a device row follows within 4 ulp)"""
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.engine import SpecBatch
    su = setups[kind]
    S = 8
    stars = _fake_stars(cases, S)
    batch = SpecBatch.from_specdata(stars)
    pd0 = {k: np.full(S, v) for k, v in PD0_STARS.items()}
    out = {}
    for tag, extra in (('nm', {}), ('fd', dict(second_minimizer=True)),
                       ('lm', dict(second_minimizer=True, second_minimizer_lm=True))):
        out[tag] = vel_fit.process(batch, dict(pd0), options=dict(npoly=NPOLY),
                                   config=dict(su['cfg'], **extra))
    a, b, nm = out['lm'], out['fd'], out['nm']
    assert 'bfgs' not in a and 'lm' not in b and 'lm' not in nm
    info = a['lm']
    assert info['device'] is True and a['second_minimizer_run']
    for k in ('nit', 'nfev', 'status', 'mu', 'fun'):
        assert np.asarray(info[k]).shape == (S, ), k
    assert (info['nfev'] >= 1).all() and info['rounds'] >= 1
    for k in ('vel', 'vel_err', 'chisq', 'vsini'):
        assert torch.isfinite(a[k]).all(), k
    for k in su['names']:
        assert torch.isfinite(a['param'][k]).all(), k
    ca, cb = a['chisq'].cpu().numpy(), b['chisq'].cpu().numpy()
    print(kind, 'chisq lm', ca, 'fd', cb, 'lm - fd', ca - cb, 'nit', info['nit'],
          b['bfgs']['nit'], 'nfev', info['nfev'], b['bfgs']['nfev'], 'status',
          info['status'], b['bfgs']['status'], 'rounds', info['rounds'],
          b['bfgs']['rounds'])
    assert (ca <= cb + 1e-6 * np.abs(cb)).all(), ca - cb
    # every run ends at or below its start
    for s in range(S):
        mapper = vel_fit.ParamMapper(su['names'], dict(PD0_STARS), [],
                                     vel_fit.VSiniMapper(su['cfg']['max_vsini']),
                                     fitVsini=True)
        args = dict(specdata=stars[s], paramMapper=mapper, options=dict(npoly=NPOLY),
                    config=su['cfg'], priors=None, min_vel=su['cfg']['min_vel'],
                    max_vel=su['cfg']['max_vel'])
        x0 = [float(nm['nm_vel'][s]), float(nm['vsini'][s])] + \
            [float(nm['param'][k][s]) for k in su['names']]
        f0, _ = vel_fit.chisq_func_grad(np.array(x0), args)
        assert info['fun'][s] <= f0 + 4 * np.spacing(abs(f0)), (s, info['fun'][s], f0)


def test_process_lm_host_machine_equals_device(cases, setups, monkeypatch):
    """RVS_BFGS_ON_DEVICE=0 (vel_fit.BFGS_ON_DEVICE False): process runs
    lm.minimize_lockstep_native around GradChain(fisher=True).rows -- the same machine
    on the same kernels; the same records come out"""
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.engine import SpecBatch
    su = setups['grid']
    S = 8
    batch = SpecBatch.from_specdata(_fake_stars(cases, S))
    pd0 = {k: np.full(S, v) for k, v in PD0_STARS.items()}
    cfg = dict(su['cfg'], second_minimizer=True, second_minimizer_lm=True)
    out = {}
    for name, flag in (('device', True), ('host', False)):
        monkeypatch.setattr(vel_fit, 'BFGS_ON_DEVICE', flag)
        out[name] = vel_fit.process(batch, dict(pd0), options=dict(npoly=NPOLY),
                                    config=cfg)
    a, b = out['device'], out['host']
    assert a['lm']['device'] and not b['lm']['device']
    print('device', a['lm'], 'host', b['lm'])
    for k in ('nit', 'nfev', 'status', 'mu', 'fun'):
        assert np.array_equal(np.asarray(a['lm'][k]), np.asarray(b['lm'][k])), k
    assert b['lm']['rounds'] <= a['lm']['rounds'] < b['lm']['rounds'] + 4
    for k in ('vel', 'vel_err', 'chisq', 'vsini', 'nm_vel'):
        assert torch.equal(a[k], b[k]), k
    for k in su['names']:
        assert torch.equal(a['param'][k], b['param'][k]), k
    assert a['objective_evals'] >= b['objective_evals'] > 0


# ---- 5. refusals ----------------------------------------------------------------------------
def test_process_lm_refuses_what_the_gradient_does_not_cover(cases, setups, monkeypatch):
    """each a ValueError naming second_minimizer_lm, from process itself and before
    anything is built"""
    import itertools
    import os
    from conftest import GOLD
    from rvspecfit_amd import optimizer, spec_fit, spec_inter, vel_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    su = setups['grid']
    stars = _fake_stars(cases, 2)
    batch = SpecBatch.from_specdata(stars)
    pd0 = {k: np.full(2, v) for k, v in PD0_STARS.items()}
    lmk = dict(second_minimizer=True, second_minimizer_lm=True)
    cfg = dict(su['cfg'], **lmk)
    name = 'second_minimizer_lm'

    def never(*a, **k):
        raise AssertionError('something was built before the scope was checked')
    monkeypatch.setattr(optimizer, 'ProcessObjective', never)
    monkeypatch.setattr(spec_fit, 'chisq_grid_jobs', never)
    with pytest.raises(ValueError, match=name):
        vel_fit.process(batch, dict(pd0), options=dict(npoly=NPOLY),
                        config=dict(cfg, second_minimizer_jac=True))
    with pytest.raises(ValueError, match=name + '.*npoly'):
        vel_fit.process(batch, dict(pd0), options=dict(npoly=17), config=cfg)
    rp = {a.name: spec_fit.construct_resol_mat(a.lam_host, 2500.) for a in batch.arms}
    with pytest.raises(ValueError, match=name + '.*resolution matrix'):
        vel_fit.process(batch, dict(pd0), options=dict(npoly=NPOLY), config=cfg,
                        resolParams=rp)
    # an MLP library (the network of nn_case.npz) without nn_gradient
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
    with pytest.raises(ValueError, match=name + '.*nn library'):
        vel_fit.process(nnb, dict(pd0), options=dict(npoly=5),
                        config=dict(GOLD_CONFIG, template_lib='golden-nn://', **lmk))
    # six stellar parameters and a fitted vsini: seven tangents
    nd = 6
    lam = stars[0][0].lam
    pts = np.array(list(itertools.product([0., 1.], repeat=nd)))
    tl = np.exp(np.linspace(np.log(lam[0] - 30), np.log(lam[-1] + 30), 1500))
    six = dict(lam=tl, log_step=np.array(True), log_ids=np.array([], dtype=int),
               parnames=np.array(['p%d' % i for i in range(nd)]),
               dats=np.zeros((2**nd, len(tl)), dtype=np.float32),
               idgrid=np.arange(2**nd).reshape((2, ) * nd), vec=pts.T.copy())
    for i in range(nd):
        six['uvec%d' % i] = np.array([0., 1.])
    spec_inter.register_library(TemplateLibrary('gold_b', six), 'golden-six-lm://')
    pd6 = {'p%d' % i: np.full(2, 0.5) for i in range(nd)}
    pd6['vsini'] = np.full(2, 5.0)
    with pytest.raises(ValueError, match=name + '.*vsini'):
        vel_fit.process(batch, pd6, options=dict(npoly=NPOLY),
                        config=dict(GOLD_CONFIG, template_lib='golden-six-lm://', **lmk))
    # more spectra than 24 chunks of the budget's rows
    monkeypatch.setattr(optimizer, "GRAD_CHAIN_BUDGET", 1 << 19)   # one row per chunk
    big = SpecBatch.from_specdata(_fake_stars(cases, 2) * 13)
    pdb = {k: np.full(26, v[0]) for k, v in pd0.items()}
    with pytest.raises(ValueError, match=name + '.*GRAD_CHAIN_BUDGET'):
        vel_fit.process(big, pdb, options=dict(npoly=NPOLY), config=cfg)
