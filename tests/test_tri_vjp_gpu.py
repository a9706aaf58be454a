"""Value and gradient on Delaunay libraries by one adjoint row contracted with the
simplex's tangents: rvs_template_tri_vjp, rvs_bfgs_run_grad_fused_tri and the
calls that take them with config['fused_gradient'] and config['tri_gradient'] together.

Fixtures: the golden Delaunay arms (ndim 4, 5718 simplices, ntp 977 / 781: ragged against
the wave and the block) with tri_grad_truth.JOBS -- six jobs inside a simplex, one outside
the hull, one with a non-finite mapped parameter -- and the synthetic triangulations of
tests/test_tri_grad_gpu.py through the C entry points.

Bounds: rvs_template_tri_vjp is held to VJP_REL_BOUND = 10 x the figure of its float64
numpy restatement (tests/test_tri_vjp_cpu.py), relative to sum_n |tbar_n dt_n/dp_k|; the
velocity and vsini components of the calls above it to the fused kernel's bound
(tests/test_objective_grad_gpu.py), the parameter components to that plus VJP_REL_BOUND
carried through sum over the arms of sum_n |tbar_n dt_n/dp_k| of the truth.

MI355X (VJP_REL_BOUND 1.98e-15 in that run): rvs_template_tri_vjp against the truth 6.59e-16 at
worst on the golden arms, 5.45e-16 on the two-triangle libraries, 3.64e-16 on the simplex in
six dimensions; against the device's own tangent rows 2.75e-16 at worst.  The gradient with
both keys against float64 autograd 7.99e-12 (npoly 5) and 3.22e-12 (npoly 10) in _rel_err's
metric, the vsini component of the broadened job 1.38e-13; chisq_func_grad against the
chain 1.39e-13.  The rounds: nit 26 / 13 / 7, njev 28 / 60 / 48 on both machines."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG
from oracle import rvs_oracle as orc

import tri_grad_truth as ttruth
import tri_vjp_truth as tv
import vsini_grad_truth as vtruth
from chisq_grad_truth import C_KMS, marginal_chisq, ortho_basis, spline_eval
from test_objective_grad_gpu import REL_ERR_BOUND as FUSED_BOUND
from test_tri_grad_gpu import _SynthLib, _call, _rel_err, _same

pytestmark = pytest.mark.gpu
J = len(ttruth.JOBS)
ND = 4
URL = 'golden-tri://'
NOSX = [ttruth.NO_SIMPLEX, ttruth.NONFINITE]
PD0 = dict(teff=6000.0, logg=2.5, feh=-0.4, alpha=0.1, vsini=30.0)


@pytest.fixture(scope='module')
def setup(cases):
    from rvspecfit_amd import _lib, spec_inter, spec_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    cfg = dict(GOLD_CONFIG, template_lib=URL)
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, ttruth.tri_lib_dict(n)), URL)
    sds = ttruth.spectra(cases, spec_fit.SpecData)
    batch = SpecBatch.from_specdata(sds)
    libs = spec_inter.get_libs(batch.names, cfg)
    assert all(l.kind == 'triangulation' and l._tri_bk is not None for l in libs.values())
    dev = batch.device
    f64 = dict(dtype=torch.float64, device=dev)
    olibs, gcases = tv.golden_cases()
    rng = np.random.default_rng(77)
    # the adjoint rows of the kernel tests: those of the CPU yardstick on the jobs inside
    # a simplex, seeded rows of the same kind on the two others
    tbar = {}
    for n in ('gold_b', 'gold_r'):
        rows = [c[4] for c in gcases if c[0] == n]
        rows += [tv.adjoint_row(rng, len(rows[0])) for _ in NOSX]
        tbar[n] = torch.as_tensor(np.array(rows)).to(dev)
    return dict(cfg=cfg, both=dict(cfg, fused_gradient=True, tri_gradient=True), sds=sds,
                batch=batch, libs=libs, dev=dev, olibs=olibs, tbar=tbar,
                want={(c[0], c[1]): (c[5], c[6]) for c in gcases},
                names=list(spec_inter.getSpecParams('gold_b', cfg)),
                idx=torch.tensor([j[0] for j in ttruth.JOBS], device=dev),
                vel=torch.tensor([j[1] for j in ttruth.JOBS], **f64),
                par=torch.tensor([j[2] for j in ttruth.JOBS], **f64),
                vs=torch.tensor([j[3] or 0.0 for j in ttruth.JOBS], **f64))


def _ld_contract(tbar, rows):
    """sum_n tbar[j, n] rows[j, k, n] in long double on the host: [J, ndim]"""
    return (tbar.cpu().numpy().astype(np.longdouble)[:, None, :] *
            rows.cpu().numpy().astype(np.longdouble)).sum(axis=2)


# ---- 1. the kernel against the truth ----------------------------------------------------------
@pytest.mark.parametrize('B', [1, 3, 8])
@pytest.mark.parametrize('name', ['gold_b', 'gold_r'])
def test_vjp_against_the_truth_on_the_golden_arms(setup, name, B):
    """against the long-double contraction of template_jacobian and against the same
    contraction of the rows 1 + k rvs_template_tri_grad writes on the device, both within
    VJP_REL_BOUND of sum_n |tbar_n dt_n/dp_k|; B = 8 holds the two rows without a simplex:
    exact zeros.  (MI355X figures: see DESIGN 4.26.)"""
    su = setup
    lib = su['libs'][name]
    P, TB = su['par'][:B].contiguous(), su['tbar'][name][:B].contiguous()
    t, out, sx, _ = lib.eval_batch(P, details=True)
    got = lib.tri_vjp(P, t, sx, TB)
    assert got.shape == (B, ND)
    rows, _ = lib.eval_batch_grad(P)
    host = _ld_contract(TB, rows[:, 1:])
    g = got.cpu().numpy()
    bound = tv.vjp_rel_bound()
    worst = worst_h = 0.0
    for j in range(B):
        if j in NOSX:
            assert int(sx[j].item()) == 0x7fffffff and t[j].isnan().all()
            assert not g[j].any() and not np.signbit(g[j]).any()
            continue
        want, scale = su['want'][name, j]
        m, mh = tv.metric(g[j], want, scale), tv.metric(g[j], host[j], scale)
        print('%s B %d job %d: against the truth %s, against the device\'s tangent rows %s'
              % (name, B, j, m, mh))
        worst, worst_h = max(worst, m.max()), max(worst_h, mh.max())
    print('%s B %d: largest %.3g / %.3g, bound %.3g' % (name, B, worst, worst_h, bound))
    assert worst <= bound and worst_h <= bound


def _synth_vjp(sl, params, tbar, dev):
    """rvs_template_tri, then rvs_template_tri_vjp on its rows and ids, on the arrays of a
    _SynthLib: (templ, simplex, gparams)"""
    from rvspecfit_amd import _lib
    nd, ntp = sl.ndim, sl.dats.shape[1]
    B = len(params)
    t, _, sx, _ = _call(sl, params, False, dev)
    f64 = dict(dtype=torch.float64, device=dev)
    keep = [torch.as_tensor(sl.dats).to(dev).contiguous(),
            torch.as_tensor(sl.simplices).to(dev).contiguous(),
            torch.as_tensor(sl.transform).to(dev).contiguous(),
            torch.as_tensor(np.asarray(params, dtype=np.float64)).to(dev).contiguous(),
            torch.as_tensor(tbar).to(dev).contiguous()]
    gp = torch.full((B, nd), -7.0, **f64)
    rc = _lib.lib().rvs_template_tri_vjp(
        _lib.ptr(keep[0]), ntp, _lib.ptr(keep[1]), _lib.ptr(keep[2]), len(sl.simplices),
        nd, sum(1 << i for i in sl.log_ids), int(sl.exp), _lib.ptr(keep[3]), B,
        _lib.ptr(sx), _lib.ptr(t), _lib.ptr(keep[4]), _lib.ptr(gp), _lib.stream())
    _lib.check(rc, 'rvs_template_tri_vjp')
    torch.cuda.synchronize()
    return t, sx, gp


def _check_synthetic(sl, params, dev, nfound, seed):
    rng = np.random.default_rng(seed)
    ntp = sl.dats.shape[1]
    tbar = np.array([tv.adjoint_row(rng, ntp) for _ in params])
    t, sx, gp = _synth_vjp(sl, params, tbar, dev)
    tg = _call(sl, params, True, dev)[0]
    host = _ld_contract(torch.as_tensor(tbar), tg[:, 1:])
    g, sx = gp.cpu().numpy(), sx.cpu().numpy()
    bound = tv.vjp_rel_bound()
    found, worst, worst_h = 0, 0.0, 0.0
    for j, p in enumerate(params):
        if sx[j] == 0x7fffffff:
            assert not g[j].any()
            continue
        found += 1
        _, want, scale = tv.truth(sl, p, tbar[j])
        worst = max(worst, tv.metric(g[j], want, scale).max())
        worst_h = max(worst_h, tv.metric(g[j], host[j], scale).max())
    print('ntp %d nd %d exp %d log %s: against the truth %.3g, against the device\'s '
          'tangent rows %.3g, bound %.3g' % (ntp, sl.ndim, sl.exp, sl.log_ids, worst,
                                             worst_h, bound))
    assert found == nfound
    assert worst <= bound and worst_h <= bound


@pytest.mark.parametrize('ntp', [33, 64, 257])
@pytest.mark.parametrize('exp_flag,log_ids', [(1, ()), (1, (0, )), (0, ()), (0, (0, ))])
def test_two_triangles(setup, ntp, exp_flag, log_ids):
    """a square split into two triangles (ndim 2); ntp below a wave, one wave, one knot
    beyond the block; with and without exp; with and without a log-mapped parameter; two
    of the seven points outside"""
    rng = np.random.default_rng(100 * ntp + 10 * exp_flag + len(log_ids))
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    sl = _SynthLib(pts, [[0, 1, 2], [1, 3, 2]],
                   0.5 * rng.standard_normal((4, ntp)) - 2.0,
                   np.array([0.0, 0.0, 0.0, 1.0]), log_ids, exp_flag)
    q = np.array([[0.2, 0.3], [0.6, 0.1], [0.7, 0.8], [0.45, 0.9], [0.31, 0.32],
                  [1.5, 0.5], [0.5, -0.2]])       # mapped; the last two outside
    params = q.copy()
    if 0 in log_ids:
        params[:, 0] = 10.0**q[:, 0]
    _check_synthetic(sl, params, setup['dev'], 5, ntp + exp_flag)


def test_six_dimensions(setup):
    """one 7-vertex simplex in six dimensions (the most the kernel takes), two log-mapped
    parameters, ntp = 300"""
    rng = np.random.default_rng(6)
    nd = 6
    pts = np.vstack([np.full(nd, 0.1), 0.1 + np.diag(rng.uniform(0.5, 2.0, nd))])
    pts += 0.05 * rng.standard_normal(pts.shape)
    sl = _SynthLib(pts, [list(range(nd + 1))], 0.5 * rng.standard_normal((7, 300)) - 2.0,
                   rng.integers(0, 2, 7).astype(np.float64), (0, 3), 1)
    b = rng.dirichlet(np.ones(nd + 1), size=3)
    q = np.vstack([b @ pts, pts.mean(axis=0)[None, :] + 5.0])    # the last one outside
    params = q.copy()
    for i in sl.log_ids:
        params[:, i] = 10.0**q[:, i]
    _check_synthetic(sl, params, setup['dev'], 3, 66)


# ---- 2. exact properties ------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['gold_b', 'gold_r'])
def test_vjp_exact_properties(setup, name):
    """two calls: the same bits; a job alone, in a batch of three and under a permuted job
    list: the bits it has among all eight; tbar scaled by 2^+-100: results scaled by exactly
    that power; a zero tbar: exact zeros; the two rows without a simplex: exact zeros,
    their neighbours the bits of the call without them"""
    su = setup
    lib = su['libs'][name]
    P, TB = su['par'], su['tbar'][name]
    t, _, sx, _ = lib.eval_batch(P, details=True)
    a = lib.tri_vjp(P, t, sx, TB)
    assert torch.equal(a, lib.tri_vjp(P, t, sx, TB))
    assert torch.isfinite(a).all() and a[ttruth.INSIDE].all()
    for j in range(J):
        one = lib.tri_vjp(P[j:j + 1], t[j:j + 1], sx[j:j + 1], TB[j:j + 1])
        assert torch.equal(one[0], a[j]), j
    assert torch.equal(lib.tri_vjp(P[2:5], t[2:5], sx[2:5], TB[2:5]), a[2:5])
    perm = torch.tensor([4, 2, 6, 0, 7, 5, 1, 3], device=su['dev'])
    assert torch.equal(lib.tri_vjp(P[perm], t[perm], sx[perm], TB[perm]), a[perm])
    for k in (100, -100):
        assert torch.equal(lib.tri_vjp(P, t, sx, torch.ldexp(TB, torch.tensor(k))),
                           torch.ldexp(a, torch.tensor(k))), k
    z = lib.tri_vjp(P, t, sx, torch.zeros_like(TB))
    assert not z.any() and not torch.signbit(z).any()
    assert t[NOSX].isnan().all() and not a[NOSX].any()
    ins = torch.tensor(ttruth.INSIDE, device=su['dev'])
    assert torch.equal(lib.tri_vjp(P[ins], t[ins], sx[ins], TB[ins]), a[ins])


# ---- 3. end to end ----------------------------------------------------------------------------
_adjoint = {}


def _param_allowance(cases, su, npoly, j, vsini_grad=False):
    """sum over the arms of sum_n |tbar_n dt_n/dp_k| [ndim] of job j: tbar = d chisq / d t
    by float64 autograd with the arm's template row as the leaf (the statements of
    tri_grad_truth.chisq_and_grad behind the row), dt/dp = template_jacobian"""
    key = (npoly, j, vsini_grad)
    if key not in _adjoint:
        s, vel, par, vs = ttruth.JOBS[j]
        tot = np.zeros(ND)
        for sd in ttruth.spectra(cases, orc.SpecData)[s]:
            lib = su['olibs'][sd.name]
            t0, jac = ttruth.template_jacobian(lib, par)
            leaf = torch.tensor(t0, requires_grad=True)
            t = leaf
            if vsini_grad:
                t = vtruth.broadened(lib, t, torch.tensor(float(vs), dtype=torch.float64))
            elif vs is not None and vs > 0:
                R = (vs / C_KMS) / np.log(lib.lam[1] / lib.lam[0])
                ker = torch.as_tensor(orc.compute_vsini_kernel(R))
                t = torch.nn.functional.conv1d(t[None, None, :], ker[None, None, :],
                                               padding=(len(ker) - 1) // 2)[0, 0]
            beta = vel / C_KMS
            xs = torch.as_tensor(sd.lam) * np.sqrt((1 - beta) / (1 + beta))
            Q, const = ortho_basis(sd.lam, npoly, True)
            marginal_chisq(spline_eval(lib.lam, t, xs), Q, const, torch.as_tensor(sd.spec),
                           torch.as_tensor(sd.espec)).backward()
            tot += np.abs(leaf.grad.numpy()[None, :] * jac).sum(axis=1)
        _adjoint[key] = tot
    return _adjoint[key]


def _within_bounds(cases, su, npoly, j, got, g, what, vsini_grad=False):
    """got against g [1 + ndim (+ 1)] in _rel_err's metric: velocity and vsini components
    within FUSED_BOUND, the parameter components within FUSED_BOUND plus VJP_REL_BOUND x
    sum |tbar dt/dp_k| over the same denominator"""
    floor = np.maximum(np.abs(g), 1e-6 * np.abs(g).max())
    rel = _rel_err(got, g)
    allowed = np.full(g.shape, FUSED_BOUND)
    allowed[1:1 + ND] += tv.vjp_rel_bound() * _param_allowance(cases, su, npoly, j,
                                                               vsini_grad) / floor[1:1 + ND]
    print('%s job %d npoly %d: rel err %s allowed %s' % (what, j, npoly, rel, allowed))
    assert (rel <= allowed).all()


def _grad_jobs(su, cfg, npoly, vsini_grad=False, order=None):
    from rvspecfit_amd import spec_fit
    sel = torch.tensor(list(range(J)) if order is None else order, device=su['dev'])
    return spec_fit.chisq_grad_jobs(su['batch'], su['idx'][sel], su['vel'][sel],
                                    su['par'][sel], su['vs'][sel], dict(npoly=npoly),
                                    su[cfg], vsini_grad=vsini_grad)


@pytest.mark.parametrize('npoly', [5, 10])
def test_gradient_with_both_keys_against_the_truth(cases, setup, npoly):
    """chisq_grad_jobs on all of JOBS and get_chisq_grad on the batch (spectra 0, 1, 2 at
    jobs 0, 1, 2) with both keys: value to 1e-7 of the truth and to 1e-11 max(|value|, 1e3)
    of the chain's, gradient within the bounds of _within_bounds; the rows without a simplex
    the chain's, NaN and zero pattern included; the broadened job with vsini_grad against
    the truth with the vsini component"""
    from rvspecfit_amd import spec_fit
    su = setup
    want = ttruth.truth_jobs(cases, su['olibs'], npoly)
    chi, grad, st = _grad_jobs(su, 'both', npoly)
    ref, gref, rst = _grad_jobs(su, 'cfg', npoly)
    assert chi.shape == (J, ) and grad.shape == (J, 1 + ND)
    assert torch.equal(st, rst)
    g_all = grad.cpu().numpy()
    for j in ttruth.INSIDE:
        val, g = want[j]
        a, b = chi[j].item(), ref[j].item()
        assert int(st[j].item()) == 0
        assert abs(a - val) <= 1e-7 * abs(val)
        assert abs(a - b) <= 1e-11 * max(abs(b), 1e3), (j, a, b)
        _within_bounds(cases, su, npoly, j, g_all[j], g, 'chisq_grad_jobs')
    for j in NOSX:
        assert chi[j].item() == 2 * 1000.0 * su['batch'].badchi == want[j][0]
        assert _same(chi[j], ref[j]) and _same(grad[j], gref[j])
        assert not g_all[j].any()
    cb, gb = spec_fit.get_chisq_grad(su['batch'], su['vel'][:3], su['par'][:3],
                                     options=dict(npoly=npoly), config=su['both'])
    assert torch.equal(cb, chi[:3]) and torch.equal(gb, grad[:3])
    # the broadened job, vsini fitted
    j = ttruth.BROADENED
    s, vel, par, vs = ttruth.JOBS[j]
    val, g = ttruth.chisq_and_grad(ttruth.spectra(cases, orc.SpecData)[s], su['olibs'],
                                   vel, par, vs, npoly=npoly, vsini_grad=True)
    c3, g3 = spec_fit.get_chisq_grad(su['sds'][s], vel, par, (vs, ),
                                     options=dict(npoly=npoly), config=su['both'],
                                     vsini_grad=True)
    assert g3.shape == (2 + ND, ) and g[1 + ND] != 0
    assert abs(c3 - val) <= 1e-7 * abs(val)
    _within_bounds(cases, su, npoly, j, g3, g, 'get_chisq_grad, vsini fitted', True)
    cv, gv, _ = _grad_jobs(su, 'both', npoly, vsini_grad=True)
    assert gv.shape == (J, 2 + ND) and c3 == cv[j].item()
    assert (gv[j].cpu().numpy() == g3).all()


def test_chisq_grad_jobs_in_chunks(setup, monkeypatch):
    """chisq_grad_jobs with both keys under byte budgets of less than one job's rows
    (chunks of one), of three jobs' rows (3, 3, 2) and the default (one chunk): the same
    bits; the jobs permuted: the permuted rows"""
    from rvspecfit_amd import engine
    su = setup
    one = _grad_jobs(su, 'both', 10, vsini_grad=True)
    per_job = sum(16 * lib.ntp + 8 * ND + 4 for lib in su['libs'].values())
    assert per_job == 16 * (977 + 781) + 2 * 36
    for budget in (100, 3 * per_job):
        monkeypatch.setattr(engine, 'TBAR_BUDGET', budget)
        got = _grad_jobs(su, 'both', 10, vsini_grad=True)
        assert all(_same(a, b) for a, b in zip(got, one)), budget
    monkeypatch.undo()
    perm = [4, 2, 6, 0, 7, 5, 1, 3]
    sel = torch.tensor(perm, device=su['dev'])
    got = _grad_jobs(su, 'both', 10, vsini_grad=True, order=perm)
    assert all(_same(a, b[sel]) for a, b in zip(got, one))


def test_chisq_func_grad_both_keys(cases, setup):
    """vel_fit.chisq_func_grad with a Normal prior on teff and alpha fixed, both keys
    against the chain: the value to 1e-11 max(|f|, 1e3), the gradient within the bounds of
    test_gradient_with_both_keys_against_the_truth (_within_bounds) around the chain's"""
    from rvspecfit_amd import vel_fit
    su = setup
    names = su['names']
    j = ttruth.BROADENED
    s, vel, par, vs = ttruth.JOBS[j]

    def run(cfg):
        mapper = vel_fit.ParamMapper(names, dict(zip(names, par)), ['alpha'],
                                     vel_fit.VSiniMapper(cfg['max_vsini']), fitVsini=True)
        args = dict(specdata=su['sds'][s], paramMapper=mapper, options=dict(npoly=10),
                    config=cfg, priors={'teff': (5800.0, 150.0)}, min_vel=cfg['min_vel'],
                    max_vel=cfg['max_vel'])
        assert mapper.get_fitted_params() == ['vel', 'vsini', 'teff', 'logg', 'feh']
        return vel_fit.chisq_func_grad(np.array([vel, vs] + list(par[:3])), args)
    f1, g1 = run(su['both'])
    f0, g0 = run(su['cfg'])
    assert g1.shape == g0.shape == (5, ) and g1.all()
    assert abs(f1 - f0) <= 1e-11 * max(abs(f0), 1e3)
    floor = np.maximum(np.abs(g0), 1e-6 * np.abs(g0).max())
    allowed = np.full(5, FUSED_BOUND)
    allowed[2:] += tv.vjp_rel_bound() * _param_allowance(cases, su, 10, j,
                                                         True)[:3] / floor[2:]
    rel = np.abs(g1 - g0) / floor
    print('chisq_func_grad: rel err %s allowed %s' % (rel, allowed))
    assert (rel <= allowed).all()


# ---- 4. the rounds ------------------------------------------------------------------------------
def _objective(su, S, cfg):
    from rvspecfit_amd import optimizer
    batch = su['batch'].subset(torch.arange(S, device=su['dev']))
    pdt = {k: torch.full((S, ), float(v), dtype=torch.float64, device=su['dev'])
           for k, v in PD0.items()}
    safe = torch.stack([pdt[k] for k in su['names']], dim=1).contiguous()
    return optimizer.ProcessObjective(batch, su['libs'], su['names'], pdt, [], True, cfg,
                                      dict(npoly=10), None, safe)


@pytest.fixture(scope='module')
def nm_start(setup):
    """the simplex optimum of the three golden stars, as vel_fit.process reaches it"""
    from rvspecfit_amd import vel_fit
    su = setup
    r = vel_fit.process(su['batch'], {k: np.full(3, v) for k, v in PD0.items()},
                        options=dict(npoly=10), config=dict(su['cfg']))
    v = dict(vel=r['nm_vel'], vsini=r['vsini'])
    v.update({k: r['param'][k] for k in su['names']})
    cols = ['vel', 'vsini'] + su['names']
    return cols, torch.stack([v[c].double() for c in cols], dim=1).contiguous()


@pytest.mark.parametrize('cap', [None, 2])
def test_run_grad_fused_tri_equals_the_host_machine(setup, nm_start, cap):
    """rvs_bfgs_run_grad_fused_tri (the sequence of DESIGN 4.26 in C) against
    bfgs.minimize_lockstep_native(jac=True) around GradChain(fused=True).rows (the same
    entry points driven from Python), three golden stars from the simplex optimum, vsini
    fitted, in one chunk and with cap = 2 in two: equal counters, equal bits"""
    from rvspecfit_amd import bfgs, optimizer, vel_fit
    su = setup
    S = 3
    cols, x0 = nm_start
    pobj = _objective(su, S, su['both'])
    chain = optimizer.GradChain(pobj, fused=True, cap=cap)
    assert chain.fused and chain.fused_tri and not chain.fused_nn
    assert chain.cap == (cap or S) and chain.nbytes > 0
    per_row = sum(8 * lib.ntp + 8 * ND for lib in su['libs'].values())
    assert chain.nbytes >= chain.cap * per_row
    H0 = vel_fit.get_hess_inv(cols)
    dev_r = bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=H0, jac=True, chain=chain)
    host = bfgs.minimize_lockstep_native(chain.rows, x0.cpu().numpy(), hess_inv0=H0,
                                         jac=True)
    d = {k: dev_r[k].cpu().numpy() for k in ('x', 'fun', 'nit', 'nfev', 'njev', 'status')}
    print('device nit', d['nit'], 'nfev', d['nfev'], 'njev', d['njev'], 'status',
          d['status'], 'fun', d['fun'])
    print('host   nit', host['nit'], 'nfev', host['nfev'], 'njev', host['njev'],
          'status', host['status'], 'fun', host['fun'])
    for k in ('nit', 'nfev', 'njev', 'status'):
        assert np.array_equal(d[k], host[k]), k
    assert np.array_equal(d['x'], host['x']) and np.array_equal(d['fun'], host['fun'])
    assert (d['njev'] > 0).all()
    f0 = chain.rows(np.arange(S), x0.cpu().numpy())[:, 0]
    assert (d['fun'] <= f0).all()


def test_process_with_the_fused_polish(setup):
    """vel_fit.process with second_minimizer_jac and both keys runs, through
    rvs_bfgs_run_grad_fused_tri, on two golden stars and ends no higher than the simplex
    optimum (the same call without a second minimiser) on each -- to 1e-11
    max(|chisq|, 1e3), what the value kernel's and the gradient kernel's values of one
    point may differ by"""
    from rvspecfit_amd import vel_fit
    su = setup
    batch = su['batch'].subset(torch.arange(2, device=su['dev']))
    pd0 = {k: np.full(2, v) for k, v in PD0.items()}
    opt = dict(npoly=10)
    r0 = vel_fit.process(batch, dict(pd0), options=opt, config=su['both'])
    r = vel_fit.process(batch, dict(pd0), options=opt,
                        config=dict(su['both'], second_minimizer=True,
                                    second_minimizer_jac=True))
    print('bfgs', r['bfgs'], 'chisq', r['chisq'].tolist(), 'simplex', r0['chisq'].tolist(),
          'vel', r['vel'].tolist())
    assert r['bfgs']['jac'] is True and r['bfgs']['fused'] is True
    assert (np.asarray(r['bfgs']['njev']) > 0).all()
    for k in ('vel', 'chisq', 'vsini'):
        assert torch.isfinite(r[k]).all(), k
    c, c0 = r['chisq'].cpu().numpy(), r0['chisq'].cpu().numpy()
    assert (c <= c0 + 1e-11 * np.maximum(np.abs(c0), 1e3)).all()


# ---- 5. what still raises ---------------------------------------------------------------------
def test_refusals_with_both_keys(setup, monkeypatch):
    """the Fisher matrix, the Levenberg-Marquardt polish, the joint-epoch fit, a resolution
    matrix, npoly 11, fast_interp and a grid set raise with both keys set, naming the key;
    without tri_gradient the Delaunay refusal stands; with library.TRI_BUCKETS False the
    rounds are not in the library and GradChain(fused=True) says so"""
    from rvspecfit_amd import library, optimizer, spec_fit, vel_fit
    from rvspecfit_amd.engine import SpecBatch
    su = setup
    opt = dict(npoly=5)
    b3, v3, p3 = su['batch'], su['vel'][:3], su['par'][:3]
    pd0 = {k: np.full(3, v) for k, v in PD0.items()}
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*Fisher'):
        spec_fit.get_chisq_fisher(b3, v3, p3, options=opt, config=su['both'])
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*second_minimizer_lm'):
        vel_fit.process(b3, dict(pd0), options=opt,
                        config=dict(su['both'], second_minimizer=True,
                                    second_minimizer_lm=True))
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*epochs'):
        vel_fit.process_epochs(b3, np.array([0, 0, 0]), {k: v[:1] for k, v in pd0.items()},
                               np.zeros(3), options=opt, config=su['both'])
    rp = {a.name: spec_fit.construct_resol_mat(a.lam_host, width=0.5) for a in b3.arms}
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*resolution matrix'):
        spec_fit.get_chisq_grad(b3, v3, p3, options=opt, config=su['both'],
                                resol_params=rp)
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*npoly'):
        spec_fit.get_chisq_grad(b3, v3, p3, options=dict(npoly=11), config=su['both'])
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*fast_interp'):
        spec_fit.get_chisq_grad(b3, v3, p3, options=opt, config=su['both'],
                                fast_interp=True)
    sd = su['sds'][0]
    other = [spec_fit.SpecData(x.name, x.lam[:-3], x.spec[:-3], x.espec[:-3],
                               badmask=x.badmask[:-3]) for x in su['sds'][1]]
    gs = SpecBatch.from_specdata([sd, other])
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*grid set'):
        spec_fit.get_chisq_grad(gs, su['vel'][:2], su['par'][:2], options=opt,
                                config=su['both'])
    for cfg in (dict(su['cfg'], fused_gradient=True),
                dict(su['cfg'], fused_gradient=True, nn_gradient=True)):
        with pytest.raises(ValueError, match=r'fused_gradient.*triangulation'):
            spec_fit.get_chisq_grad(b3, v3, p3, options=opt, config=cfg)
    pobj = _objective(su, 2, su['both'])
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*Fisher'):
        optimizer.GradChain(pobj, fused=True, fisher=True)
    optimizer.GradChain(pobj, fused=True)
    monkeypatch.setattr(library, 'TRI_BUCKETS', False)
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*rounds inside the library'):
        optimizer.GradChain(_objective(su, 2, su['both']), fused=True)
