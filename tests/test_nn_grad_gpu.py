"""rvs_template_nn_grad and everything that takes a gradient on MLP libraries, against
tests/nn_grad_truth.py (float64 torch on the CPU, pinned by test_nn_grad_cpu.py).  The
network is tests/golden/nn_case.npz, 4 -> 64 -> 64 -> 64 -> 40 -> 333 with log10 on teff:
40 inputs to a last layer of 333 columns, neither a multiple of a tile.

Tile paths of the launcher (csrc/nn.hip, rvs_template_nn_grad): with 1 + ndim = 5 rows per
job a 32-row tile takes 6 jobs and a 128-row tile 25; the last layer goes through 128-row
tiles from 1024 tiles on -- 3 column tiles here, so from ceil(B / 25) = 342, B = 8526 --
and through vector or scalar operand loads as its input width is or is not a multiple
of 4 (40, and 39 in a copy of the network cut to that width).  B = 1, 7, 27 cross a
32-row tile in mid-job and leave tails; 8526 is the first batch on 128-row tiles.

MI355X figures (tangent metric: per job and parameter, max_pix |got - truth| /
max_pix |truth|): see the docstring of test_template_rows."""
import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG

import nn_grad_truth as nt
from test_chisq_grad_gpu import REL_ERR_BOUND
from test_chisq_fisher_gpu import BOUND as FISHER_BOUND

pytestmark = pytest.mark.gpu
ND = nt.NDIM
R = 1 + ND
BIG_B = 8526          # 3 * ceil(8526 / 25) = 1026 >= 1024 tiles of 128 rows; 8525: 1023
URL = 'golden-nn-grad://'
NAME = 'aat_580v'
LAM = np.exp(np.linspace(np.log(3950.), np.log(5060.), 333))
NPOLY = 5


def _same(a, b):
    """bit for bit, NaN == NaN"""
    return torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


def _cut39(net):
    """the network with its last hidden layer cut to 39 units: the last layer's input
    width is then no multiple of 4 (scalar operand loads)"""
    W, b = list(net['W']), list(net['b'])
    W[-2], b[-2], W[-1] = W[-2][:39].copy(), b[-2][:39].copy(), W[-1][:, :39].copy()
    dims = np.array(net['dims'], dtype=np.int32)
    dims[-2] = 39
    return dict(net, W=W, b=b, dims=dims)


@pytest.fixture(scope='module')
def nets():
    net = nt.network()
    return dict(k40=net, k39=_cut39(net))


@pytest.fixture(scope='module')
def libs(nets):
    from rvspecfit_amd import _lib
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    return {k: TemplateLibrary(NAME, nt.lib_dict(n, LAM)) for k, n in nets.items()}


_truths = {}


def _truth(nets, which, B):
    """(points, truth template, truth tangents, float32-statement metric) -- once"""
    if (which, B) not in _truths:
        p = nt.points(nets[which], B, seed=B)
        t, jac = nt.jacobian64(nets[which], p)
        _, jac32 = nt.forward32(nets[which], p)
        _truths[which, B] = (p, t, jac, nt.tangent_metric(jac32, jac))
    return _truths[which, B]


# ---- 1. the template rows against the truth ----------------------------------------------
@pytest.mark.parametrize('which,B', [('k40', 1), ('k40', 7), ('k40', 27), ('k40', BIG_B),
                                     ('k39', 7), ('k39', BIG_B)])
def test_template_rows(nets, libs, which, B):
    """row 0 is eval_batch's template bit for bit, the outside flags are eval_batch's;
    every tangent row of every job within 4 x the largest error of the float32 CPU
    statement at the same points (the factor covers the MFMA's summation order).

    MI355X, first device run (largest tangent metric, device / float32 CPU statement):
      k40: B 1 4.94e-07 / 4.24e-07, B 7 4.82e-07 / 4.50e-07, B 27 5.84e-07 / 5.83e-07,
           B 8526 7.71e-07 / 9.40e-07
      k39: B 7 4.80e-07 / 4.69e-07, B 8526 7.82e-07 / 8.44e-07"""
    lib = libs[which]
    p, t, jac, m32 = _truth(nets, which, B)
    P = torch.as_tensor(p).to(lib.device)
    t0, o0 = lib.eval_batch(P)
    tg, og = lib.eval_batch_grad(P)
    assert tg.shape == (B, R, lib.ntp) and og.shape == (B, )
    assert torch.equal(tg[:, 0], t0) and torch.equal(og, o0)
    assert not og.any()                       # inside the training hull
    got = tg.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.abs(got[:, 0] / t - 1).max() < 3e-6     # (the value path's golden bound)
    m = nt.tangent_metric(got[:, 1:], jac)
    assert m.shape == (B, ND)
    print('%s B %d: largest tangent metric %.3g (job %d), float32 CPU statement %.3g, '
          'bound %.3g' % (which, B, m.max(), int(m.max(axis=1).argmax()), m32.max(),
                          4 * m32.max()))
    assert (m <= 4 * m32.max()).all()


# ---- 2. clip and non-finite input ----------------------------------------------------------
def test_clip_is_flat(nets):
    """a last-layer bias of 400 / -400: row 0 there is exp(+-300), the tangent rows
    exactly 0, every other column the bits of the unchanged network"""
    from rvspecfit_amd.library import TemplateLibrary
    net = nets['k40']
    hot = dict(net, b=[b.copy() for b in net['b']])
    hot['b'][-1][5], hot['b'][-1][200] = 400.0, -400.0
    P = torch.as_tensor(nt.points(net, 27, seed=2)).to('cuda')
    tg, _ = TemplateLibrary(NAME, nt.lib_dict(net, LAM)).eval_batch_grad(P)
    hlib = TemplateLibrary(NAME, nt.lib_dict(hot, LAM))
    th, _ = hlib.eval_batch_grad(P)
    assert torch.equal(th[:, 0], hlib.eval_batch(P)[0])
    assert (th[:, 0, 5] / np.exp(300.0) - 1).abs().max().item() < 1e-14
    assert (th[:, 0, 200] / np.exp(-300.0) - 1).abs().max().item() < 1e-14
    assert not th[:, 1:, [5, 200]].any()
    keep = [c for c in range(333) if c not in (5, 200)]
    assert torch.equal(th[:, :, keep], tg[:, :, keep])
    assert tg[:, 1:, [5, 200]].all()


def test_non_finite_jobs(nets, libs):
    """NaN logg, teff = -5 (log10 of a negative number): all five rows NaN, outside
    NaN; the other jobs of the same tiles keep their bits"""
    lib = libs['k40']
    p = nt.points(nets['k40'], 27, seed=3)
    P = torch.as_tensor(p).to(lib.device)
    clean, oc = lib.eval_batch_grad(P)
    p[3, 1] = np.nan
    p[11, 0] = -5.0
    tg, og = lib.eval_batch_grad(torch.as_tensor(p).to(lib.device))
    bad = torch.zeros(27, dtype=torch.bool, device=lib.device)
    bad[[3, 11]] = True
    assert tg[bad].isnan().all() and og[bad].isnan().all()
    assert torch.equal(tg[~bad], clean[~bad]) and torch.equal(og[~bad], oc[~bad])


# ---- 3. repeatability -----------------------------------------------------------------
def test_two_calls_and_job_by_job(nets, libs):
    """two calls: the same bits; a batch equals its jobs evaluated one by one (a tangent
    that read another job's value row would not)"""
    lib = libs['k40']
    P = torch.as_tensor(nt.points(nets['k40'], 27, seed=4)).to(lib.device)
    a, oa = lib.eval_batch_grad(P)
    b, ob = lib.eval_batch_grad(P)
    assert torch.equal(a, b) and torch.equal(oa, ob)
    for j in range(27):
        one, oo = lib.eval_batch_grad(P[j:j + 1])
        assert torch.equal(one[0], a[j]) and torch.equal(oo[0], oa[j]), j


# ---- 4. the chain behind the rows -------------------------------------------------------
S = 3
VEL = [12.5, -83.0, 140.25]
VSINI = [380.0, 250.0, 520.0]        # R = vsini / (c lnstep) = 1.70, 1.12, 2.33


@pytest.fixture(scope='module')
def chain(nets, libs):
    """three noisy spectra of the network's own templates on a 257-pixel grid, the
    library registered under a URL of its own"""
    from rvspecfit_amd import spec_inter, spec_fit
    from rvspecfit_amd.engine import SpecBatch
    net = nets['k40']
    lib = libs['k40']
    spec_inter.register_library(lib, URL)
    cfg = dict(GOLD_CONFIG, template_lib=URL, max_vsini=600)
    rng = np.random.RandomState(5)
    wave = np.linspace(4000., 5000., 257)
    par = nt.points(net, S, seed=6)
    t = nt.jacobian64(net, par)[0]
    sds = []
    for s in range(S):
        f = np.sqrt((1 - VEL[s] / nt.C_KMS) / (1 + VEL[s] / nt.C_KMS))
        m = np.interp(wave * f, LAM, t[s]) * (1.0 + 0.1 * (wave - 4500.) / 500.)
        e = np.full(257, 0.02)
        sds.append([spec_fit.SpecData(NAME, wave, m + e * rng.normal(size=257), e)])
    batch = SpecBatch.from_specdata(sds)
    # The points of the calls: well off the spectra's own parameters (every mapped
    # coordinate up to 10 % nearer the origin).  At the optimum each component of the
    # gradient is the difference of sums that cancel, and the gradient metric
    # (relative to max(|g_k|, 1e-6 |g|_inf)) then measures the rounding of that
    # cancellation on either side, not the wiring this test is about.
    par = nt.points(net, S, seed=6, shrink=0.1)
    return dict(cfg=cfg, sds=sds, batch=batch, lib=lib, wave=wave, par=par,
                P=torch.as_tensor(par).to(lib.device))


def _rel_err(got, g):
    return np.abs(got - g) / np.maximum(np.abs(g), 1e-6 * np.abs(g).max())


@pytest.mark.parametrize('vsini_grad', [False, True])
def test_gradient_and_fisher_of_the_device_rows(chain, vsini_grad):
    """spec_fit.get_chisq_grad / get_chisq_fisher with config['nn_gradient'] against
    float64 torch applied to the device's own template rows (eval_batch_grad copied to
    the host): chi^2 as tests/chisq_grad_truth.py states it, autograd's gradient by the
    template contracted with each tangent row, the velocity (and vsini) derivative
    directly, the Fisher matrix as tests/chisq_fisher_truth.py builds it.  Metrics and
    bounds of test_chisq_grad_gpu.py (REL_ERR_BOUND of max(|g_k|, 1e-6 |g|_inf), value
    to 1e-7) and test_chisq_fisher_gpu.py (BOUND of sqrt(G_ii G_ll), cond(A) < 100)."""
    from rvspecfit_amd import spec_fit
    su = chain
    cfg = dict(su['cfg'], nn_gradient=True)
    opt = dict(npoly=NPOLY)
    vel = torch.tensor(VEL, dtype=torch.float64, device=su['lib'].device)
    rot = torch.tensor(VSINI, dtype=torch.float64, device=su['lib'].device) \
        if vsini_grad else None
    chi, grad = spec_fit.get_chisq_grad(su['batch'], vel, su['P'], rot, options=opt,
                                        config=cfg, vsini_grad=vsini_grad)
    chi2, grad2, F = spec_fit.get_chisq_fisher(su['batch'], vel, su['P'], rot,
                                               options=opt, config=cfg,
                                               vsini_grad=vsini_grad)
    K = 1 + ND + (1 if vsini_grad else 0)
    assert grad.shape == (S, K) and F.shape == (S, K, K)
    assert torch.equal(chi, chi2) and torch.equal(grad, grad2)
    assert torch.equal(F, F.transpose(1, 2))
    rows, outside = su['lib'].eval_batch_grad(su['P'])
    assert not outside.any()
    rows = rows.cpu().numpy()
    grad, F = grad.cpu().numpy(), F.cpu().numpy()
    worst_g = worst_f = 0.0
    for s in range(S):
        sd = su['sds'][s][0]
        w = nt.chain_truth([(sd.lam, sd.spec, sd.espec, LAM, rows[s])], VEL[s],
                           VSINI[s] if vsini_grad else None, NPOLY, vsini_grad)
        assert abs(chi[s].item() - w['chi']) <= 1e-7 * abs(w['chi'])
        rel = _rel_err(grad[s], w['grad'])
        g = np.sqrt(np.diag(w['G']))
        relf = np.abs(F[s] - w['F']) / (g[:, None] * g[None, :])
        ratio = (np.diag(w['F']) / np.diag(w['G'])).min()
        print('vsini_grad %d spectrum %d chi %.10g truth %.10g; gradient %s largest rel '
              'err %.3g; cond(A) %.3g min F_ii/G_ii %.3g Fisher largest err %.3g'
              % (vsini_grad, s, chi[s].item(), w['chi'], np.array2string(
                  w['grad'], precision=4), rel.max(), w['cond'], ratio, relf.max()))
        assert w['cond'] < 100
        worst_g, worst_f = max(worst_g, float(rel.max())), max(worst_f, float(relf.max()))
    print('vsini_grad %d: gradient %.3g (bound %.3g), Fisher %.3g (bound %.3g)'
          % (vsini_grad, worst_g, REL_ERR_BOUND, worst_f, FISHER_BOUND))
    assert worst_g <= REL_ERR_BOUND and worst_f <= FISHER_BOUND


def test_job_forms_and_vsini_rows(chain):
    """chisq_grad_jobs / chisq_fisher_jobs give the numbers of the batch forms; with
    vsini_grad the first 1 + ndim components are the bits of the call without it and
    build_templates appends the vsini row to unchanged rows (5 tangents on MLP rows)"""
    from rvspecfit_amd import engine, spec_fit
    su = chain
    cfg = dict(su['cfg'], nn_gradient=True)
    opt = dict(npoly=NPOLY)
    dev = su['lib'].device
    vel = torch.tensor(VEL, dtype=torch.float64, device=dev)
    rot = torch.tensor(VSINI, dtype=torch.float64, device=dev)
    idx = torch.arange(S, device=dev)
    c0, g0 = spec_fit.get_chisq_grad(su['batch'], vel, su['P'], rot, options=opt,
                                     config=cfg)
    c1, g1 = spec_fit.get_chisq_grad(su['batch'], vel, su['P'], rot, options=opt,
                                     config=cfg, vsini_grad=True)
    assert torch.equal(c0, c1) and torch.equal(g1[:, :R], g0) and g1[:, R].all()
    cj, gj, stj = spec_fit.chisq_grad_jobs(su['batch'], idx, vel, su['P'], rot, opt, cfg,
                                           vsini_grad=True)
    assert torch.equal(cj, c1) and torch.equal(gj, g1) and not stj.any()
    cf, gf, Ff, stf = spec_fit.chisq_fisher_jobs(su['batch'], idx, vel, su['P'], rot, opt,
                                                 cfg, vsini_grad=True)
    _, _, F = spec_fit.get_chisq_fisher(su['batch'], vel, su['P'], rot, options=opt,
                                        config=cfg, vsini_grad=True)
    assert torch.equal(cf, c1) and torch.equal(gf, g1) and torch.equal(Ff, F)
    k1, o1, t1 = engine.build_templates(su['lib'], su['P'], rot, return_templ=True,
                                        tangents=True, vsini_tangent=True)
    k0, o0, t0 = engine.build_templates(su['lib'], su['P'], rot, return_templ=True,
                                        tangents=True)
    assert t1.shape == (S, R + 1, 333) and k1.shape == (S, R + 1, 333, 4)
    assert torch.equal(t1[:, :R], t0) and torch.equal(k1[:, :R], k0)
    assert torch.isfinite(t1).all() and t1[:, R].any()


def test_chisq_func_grad(chain):
    """vel_fit.chisq_func_grad: get_chisq_grad(vsini_grad=True) in the optimiser's
    column order; a Normal prior on teff adds 2 (p - mu) / sigma^2 to its component"""
    from rvspecfit_amd import spec_fit, vel_fit
    from rvspecfit_amd.spec_inter import getSpecParams
    su = chain
    cfg = dict(su['cfg'], nn_gradient=True)
    names = list(getSpecParams(NAME, cfg))
    par = [float(_) for _ in su['par'][0]]
    vel, vs = VEL[0], VSINI[0]

    def func_args(priors=None, config=cfg):
        mapper = vel_fit.ParamMapper(names, dict(zip(names, par)), [],
                                     vel_fit.VSiniMapper(cfg['max_vsini']),
                                     fitVsini=True)
        return dict(specdata=su['sds'][0], paramMapper=mapper, options=dict(npoly=NPOLY),
                    config=config, priors=priors, min_vel=cfg['min_vel'],
                    max_vel=cfg['max_vel'])
    args = func_args()
    p = np.array([vel, vs] + par)
    f, g = vel_fit.chisq_func_grad(p, args)
    ref = vel_fit.chisq_func(p, args)
    assert abs(f - ref) < 1e-11 * max(abs(ref), 1e3), (f, ref)
    _, gp = spec_fit.get_chisq_grad(su['sds'][0], vel, par, (vs, ), options=args['options'],
                                    config=cfg, vsini_grad=True)
    assert args['paramMapper'].get_fitted_params() == ['vel', 'vsini'] + names
    assert (g == gp[[0, 5, 1, 2, 3, 4]]).all() and g.all()
    mu, sig = 5800.0, 150.0
    f1, g1 = vel_fit.chisq_func_grad(p, func_args(priors={'teff': (mu, sig)}))
    it = names.index('teff')
    d = g1 - g
    assert d[2 + it] == pytest.approx(2 * (par[it] - mu) / sig**2, rel=1e-9)
    d[2 + it] = 0
    assert not d.any()
    # 5. without the key: today's refusal
    with pytest.raises(ValueError, match='regular-grid'):
        vel_fit.chisq_func_grad(p, func_args(config=su['cfg']))


# ---- 5. opt-in --------------------------------------------------------------------------
def test_without_the_key_the_calls_are_refused(chain):
    from rvspecfit_amd import optimizer, spec_fit, vel_fit
    su = chain
    dev = su['lib'].device
    vel = torch.tensor(VEL, dtype=torch.float64, device=dev)
    rot = torch.tensor(VSINI, dtype=torch.float64, device=dev)
    idx = torch.arange(S, device=dev)
    opt = dict(npoly=NPOLY)
    for cfg in (su['cfg'], dict(su['cfg'], nn_gradient=False)):
        for f in (spec_fit.get_chisq_grad, spec_fit.get_chisq_fisher):
            for vg in (False, True):
                with pytest.raises(ValueError, match='regular-grid'):
                    f(su['batch'], vel, su['P'], rot, options=opt, config=cfg,
                      vsini_grad=vg)
        for f in (spec_fit.chisq_grad_jobs, spec_fit.chisq_fisher_jobs):
            with pytest.raises(ValueError, match='regular-grid'):
                f(su['batch'], idx, vel, su['P'], rot, opt, cfg)
        with pytest.raises(ValueError, match='regular-grid'):
            vel_fit.fisher_uncertainties(su['batch'], vel, su['P'], rot, options=opt,
                                         config=cfg)
        pd0 = _pd0(su, S)
        with pytest.raises(ValueError, match='nn library'):
            vel_fit.process(su['batch'], pd0, options=opt,
                            config=dict(cfg, second_minimizer=True,
                                        second_minimizer_jac=True))
        pobj, _ = _objective(su, S, cfg)
        with pytest.raises(ValueError, match='regular-grid'):
            optimizer.GradChain(pobj)


# ---- 6. the BFGS polish -----------------------------------------------------------------
def _pd0(su, n):
    pd0 = {k: su['par'][:n, i].copy() for i, k in
           enumerate(['teff', 'logg', 'feh', 'alpha'])}
    pd0['vsini'] = np.full(n, 300.0)
    return pd0


def _objective(su, n, cfg):
    from rvspecfit_amd import optimizer, spec_inter
    batch = su['batch'].subset(torch.arange(n, device=su['lib'].device))
    names = list(spec_inter.getSpecParams(NAME, cfg))
    libs = spec_inter.get_libs(batch.names, cfg)
    dev = batch.device
    pdt = {k: torch.as_tensor(v, dtype=torch.float64).to(dev)
           for k, v in _pd0(su, n).items()}
    safe = torch.stack([pdt[k] for k in names], dim=1).contiguous()
    pobj = optimizer.ProcessObjective(batch, libs, names, pdt, [], True, cfg,
                                      dict(npoly=NPOLY), None, safe)
    return pobj, names


def test_run_grad_equals_the_host_machine(chain):
    """rvs_bfgs_run_grad (the MLP branch of the chain in C) against
    bfgs.minimize_lockstep_native(jac=True) around GradChain.rows (the same entry
    points driven from Python), two spectra, vsini fitted: the criteria of
    test_bfgs_jac_gpu.py::_compare -- equal counters, then equal bits"""
    from rvspecfit_amd import bfgs, optimizer, vel_fit
    su = chain
    n = 2
    cfg = dict(su['cfg'], nn_gradient=True)
    pobj, names = _objective(su, n, cfg)
    chain_ = optimizer.GradChain(pobj)
    cols = ['vel', 'vsini'] + names
    x0 = np.column_stack([VEL[:n], [300.0] * n, su['par'][:n]])
    x0[:, 0] += 4.0
    H0 = vel_fit.get_hess_inv(cols)
    xt = torch.as_tensor(x0).to(su['lib'].device)
    dev_r = bfgs.minimize_lockstep_device(pobj, xt, hess_inv0=H0, jac=True, chain=chain_)
    host = bfgs.minimize_lockstep_native(chain_.rows, x0, hess_inv0=H0, jac=True)
    d = {k: dev_r[k].cpu().numpy() for k in ('x', 'fun', 'nit', 'nfev', 'njev', 'status')}
    print('device nit', d['nit'], 'nfev', d['nfev'], 'njev', d['njev'], 'status',
          d['status'], 'fun', d['fun'])
    print('host   nit', host['nit'], 'nfev', host['nfev'], 'njev', host['njev'],
          'status', host['status'], 'fun', host['fun'])
    for k in ('nit', 'nfev', 'njev', 'status'):
        assert np.array_equal(d[k], host[k]), k
    assert np.array_equal(d['x'], host['x']) and np.array_equal(d['fun'], host['fun'])
    assert (d['njev'] > 0).all() and (d['nit'] > 0).all()
    f0 = chain_.rows(np.arange(n), x0)[:, 0]
    assert (d['fun'] <= f0).all()


def test_process_with_the_polish_and_fisher_uncertainties(chain):
    """vel_fit.process on two noisy spectra against the MLP library with
    second_minimizer_jac, fisher_uncertainties and nn_gradient, vsini fitted"""
    from rvspecfit_amd import vel_fit
    su = chain
    n = 2
    batch = su['batch'].subset(torch.arange(n, device=su['lib'].device))
    cfg = dict(su['cfg'], nn_gradient=True, second_minimizer=True,
               second_minimizer_jac=True, fisher_uncertainties=True)
    r = vel_fit.process(batch, _pd0(su, n), options=dict(npoly=NPOLY), config=cfg)
    print('bfgs', r['bfgs'], 'vel', r['vel'], 'vel_err', r['vel_err'], 'vsini', r['vsini'])
    assert r['bfgs']['jac'] is True and (np.asarray(r['bfgs']['njev']) > 0).all()
    for k in ('vel', 'vel_err', 'chisq', 'vsini'):
        assert torch.isfinite(r[k]).all(), k
    assert (r['vel_err'] > 0).all()
    assert (r['vel'].cpu() - torch.tensor(VEL[:n])).abs().max().item() < 30.0


# ---- 7. refused shapes ------------------------------------------------------------------
def _c_call(lib, P):
    """rvs_template_nn_grad itself on the library's own device arrays and buffers of
    the full size: were the argument check to let a shape through, the launches would
    stay inside them"""
    import ctypes
    from rvspecfit_amd import _lib
    B, Rr = P.shape[0], 1 + lib.ndim
    nl = len(lib.nn_W)
    Wp = (ctypes.c_void_p * nl)(*[w.data_ptr() for w in lib.nn_W])
    bp = (ctypes.c_void_p * nl)(*[b.data_ptr() for b in lib.nn_b])
    a0 = torch.zeros((B * Rr, 256), dtype=torch.float32, device='cuda')
    a1 = torch.zeros_like(a0)
    templ = torch.zeros((B, Rr, lib.ntp), dtype=torch.float64, device='cuda')
    rc = _lib.lib().rvs_template_nn_grad(
        _lib.ptr(P), B, lib.ndim, lib.log_mask, _lib.ptr(lib.nn_M), _lib.ptr(lib.nn_S),
        nl, ctypes.cast(Wp, ctypes.c_void_p), ctypes.cast(bp, ctypes.c_void_p),
        _lib.ptr(lib.nn_dims), _lib.ptr(a0), _lib.ptr(a1), _lib.ptr(templ), _lib.stream())
    torch.cuda.synchronize()
    assert not templ.any()           # nothing was launched
    return rc


def test_refused_shapes(nets):
    """a hidden width of 48 and ndim = 7: RVS_E_ARG from C, a ValueError that names the
    network from eval_batch_grad -- before any launch (nothing is allocated for them)"""
    from rvspecfit_amd.library import TemplateLibrary
    rng = np.random.default_rng(8)

    def net(dims):
        W = [(rng.standard_normal((dims[i + 1], dims[i])) / np.sqrt(dims[i]))
             .astype(np.float32) for i in range(len(dims) - 1)]
        return dict(W=W, b=[np.zeros(w.shape[0], dtype=np.float32) for w in W],
                    M=np.zeros(dims[0]), S=np.ones(dims[0]),
                    dims=np.array(dims, dtype=np.int32), pts=None)
    for dims, word in (([4, 64, 48, 64, 40, 333], 'multiple of 32'),
                       ([7, 64, 64, 40, 333], 'ndim = 7')):
        lib = TemplateLibrary('odd', nt.lib_dict(net(dims), LAM, hull=False))
        P = torch.full((3, dims[0]), 0.5, dtype=torch.float64, device='cuda')
        assert _c_call(lib, P) == -1
        t, _ = lib.eval_batch(P)              # the value path takes them
        assert torch.isfinite(t).all()
        with pytest.raises(ValueError, match=word):
            lib.eval_batch_grad(P)
