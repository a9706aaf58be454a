"""Value and gradient on MLP libraries by one adjoint row back through the net (DESIGN
4.25): rvs_objective_grad_from_template, rvs_template_nn_vjp, rvs_objective_grad_join and
the calls that take them with config['fused_gradient'] and config['nn_gradient'] together.

Fixture: that of tests/test_nn_grad_gpu.py (tests/golden/nn_case.npz, 4 -> 64^3 -> 40 ->
333 and its 39-wide cut, three noisy spectra, VEL, VSINI, points off the optimum) with 129
pixels on 4000-5000 A, so that 2 npix <= 333 holds.

Paths of rvs_template_nn_vjp (csrc/nn.hip): the last layer's transposed product takes 32
jobs per block and the 333 pixels in two runs (256 + 77: a full run and a partial one in
every call); the hidden stack's reverse pass takes 16 jobs per block.  B = 1, 7, 27 leave
tails in both; ROWS16_B = 17 is the first batch with a second block of the hidden stack,
ROWS32_B = 33 the first with a second row tile of the last layer.

MI355X figures: see the docstrings of the tests."""
import numpy as np
import pytest
import torch

import nn_grad_truth as nt
import nn_vjp_truth as vt
import objective_grad_shapes as shapes
from test_nn_vjp_cpu import LAM, VEL, _cut39, adjoint_rows, fixture_spectra
from test_chisq_grad_gpu import REL_ERR_BOUND as CHAIN_BOUND
from test_objective_grad_gpu import REL_ERR_BOUND as FUSED_BOUND

pytestmark = pytest.mark.gpu
ND = nt.NDIM
ROWS16_B = 17         # 16 jobs per block of nn_vjp_hidden_kernel
ROWS32_B = 33         # 32 jobs per block of nn_vjp_last_kernel
URL = 'golden-nn-vjp://'
NAME = 'aat_580v'
S = 3
VSINI = [380.0, 250.0, 520.0]
# measured on an MI355X, times ten (the rule of DESIGN 4.21); see the tests' docstrings
TWIN_CONTRACTION_BOUND = 10 * 5.35e-15
TBAR_BOUND = 10 * 1.94e-13
VALUE_BOUND = 10 * 1.77e-15


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


@pytest.fixture(scope='module')
def chain(nets, libs):
    from conftest import GOLD_CONFIG
    from rvspecfit_amd import spec_inter, spec_fit
    from rvspecfit_amd.engine import SpecBatch
    net, lib = nets['k40'], libs['k40']
    spec_inter.register_library(lib, URL)
    cfg = dict(GOLD_CONFIG, template_lib=URL, max_vsini=600, nn_gradient=True)
    sp = fixture_spectra(net)
    sds = [[spec_fit.SpecData(NAME, w, d, e)] for w, d, e in sp]
    par = nt.points(net, S, seed=6, shrink=0.1)
    dev = lib.device
    return dict(cfg=cfg, both=dict(cfg, fused_gradient=True), sds=sds, sp=sp,
                batch=SpecBatch.from_specdata(sds), lib=lib, par=par,
                P=torch.as_tensor(par).to(dev),
                vel=torch.tensor(VEL, dtype=torch.float64, device=dev),
                rot=torch.tensor(VSINI, dtype=torch.float64, device=dev))


# ---- 1. the kernel against its regular-grid twin --------------------------------------------
TWINS = ['chunk-cut32', 'chunk-cut263', 'pack-cut64-32', 'pack-cut32-kmax13', 'nd2-vsini',
         'mixed-cut32-fine6485', 'prod-lds-limit']


@pytest.mark.parametrize('name', TWINS)
def test_kernel_against_its_regular_grid_twin(name):
    """rvs_objective_grad_from_template on the rows rvs_template_polylinear writes for the
    same jobs, against rvs_objective_grad: 32 knots and the largest ntp the geometry admits
    (6485), copy branch and fixed vsini (the chunk cases: two jobs each), fitted vsini (the
    others), two arms of different length, a job list permuted.  Status equal; value,
    velocity and vsini components within 1e-11 max(|x|, 1e3) / 1e-11 |g|_inf, the bound
    tests/test_gpu_parity.py::test_objective_from_template holds the value kernel's two
    forms to (it states no bit equality) -- and, as measured, the same bits in all seven
    cases: the rows of rvs_template_polylinear are the bits of the kernel's own gather, and
    everything behind the row is one text.  tbar contracted on the host in float64 with the
    tangent rows of rvs_template_polylinear_grad against the parameter components of
    rvs_objective_grad, relative to max(|g_k|, 1e-6 |g|_inf).

    MI355X: chunk-cut32 1.31e-15, chunk-cut263 1.1e-15, pack-cut64-32 9.69e-16,
    pack-cut32-kmax13 5.94e-16, nd2-vsini 1.89e-15, mixed-cut32-fine6485 5.35e-15,
    prod-lds-limit 2.56e-15; the bound is ten times the largest."""
    import test_objective_grad_shapes_gpu as tg
    from rvspecfit_amd import engine
    c = shapes.case(name)
    d = tg._device(c)
    order = [2, 0, 3, 1] if len(c.jobs) == 4 else None
    chi, grad, st = tg._fused(c, d, order)
    sel = torch.arange(len(c.jobs), device=d['vel'].device) if order is None else \
        torch.tensor(order, device=d['vel'].device)
    par = d['par'][sel].contiguous()
    vs = None if d['vs'] is None else d['vs'][sel].contiguous()
    ls = [d['libs'][arm.name] for arm in d['batch'].arms]
    rows = [lib.eval_batch_grad(par) for lib in ls]
    o, gvv, st2, tbars, _ = engine.objective_grad_from_template(
        d['batch'], d['libs'], [r[0][:, 0].contiguous() for r in rows],
        [r[1] for r in rows], vs, d['vel'][sel].contiguous(), c.npoly, c.rbf,
        d['idx'][sel].contiguous(), c.vsini_grad)
    nd = c.ndim
    assert gvv.shape == (len(c.jobs), 1 + int(c.vsini_grad))
    assert torch.equal(st, st2)
    cols = [0] + ([1 + nd] if c.vsini_grad else [])
    g0 = grad[:, cols]
    bits = torch.equal(o, chi) and torch.equal(gvv, g0)
    ev = ((o - chi).abs() / chi.abs().clamp(min=1e3)).max().item()
    eg = ((gvv - g0).abs() / grad.abs().max(dim=1, keepdim=True)[0]).max().item()
    host = sum(torch.einsum('jn,jkn->jk', tb, r[0][:, 1:]) for tb, r in zip(tbars, rows))
    ec = shapes.rel_err(host.cpu().numpy(), grad[:, 1:1 + nd].cpu().numpy()).max()
    print('%s: value, d/dvel%s the same bits: %s (largest differences %.3g, %.3g); tbar '
          'contracted on the host against the kernel\'s parameter components %.3g'
          % (name, ', d/dvsini' if c.vsini_grad else '', bits, ev, eg, ec))
    assert ev <= 1e-11 and eg <= 1e-11
    assert bits
    assert ec <= TWIN_CONTRACTION_BOUND


def test_skipped_arm_and_outside_flag(chain):
    """an outside flag of NaN: the arm is skipped -- 1000 badchi on the value, a zero
    gradient, a tbar row of zeros; a finite positive flag: flag x badchi on the value, the
    gradient and tbar the bits of the job inside"""
    from rvspecfit_amd import engine
    su = chain
    t, out = su['lib'].eval_batch(su['P'])
    assert not out.any()
    call = lambda o: engine.objective_grad_from_template(      # noqa: E731
        su['batch'], {NAME: su['lib']}, [t], [o], su['rot'], su['vel'], 5, True, None,
        True)
    c0, g0, s0, tb0, _ = call(out)
    o2 = out.clone()
    o2[0], o2[2] = float('nan'), 0.25
    c1, g1, s1, tb1, _ = call(o2)
    bad = float(su['batch'].badchi)
    assert c1[0].item() == 1000.0 * bad and not g1[0].any() and not tb1[0][0].any()
    assert torch.equal(g1[1:], g0[1:]) and torch.equal(tb1[0][1:], tb0[0][1:])
    assert c1[1].item() == c0[1].item()
    assert abs(c1[2].item() - (c0[2].item() + 0.25 * bad)) <= 1e-12 * abs(c1[2].item())
    assert torch.equal(s0, s1)


# ---- 2. tbar against the truth ------------------------------------------------------------
@pytest.mark.parametrize('npoly', [5, 10])
@pytest.mark.parametrize('rot', [False, True])
def test_tbar_against_the_truth(chain, npoly, rot):
    """the adjoint row of the kernel at the device's own template rows against float64
    autograd with the row as the leaf (template_adjoint_truth), relative to |tbar|_inf;
    value to 1e-7; the velocity component to the fused kernel's bound
    (tests/test_objective_grad_gpu.py) relative to max(|g_vel|, 1e-6 |g|_inf), the
    parameter components of g from the truth's tbar and the device's tangent rows;
    cond(A) < 100.

    MI355X, largest tbar error of the three spectra: npoly 5 1.94e-13, npoly 10 1.91e-13;
    with the fixed vsini 9.72e-14 and 9.39e-14 (|tbar|_inf 360 ... 560); the bound is ten
    times the largest."""
    from rvspecfit_amd import engine
    su = chain
    rows, out = su['lib'].eval_batch_grad(su['P'])
    t, tan = rows[:, 0].contiguous(), rows[:, 1:].cpu().numpy()
    chi, gvv, st, tbars, _ = engine.objective_grad_from_template(
        su['batch'], {NAME: su['lib']}, [t], [out], su['rot'] if rot else None, su['vel'],
        npoly, True, None, False)
    assert not st.any()
    th, tb = t.cpu().numpy(), tbars[0].cpu().numpy()
    worst = 0.0
    for s in range(S):
        w, d, e = su['sp'][s]
        c, gv, want, cond = vt.template_adjoint_truth(w, d, e, LAM, th[s], VEL[s],
                                                      VSINI[s] if rot else None, npoly)
        assert cond < 100
        err = np.abs(tb[s] - want).max() / np.abs(want).max()
        worst = max(worst, err)
        print('npoly %d rot %d spectrum %d: chi %.10g truth %.10g, d/dvel %.6g truth %.6g,'
              ' tbar error %.3g of |tbar|_inf = %.3g'
              % (npoly, rot, s, chi[s].item(), c, gvv[s, 0].item(), gv, err,
                 np.abs(want).max()))
        assert abs(chi[s].item() - c) <= 1e-7 * abs(c)
        ginf = max(abs(gv), np.abs(tan[s] @ want).max())
        assert abs(gvv[s, 0].item() - gv) <= FUSED_BOUND * max(abs(gv), 1e-6 * ginf)
    assert worst <= TBAR_BOUND


# ---- 3. the network's reverse pass ------------------------------------------------------------
_inputs = {}


def _vjp_inputs(nets, libs, which, B):
    """(points, tbar rows, vjp64, its scale, reverse32's largest metric) -- once"""
    if (which, B) not in _inputs:
        net = nets[which]
        p = nt.points(net, B, seed=B, shrink=0.1)
        _, tbar = adjoint_rows(net, p)
        want, scale = vt.vjp64(net, p, tbar)
        r32 = vt.reverse32(net, p, nt.forward32(net, p)[0], tbar)
        _inputs[which, B] = (p, tbar, want, scale, vt.vjp_metric(r32, want, scale).max())
    return _inputs[which, B]


@pytest.mark.parametrize('which,B', [('k40', 1), ('k40', 7), ('k40', 27),
                                     ('k40', ROWS16_B), ('k40', ROWS32_B), ('k39', 7),
                                     ('k39', ROWS32_B)])
def test_vjp_against_the_truth(nets, libs, which, B):
    """against vjp64 in the metric |got - want| / sum_n |tbar_n jac64[k, n]| within 4 x the
    largest figure of the float32 CPU statement at the same points; and against the host's
    float64 contraction of tbar with rows 1 ... of rvs_template_nn_grad within the sum of
    the two float32 bounds: 4 x reverse32's figure plus 4 x forward32's tangent metric
    (relative to max_n |jac_k|) carried into this metric by sum |tbar| max |jac_k| /
    sum |tbar jac_k| (>= 1).

    MI355X (device against vjp64 / float32 CPU statement; against the forward-mode rows):
      k40: B 1 6.63e-08 / 8.95e-08; 1.24e-07   B 7 9.75e-08 / 1.49e-07; 2.17e-07
           B 27 1.76e-07 / 2.02e-07; 1.34e-07  B 17 1.36e-07 / 2.62e-07; 1.96e-07
           B 33 1.62e-07 / 1.94e-07; 2.32e-07
      k39: B 7 2.65e-07 / 2.24e-07; 2.60e-07   B 33 2.11e-07 / 2.05e-07; 2.38e-07"""
    lib, net = libs[which], nets[which]
    p, tbar, want, scale, m32 = _vjp_inputs(nets, libs, which, B)
    P = torch.as_tensor(p).to(lib.device)
    TB = torch.as_tensor(tbar).to(lib.device)
    rows, out = lib.eval_batch_grad(P)
    assert not out.any()
    got = lib.nn_vjp(P, rows[:, 0].contiguous(), TB)
    assert got.shape == (B, ND) and torch.isfinite(got).all()
    g = got.cpu().numpy()
    m = vt.vjp_metric(g, want, scale)
    host = torch.einsum('jn,jkn->jk', TB, rows[:, 1:]).cpu().numpy()
    _, jac = nt.jacobian64(net, p)
    fwd = nt.tangent_metric(nt.forward32(net, p)[1], jac).max()
    carry = (np.abs(tbar).sum(axis=1)[:, None] * np.abs(jac).max(axis=2)) / scale
    mh = vt.vjp_metric(g, host, scale)
    print('%s B %d: against vjp64 %.3g (job %d), float32 CPU statement %.3g, bound %.3g; '
          'against the forward-mode rows %.3g (bound %.3g at that job)'
          % (which, B, m.max(), int(m.max(axis=1).argmax()), m32, 4 * m32, mh.max(),
             (4 * m32 + 4 * fwd * carry).flat[mh.argmax()]))
    assert (m <= 4 * m32).all()
    assert (mh <= 4 * m32 + 4 * fwd * carry).all()


def test_vjp_exact_properties(nets, libs):
    """two calls: the same bits; a job alone: the bits it has inside the batch of 27;
    tbar scaled by 2^+-100: results scaled by exactly that power; a zero tbar row:
    exactly 0; a non-finite mapped parameter: NaN in all components of that job and
    nothing else"""
    lib = libs['k40']
    p, tbar, _, _, _ = _vjp_inputs(nets, libs, 'k40', 27)
    P = torch.as_tensor(p).to(lib.device)
    TB = torch.as_tensor(tbar).to(lib.device)
    t, _ = lib.eval_batch(P)
    a = lib.nn_vjp(P, t, TB)
    assert torch.equal(a, lib.nn_vjp(P, t, TB))
    for j in (0, 5, 15, 16, 26):
        one = lib.nn_vjp(P[j:j + 1], t[j:j + 1], TB[j:j + 1])
        assert torch.equal(one[0], a[j]), j
    for k in (100, -100):
        assert torch.equal(lib.nn_vjp(P, t, torch.ldexp(TB, torch.tensor(k))),
                           torch.ldexp(a, torch.tensor(k))), k
    z = TB.clone()
    z[4] = 0.0
    az = lib.nn_vjp(P, t, z)
    assert not az[4].any() and torch.equal(az[[0, 3, 5, 26]], a[[0, 3, 5, 26]])
    assert az[4].abs().sum().item() == 0.0 and not torch.signbit(az[4]).any()
    p2 = p.copy()
    p2[3, 1] = np.nan
    p2[11, 0] = -5.0
    P2 = torch.as_tensor(p2).to(lib.device)
    b = lib.nn_vjp(P2, t, TB)
    bad = torch.zeros(27, dtype=torch.bool, device=lib.device)
    bad[[3, 11]] = True
    assert b[bad].isnan().all() and torch.equal(b[~bad], a[~bad])


def test_vjp_clip_is_flat(nets):
    """a last-layer bias of 400 / -400: the template is exp(+-300) there and the pixel
    contributes exactly nothing -- the result is the bits of the call with tbar zeroed at
    those pixels, and differs from the unchanged network's"""
    from rvspecfit_amd.library import TemplateLibrary
    net = nets['k40']
    hot = dict(net, b=[b.copy() for b in net['b']])
    hot['b'][-1][5], hot['b'][-1][200] = 400.0, -400.0
    hlib = TemplateLibrary(NAME, nt.lib_dict(hot, LAM))
    p = nt.points(net, 7, seed=2)
    P = torch.as_tensor(p).to(hlib.device)
    t, _ = hlib.eval_batch(P)
    assert (t[:, 5] / np.exp(300.0) - 1).abs().max().item() < 1e-14
    assert (t[:, 200] / np.exp(-300.0) - 1).abs().max().item() < 1e-14
    rng = np.random.default_rng(3)
    TB = torch.as_tensor(rng.standard_normal((7, 333))).to(hlib.device)
    TB[:, 5] = 1e-120            # (times exp(300): the row's largest entry, were it kept)
    a = hlib.nn_vjp(P, t, TB)
    z = TB.clone()
    z[:, [5, 200]] = 0.0
    assert torch.equal(a, hlib.nn_vjp(P, t, z))
    assert torch.isfinite(a).all() and a.all()


# ---- 4. end to end ----------------------------------------------------------------------------
def _rel_err(got, g):
    return np.abs(got - g) / np.maximum(np.abs(g), 1e-6 * np.abs(g).max())


def _param_bound(su, npoly, rot, nets, par=None, vel=None, idx=None):
    """per (job, k): what the forward-mode and the reverse-mode float32 bounds allow
    between the two paths' parameter components: (4 x reverse32's figure + 4 x forward32's
    tangent metric carried into it) x sum_n |tbar_n jac_kn|, from the device's own rows;
    par [J, ndim] (numpy), vel, idx: the jobs (default: the fixture's three spectra)"""
    from rvspecfit_amd import engine
    net = nets['k40']
    par = su['par'] if par is None else par
    vel = su['vel'] if vel is None else vel
    P = torch.as_tensor(par).to(su['lib'].device)
    rows, out = su['lib'].eval_batch_grad(P)
    _, _, _, tbars, _ = engine.objective_grad_from_template(
        su['batch'], {NAME: su['lib']}, [rows[:, 0].contiguous()], [out], rot, vel,
        npoly, True, idx, False)
    tb, jac = tbars[0].cpu().numpy(), rows[:, 1:].cpu().numpy()
    scale = np.abs(tb[:, None, :] * jac).sum(axis=2)
    j64 = nt.jacobian64(net, par)[1]
    fwd = nt.tangent_metric(nt.forward32(net, par)[1], j64).max()
    want, sc64 = vt.vjp64(net, par, tb)
    r32 = vt.reverse32(net, par, nt.forward32(net, par)[0], tb)
    m32 = vt.vjp_metric(r32, want, sc64).max()
    carry = np.abs(tb).sum(axis=1)[:, None] * np.abs(jac).max(axis=2)
    return 4 * m32 * scale + 4 * fwd * carry


def _gradient_within_bounds(g1, g0, pb, what):
    """g1 (both keys) against g0 (nn_gradient alone), [J, 1 + ndim (+ 1)] numpy, in
    _rel_err's metric: velocity and vsini components within the sum of the chain's and the
    fused kernel's float64 bounds, the parameter components within pb (_param_bound) beside
    it"""
    floor = np.maximum(np.abs(g0), 1e-6 * np.abs(g0).max(axis=1, keepdims=True))
    rel = np.abs(g1 - g0) / floor
    allowed = np.full(g0.shape, CHAIN_BOUND + FUSED_BOUND)
    allowed[:, 1:1 + ND] += pb / floor[:, 1:1 + ND]
    print('%s: gradient, largest rel err vel %.3g, parameters %.3g (allowed there %.3g)%s'
          % (what, rel[:, 0].max(), rel[:, 1:1 + ND].max(),
             allowed[:, 1:1 + ND].flat[rel[:, 1:1 + ND].argmax()],
             ', vsini %.3g' % rel[:, -1].max() if g0.shape[1] > 1 + ND else ''))
    assert (rel <= allowed).all()


@pytest.mark.parametrize('npoly', [5, 10])
def test_get_chisq_grad_both_keys_against_the_chain(chain, nets, npoly):
    """spec_fit.get_chisq_grad with both keys against the same call with nn_gradient alone
    (the forward-mode chain): values within VALUE_BOUND relative (the issue's 1e-7,
    tightened to ten times the 1.77e-15 measured); velocity and vsini components,
    float64 on both sides, within the sum of the chain's and the fused kernel's bounds
    (tests/test_chisq_grad_gpu.py, tests/test_objective_grad_gpu.py) in _rel_err's metric; the
    parameter components within the sum of the forward-mode and reverse-mode float32
    bounds (_param_bound).  With vsini_grad the first 1 + ndim components are the bits of
    the call without it.

    MI355X: values differ by 1.77e-15 (npoly 5) and 9.9e-16 (10); velocity 2.1e-14, vsini
    2.7e-14; parameters 1.0e-05 (allowed at that component 3.1e-03) and 3.2e-06 (allowed
    6.8e-04): the largest figures sit on components far below |g|_inf of their job, where
    the metric's denominator is small and the allowance, an absolute error over the same
    denominator, is large too."""
    from rvspecfit_amd import spec_fit
    su = chain
    opt = dict(npoly=npoly)
    out = {}
    for vg in (False, True):
        for key in ('cfg', 'both'):
            out[key, vg] = spec_fit.get_chisq_grad(su['batch'], su['vel'], su['P'],
                                                   su['rot'], options=opt, config=su[key],
                                                   vsini_grad=vg)
    assert torch.equal(out['both', True][0], out['both', False][0])
    assert torch.equal(out['both', True][1][:, :1 + ND], out['both', False][1])
    pb = _param_bound(su, npoly, su['rot'], nets)
    for vg in (False, True):
        (c1, g1), (c0, g0) = out['both', vg], out['cfg', vg]
        assert g1.shape == g0.shape == (S, 1 + ND + int(vg))
        ev = ((c1 - c0).abs() / c0.abs()).max().item()
        print('npoly %d vsini_grad %d: values differ by %.3g' % (npoly, vg, ev))
        assert ev <= VALUE_BOUND
        _gradient_within_bounds(g1.cpu().numpy(), g0.cpu().numpy(), pb,
                                'npoly %d vsini_grad %d' % (npoly, vg))


def test_chisq_grad_jobs_in_chunks(chain, nets, monkeypatch):
    """spec_fit.chisq_grad_jobs with both keys: seven jobs over the three spectra against
    the chain (values within VALUE_BOUND, status equal, the gradient within the bounds of
    test_get_chisq_grad_both_keys_against_the_chain); under a byte budget of two jobs' rows
    (chunks of 2, 2, 2, 1) and of less than one job's (chunks of one) the bits of one
    call"""
    from rvspecfit_amd import engine, spec_fit
    su = chain
    dev = su['lib'].device
    idx = torch.tensor([0, 1, 2, 2, 1, 0, 1], device=dev)
    P = torch.as_tensor(nt.points(nets['k40'], 7, seed=9, shrink=0.1)).to(dev)
    vel = su['vel'][idx] + torch.arange(7, dtype=torch.float64, device=dev)
    rot = su['rot'][idx]
    opt = dict(npoly=5)
    ref = spec_fit.chisq_grad_jobs(su['batch'], idx, vel, P, rot, opt, su['cfg'],
                                   vsini_grad=True)
    one = spec_fit.chisq_grad_jobs(su['batch'], idx, vel, P, rot, opt, su['both'],
                                   vsini_grad=True)
    assert one[1].shape == (7, 2 + ND) and torch.equal(one[2], ref[2])
    assert ((one[0] - ref[0]).abs() / ref[0].abs()).max().item() <= VALUE_BOUND
    pb = _param_bound(su, 5, rot, nets, par=P.cpu().numpy(), vel=vel, idx=idx)
    _gradient_within_bounds(one[1].cpu().numpy(), ref[1].cpu().numpy(), pb,
                            'chisq_grad_jobs')
    for budget in (2 * (16 * 333 + 4 * 2 * 40), 100):
        monkeypatch.setattr(engine, 'TBAR_BUDGET', budget)
        got = spec_fit.chisq_grad_jobs(su['batch'], idx, vel, P, rot, opt, su['both'],
                                       vsini_grad=True)
        assert all(torch.equal(a, b) for a, b in zip(got, one)), budget


def test_chisq_func_grad_both_keys(chain, nets):
    """vel_fit.chisq_func_grad with both keys: get_chisq_grad(vsini_grad=True) of the same
    configuration in the optimiser's column order, the value chisq_func's; against the call
    with nn_gradient alone the gradient within the bounds of
    test_get_chisq_grad_both_keys_against_the_chain"""
    from rvspecfit_amd import spec_fit, vel_fit
    from rvspecfit_amd.spec_inter import getSpecParams
    su = chain
    cfg = su['both']
    names = list(getSpecParams(NAME, cfg))
    par = [float(_) for _ in su['par'][0]]
    vel, vs = VEL[0], VSINI[0]
    mapper = vel_fit.ParamMapper(names, dict(zip(names, par)), [],
                                 vel_fit.VSiniMapper(cfg['max_vsini']), fitVsini=True)
    args = dict(specdata=su['sds'][0], paramMapper=mapper, options=dict(npoly=5),
                config=cfg, priors=None, min_vel=cfg['min_vel'], max_vel=cfg['max_vel'])
    p = np.array([vel, vs] + par)
    f, g = vel_fit.chisq_func_grad(p, args)
    ref = vel_fit.chisq_func(p, args)
    assert abs(f - ref) < 1e-11 * max(abs(ref), 1e3), (f, ref)
    _, gp = spec_fit.get_chisq_grad(su['sds'][0], vel, par, (vs, ), options=args['options'],
                                    config=cfg, vsini_grad=True)
    assert (g == gp[[0, 5, 1, 2, 3, 4]]).all() and g.all()
    _, gc = vel_fit.chisq_func_grad(p, dict(args, config=su['cfg']))
    # (x = vsini inside (0, max_vsini): the penalty term 2 (x - clamp(x)) is zero, the
    # columns are the physical gradient's)
    pb = _param_bound(su, 5, su['rot'][:1], nets, par=su['par'][:1], vel=su['vel'][:1],
                      idx=torch.zeros(1, dtype=torch.int32, device=su['lib'].device))
    back = [0, 2, 3, 4, 5, 1]
    _gradient_within_bounds(g[back][None], gc[back][None], pb, 'chisq_func_grad')


# ---- 5. the rounds ------------------------------------------------------------------------------
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
    pdt = {k: torch.as_tensor(v, dtype=torch.float64).to(batch.device)
           for k, v in _pd0(su, n).items()}
    safe = torch.stack([pdt[k] for k in names], dim=1).contiguous()
    pobj = optimizer.ProcessObjective(batch, libs, names, pdt, [], True, cfg,
                                      dict(npoly=5), None, safe)
    return pobj, names


def test_run_grad_fused_nn_equals_the_host_machine(chain):
    """rvs_bfgs_run_grad_fused_nn (the sequence of DESIGN 4.25 in C) against
    bfgs.minimize_lockstep_native(jac=True) around GradChain(fused=True).rows (the same
    entry points driven from Python), two spectra, vsini fitted: equal counters, then
    equal bits -- the pattern of tests/test_nn_grad_gpu.py's
    test_run_grad_equals_the_host_machine"""
    from rvspecfit_amd import bfgs, optimizer, vel_fit
    su = chain
    n = 2
    pobj, names = _objective(su, n, su['both'])
    chain_ = optimizer.GradChain(pobj, fused=True)
    assert chain_.fused and chain_.fused_nn
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


def test_process_with_the_fused_polish(chain):
    """vel_fit.process with second_minimizer_jac and both keys runs, through
    rvs_bfgs_run_grad_fused_nn, and ends no higher than the simplex optimum (the same call
    without a second minimiser) on each spectrum -- to 1e-11 max(|chisq|, 1e3), what the
    value kernel's and the gradient kernel's values of one point may differ by"""
    from rvspecfit_amd import vel_fit
    su = chain
    opt = dict(npoly=5)
    r0 = vel_fit.process(su['batch'], _pd0(su, S), options=opt, config=su['both'])
    r = vel_fit.process(su['batch'], _pd0(su, S), options=opt,
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


# ---- 6. what still raises ---------------------------------------------------------------------
def test_refusals_with_both_keys(chain):
    """the Fisher matrix, fast_interp, a resolution matrix, an npoly beyond 10, the
    Levenberg-Marquardt polish and the joint-epoch fit raise with both keys set, naming the
    key; an MLP arm outside the kernel's geometry (1000 pixels on 333 knots) raises naming
    the nn library, from get_chisq_grad, from GradChain(fused=True) and from process"""
    from rvspecfit_amd import optimizer, spec_fit, vel_fit
    from rvspecfit_amd.engine import SpecBatch
    su = chain
    opt = dict(npoly=5)
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*Fisher'):
        spec_fit.get_chisq_fisher(su['batch'], su['vel'], su['P'], su['rot'], options=opt,
                                  config=su['both'])
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*fast_interp'):
        spec_fit.get_chisq_grad(su['batch'], su['vel'], su['P'], su['rot'], options=opt,
                                config=su['both'], fast_interp=True)
    rp = {NAME: spec_fit.construct_resol_mat(su['sp'][0][0], width=0.5)}
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*resolution matrix'):
        spec_fit.get_chisq_grad(su['batch'], su['vel'], su['P'], su['rot'], options=opt,
                                config=su['both'], resol_params=rp)
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*npoly'):
        spec_fit.get_chisq_grad(su['batch'], su['vel'], su['P'], su['rot'],
                                options=dict(npoly=11), config=su['both'])
    pd0 = _pd0(su, S)
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*second_minimizer_lm'):
        vel_fit.process(su['batch'], dict(pd0), options=opt,
                        config=dict(su['both'], second_minimizer=True,
                                    second_minimizer_lm=True))
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*epochs'):
        vel_fit.process_epochs(su['batch'], np.array([0, 0, 0]),
                               {k: v[:1] for k, v in pd0.items()}, np.zeros(S),
                               options=opt, config=su['both'])
    pobj, _ = _objective(su, 2, su['both'])
    with pytest.raises(ValueError, match=r'(?s)fused_gradient.*Fisher'):
        optimizer.GradChain(pobj, fused=True, fisher=True)
    # outside the geometry
    wave = np.linspace(4000., 5000., 1000)
    rng = np.random.RandomState(3)
    wide = [[spec_fit.SpecData(NAME, wave, rng.normal(1, 0.1, 1000), np.full(1000, 0.1))]
            for _ in range(2)]
    wb = SpecBatch.from_specdata(wide)
    pat = r'(?s)fused_gradient.*nn library'
    with pytest.raises(ValueError, match=pat):
        spec_fit.get_chisq_grad(wb, su['vel'][:2], su['P'][:2], su['rot'][:2], options=opt,
                                config=su['both'])
    with pytest.raises(ValueError, match=pat):
        vel_fit.process(wb, _pd0(su, 2), options=opt,
                        config=dict(su['both'], second_minimizer=True,
                                    second_minimizer_jac=True))
