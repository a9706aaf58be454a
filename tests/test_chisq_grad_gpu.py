"""rvs_template_polylinear_grad / rvs_chisq_point_grad and the interfaces above them
against tests/chisq_grad_truth.py (float64 torch + autograd on the CPU, itself pinned
to the oracle by test_chisq_grad_cpu.py): J = 7 jobs over 3 spectra on the two golden
arms, at npoly 5, 10 and 16."""
import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG, gold_lib_dict
from oracle import rvs_oracle as orc

import chisq_grad_truth as truth

pytestmark = pytest.mark.gpu
NPOLY = [5, 10, 16]
J = len(truth.JOBS)
# job -> template row: the templates are built in another order than the jobs
TEMPL_OF_JOB = [3, 0, 6, 1, 5, 2, 4]

# Largest error of the analytic gradient against the truth seen on an MI355X, over the
# in-cell jobs and npoly 5 / 10 / 16, relative to max(|g_k|, 1e-6 max_k |g_k|):
#   3.3e-13 (npoly 5), 5.8e-13 (npoly 10), 3.6e-13 (npoly 16)    
# -- the truth's own float64 rounding is of that order.  The bound is 10 x the largest:
# the kernel sums in a fixed order, the factor covers another machine's exp / log /
# sqrt code and the host BLAS under the truth.
MEASURED_REL_ERR = 5.84e-13
REL_ERR_BOUND = 10 * MEASURED_REL_ERR


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
    par = torch.tensor([j[2] for j in truth.JOBS], **f64)
    vs = torch.tensor([j[3] or 0.0 for j in truth.JOBS], **f64)
    return dict(cfg=cfg, sds=sds, batch=batch, libs=libs, dev=dev,
                idx=torch.tensor([j[0] for j in truth.JOBS], device=dev),
                vel=torch.tensor([j[1] for j in truth.JOBS], **f64), par=par, vs=vs)


@pytest.fixture(scope='module')
def olibs():
    return {n: orc.Library(gold_lib_dict(n)) for n in ('gold_b', 'gold_r')}


def _engine_call(su, npoly, order=None):
    """engine.chisq_point_grad and engine.chisq_point on JOBS, templates built in the
    order TEMPL_OF_JOB gives (job -> spectrum and job -> template indirection)"""
    from rvspecfit_amd import engine
    order = list(range(J)) if order is None else order
    trow = torch.tensor(TEMPL_OF_JOB, device=su['dev'])
    inv = torch.argsort(trow)             # template row -> job
    b, libs = su['batch'], su['libs']
    cg, c0, og = [], [], []
    for arm in b.arms:
        c, o = engine.build_templates(libs[arm.name], su['par'][inv], su['vs'][inv],
                                      tangents=True)
        cg.append(c)
        og.append(o)
        c0.append(engine.build_templates(libs[arm.name], su['par'][inv],
                                         su['vs'][inv])[0])
    sel = torch.tensor(order, device=su['dev'])
    js = su['idx'][sel].to(torch.int32).contiguous()
    jt = trow[sel].to(torch.int32).contiguous()
    vel = su['vel'][sel].contiguous()
    chi, grad, st = engine.chisq_point_grad(b, libs, cg, og, vel, npoly, True, js, jt,
                                            0.0, True)
    ref, rst = engine.chisq_point(b, libs, c0, og, vel, npoly=npoly, rbf=True,
                                  job_spec=js, job_templ=jt)
    return chi, grad, st, ref, rst


@pytest.mark.parametrize('npoly', NPOLY)
def test_values_are_chisq_points(cases, setup, npoly):
    """the value beside the gradient == engine.chisq_point on the same jobs, to the
    1e-11 * max(|value|, 1e3) of test_gpu_parity.py::test_objective_fused (the
    orthonormal basis and the order of the sums differ, the quantity does not)"""
    chi, grad, st, ref, rst = _engine_call(setup, npoly)
    assert torch.equal(st, rst)
    assert grad.shape == (J, 5)
    for j in range(J):
        a, b = chi[j].item(), ref[j].item()
        print('npoly %d job %d value %.12g chisq_point %.12g' % (npoly, j, a, b))
        assert abs(a - b) < 1e-11 * max(abs(b), 1e3), (j, a, b)


def test_template_kernel(setup, olibs):
    """rvs_template_polylinear_grad: template row, outside flag and cellinfo are the
    bits of rvs_template_polylinear; the tangent rows are the truth's dt/dp inside a
    cell and exactly zero outside the grid and on a cell with a missing vertex"""
    par = torch.cat([setup['par'], torch.tensor([truth.HOLE_PARAM], dtype=torch.float64,
                                                device=setup['dev'])])
    for name, lib in setup['libs'].items():
        t0, o0, c0, w0 = lib.eval_batch(par, details=True)
        tg, og, cg, wg = lib.eval_batch_grad(par, details=True)
        assert tg.shape == (J + 1, 5, lib.ntp)
        assert torch.equal(tg[:, 0], t0) and torch.equal(cg, c0)
        assert torch.equal(wg, w0)
        assert torch.equal(og.isnan(), o0.isnan())
        assert torch.equal(og.nan_to_num(-1.0), o0.nan_to_num(-1.0))
        mode = cg[:, 0].cpu().numpy()
        assert list(mode) == [0, 0, 0, 0, 0, 1, 2, 1]
        tg = tg.cpu().numpy()
        for j in range(J + 1):
            if mode[j] != 0:
                assert not tg[j, 1:].any(), (name, j)
                continue
            t, jac = truth.template_jacobian(olibs[name], par[j].cpu().numpy())
            # float64 sums of 16 float32 rows: the log-flux rows (|L| <~ 40) differ by
            # O(0.01-1) between vertices, so sum_v dw_v L_v loses <~ 4 digits of the
            # 16: 1e-11 of the row's largest entry leaves a decade
            for k in range(4):
                err = np.abs(tg[j, 1 + k] - jac[k]).max()
                print('%s job %d dt/dp_%d max %.3g err %.3g' %
                      (name, j, k, np.abs(jac[k]).max(), err))
                assert err <= 1e-11 * np.abs(jac[k]).max(), (name, j, k)


def _forward_difference(su, npoly):
    """what BFGS differences today: scipy's forward difference, step 1.49e-8 *
    max(|x|, 1), of engine.chisq_point (templates rebuilt at every point)"""
    from rvspecfit_amd import engine
    b, libs = su['batch'], su['libs']
    x = torch.cat([su['vel'][:, None], su['par']], dim=1)           # [J, 5]
    h = 1.4901161193847656e-08 * torch.clamp(x.abs(), min=1.0)
    pts = x[:, None, :].repeat(1, 6, 1)
    for k in range(5):
        pts[:, 1 + k, k] += h[:, k]
    h = pts[:, 1:, :].diagonal(dim1=1, dim2=2) - x                   # as rounded
    pts = pts.reshape(J * 6, 5)
    vs = su['vs'].repeat_interleave(6)
    cf, og = [], []
    for arm in b.arms:
        c, o = engine.build_templates(libs[arm.name], pts[:, 1:].contiguous(), vs)
        cf.append(c)
        og.append(o)
    js = su['idx'].repeat_interleave(6).to(torch.int32).contiguous()
    f, _ = engine.chisq_point(b, libs, cf, og, pts[:, 0].contiguous(), npoly=npoly,
                              rbf=True, job_spec=js)
    f = f.reshape(J, 6)
    return ((f[:, 1:] - f[:, :1]) / h).cpu().numpy()


@pytest.mark.parametrize('npoly', NPOLY)
def test_gradient_against_the_truth(cases, setup, olibs, npoly):
    """in-cell jobs (one broadened; teff is the log-mapped parameter): per component the
    analytic gradient is no further from the truth than the forward difference BFGS
    uses today, and within REL_ERR_BOUND of it relative to max(|g_k|, 1e-6 |g|_inf)"""
    want = truth.truth_jobs(cases, olibs, npoly)
    chi, grad, st, _, _ = _engine_call(setup, npoly)
    grad = grad.cpu().numpy()
    fd = _forward_difference(setup, npoly)
    worst = 0.0
    bad = []
    for j in truth.INSIDE:
        val, g = want[j]
        assert int(st[j].item()) == 0
        assert abs(chi[j].item() - val) <= 1e-7 * abs(val)
        scale = np.maximum(np.abs(g), 1e-6 * np.abs(g).max())
        e_an, e_fd = np.abs(grad[j] - g), np.abs(fd[j] - g)
        for k in range(5):
            print('npoly %d job %d comp %d truth %.12g analytic err %.3g (rel %.3g) '
                  'forward-difference err %.3g' % (npoly, j, k, g[k], e_an[k],
                                                   e_an[k] / scale[k], e_fd[k]))
            if not (e_an[k] <= e_fd[k] and e_an[k] <= REL_ERR_BOUND * scale[k]):
                bad.append((j, k, e_an[k], e_fd[k], e_an[k] / scale[k]))
        worst = max(worst, float((e_an / scale).max()))
    print('npoly %d largest relative error %.3g' % (npoly, worst))
    assert not bad, bad


def test_penalties(cases, setup, olibs):
    """outside the grid: the value of chisq_point, no parameter gradient, the truth's
    velocity gradient; a non-finite outside flag: 1000 * badchi per arm, no gradient"""
    npoly = 10
    want = truth.truth_jobs(cases, olibs, npoly)
    chi, grad, st, ref, _ = _engine_call(setup, npoly)
    grad = grad.cpu().numpy()
    val, g = want[5]
    assert abs(chi[5].item() - ref[5].item()) < 1e-11 * max(abs(ref[5].item()), 1e3)
    assert abs(chi[5].item() - val) <= 1e-7 * abs(val)
    assert not grad[5, 1:].any() and not g[1:].any()
    print('outside job d/dvel %.12g truth %.12g' % (grad[5, 0], g[0]))
    assert abs(grad[5, 0] - g[0]) <= REL_ERR_BOUND * abs(g[0])
    assert chi[6].item() == 2 * 1000.0 * setup['batch'].badchi == want[6][0]
    assert not grad[6].any()


def test_determinism(setup):
    """two calls: the same bits; the jobs permuted: the permuted rows, bit for bit"""
    chi, grad, st, _, _ = _engine_call(setup, 10)
    chi2, grad2, st2, _, _ = _engine_call(setup, 10)
    assert torch.equal(grad, grad2) and torch.equal(chi, chi2)
    perm = [4, 2, 6, 0, 5, 1, 3]
    chi3, grad3, st3, _, _ = _engine_call(setup, 10, perm)
    sel = torch.tensor(perm, device=setup['dev'])
    assert torch.equal(grad3, grad[sel]) and torch.equal(chi3, chi[sel])
    assert torch.equal(st3, st[sel])


def test_public_interface(cases, setup, olibs):
    from rvspecfit_amd import spec_fit, vel_fit
    su = setup
    opt = dict(npoly=10)
    want = truth.truth_jobs(cases, olibs, 10)
    # many points per spectrum
    chi, grad, st = spec_fit.chisq_grad_jobs(su['batch'], su['idx'], su['vel'],
                                             su['par'], su['vs'], opt, su['cfg'])
    ref, _ = spec_fit.chisq_jobs(su['batch'], su['idx'], su['vel'], su['par'],
                                 su['vs'], opt, su['cfg'])
    for j in range(J):
        assert abs(chi[j].item() - ref[j].item()) < 1e-11 * max(abs(ref[j].item()), 1e3)
    for j in truth.INSIDE:
        g = want[j][1]
        scale = np.maximum(np.abs(g), 1e-6 * np.abs(g).max())
        assert (np.abs(grad[j].cpu().numpy() - g) <= REL_ERR_BOUND * scale).all()
    # one spectrum == the batch form (spectra 0, 1, 2 at jobs 0, 1, 2)
    cb, gb = spec_fit.get_chisq_grad(su['batch'], su['vel'][:3], su['par'][:3],
                                     options=opt, config=su['cfg'])
    assert cb.shape == (3, ) and gb.shape == (3, 5)
    for s in range(3):
        _, vel, par, _ = truth.JOBS[s]
        c1, g1 = spec_fit.get_chisq_grad(su['sds'][s], vel, par, options=opt,
                                         config=su['cfg'])
        assert isinstance(c1, float) and g1.shape == (5, )
        assert c1 == cb[s].item() and (g1 == gb[s].cpu().numpy()).all()
        assert c1 == spec_fit.get_chisq(su['sds'][s], vel, par, options=opt,
                                        config=su['cfg']) or \
            abs(c1 - ref[s].item()) < 1e-11 * max(abs(c1), 1e3)
    # broadened: job 3 through rot_params
    _, vel, par, vs = truth.JOBS[3]
    c3, g3 = spec_fit.get_chisq_grad(su['sds'][0], vel, par, (vs, ), options=opt,
                                     config=su['cfg'])
    assert c3 == chi[3].item() and (g3 == grad[3].cpu().numpy()).all()
    # chisq_func0_grad: a Normal prior on teff adds 2 (p - mu) / sigma^2 there only
    from rvspecfit_amd.spec_inter import getSpecParams
    names = list(getSpecParams('gold_b', su['cfg']))

    class PM:
        specParams = names
    args = dict(specdata=su['sds'][0], paramMapper=PM, options=opt, config=su['cfg'],
                priors=None)
    pd = dict(vel=truth.JOBS[0][1], params=list(truth.JOBS[0][2]), rot_params=None)
    f0, gr0 = vel_fit.chisq_func0_grad(pd, args)
    assert f0 == vel_fit.chisq_func0(pd, args) or abs(
        f0 - vel_fit.chisq_func0(pd, args)) < 1e-11 * max(abs(f0), 1e3)
    mu, sig = 5800.0, 150.0
    args['priors'] = {'teff': (mu, sig)}
    f1, gr1 = vel_fit.chisq_func0_grad(pd, args)
    it = names.index('teff')
    d = gr1 - gr0
    assert d[1 + it] == pytest.approx(2 * (pd['params'][it] - mu) / sig**2, rel=1e-9)
    d[1 + it] = 0
    assert not d.any()
    assert f1 - f0 == pytest.approx(((pd['params'][it] - mu) / sig)**2, rel=1e-9)


def test_unsupported_options_raise(cases, setup):
    """what the kernel does not cover is refused by name, not differenced"""
    from rvspecfit_amd import spec_fit, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    su = setup
    _, vel, par, _ = truth.JOBS[0]
    sd = su['sds'][0]
    kw = dict(config=su['cfg'])
    with pytest.raises(ValueError, match='npoly'):
        spec_fit.get_chisq_grad(sd, vel, par, options=dict(npoly=17), **kw)
    with pytest.raises(ValueError, match='fast_interp'):
        spec_fit.get_chisq_grad(sd, vel, par, options=dict(npoly=10),
                                fast_interp=True, **kw)
    rp = {x.name: spec_fit.construct_resol_mat(x.lam, width=0.5) for x in sd}
    with pytest.raises(ValueError, match='resolution'):
        spec_fit.get_chisq_grad(sd, vel, par, options=dict(npoly=10),
                                resol_params=rp, **kw)
    # a grid set: the second spectrum on a wavelength grid of its own
    other = [spec_fit.SpecData(x.name, x.lam[:-3], x.spec[:-3], x.espec[:-3],
                               badmask=x.badmask[:-3]) for x in su['sds'][1]]
    gs = SpecBatch.from_specdata([sd, other])
    with pytest.raises(ValueError, match='grid set'):
        spec_fit.get_chisq_grad(gs, [vel, vel], par, options=dict(npoly=10), **kw)
    # an MLP library (the network of nn_case.npz on the blue arm's wavelengths)
    import os
    from conftest import GOLD
    d = dict(np.load(os.path.join(GOLD, 'nn_case.npz')))
    lam = np.exp(np.linspace(np.log(4350.), np.log(4800.), int(d['dims'][-1])))
    dd = dict(lam=lam, log_step=np.array(True), log_ids=np.array([0]),
              parnames=np.array(['teff', 'logg', 'feh', 'alpha']),
              nn_dims=d['dims'], nn_M=d['M'], nn_S=d['S'], nn_pts=d['pts'])
    for i in range(len(d['dims']) - 1):
        dd['nn_W%d' % i] = d['W%d' % i]
        dd['nn_b%d' % i] = d['b%d' % i]
    spec_inter.register_library(TemplateLibrary('gold_b', dd), 'golden-nn://')
    b1 = SpecBatch.from_specdata([sd[:1]])
    with pytest.raises(ValueError, match='regular-grid'):
        spec_fit.get_chisq_grad(b1, vel, par, options=dict(npoly=10),
                                config=dict(su['cfg'], template_lib='golden-nn://'))
