"""rvs_chisq_point_grad_resol / rvs_chisq_point_fisher_resol and the interfaces above
them (config['resol_gradient']) against tests/chisq_grad_resol_truth.py (float64 torch /
numpy on the CPU, itself pinned to the oracle by test_chisq_grad_resol_cpu.py): the J = 7
jobs of chisq_grad_truth.JOBS over 3 spectra on the two golden arms at npoly 5, 10 and 16,
every spectrum under Gaussian resolution matrices of its own (9 ... 25 diagonals on arms
of 401 and 301 pixels: the bands cross pixel 256, the stride of the block's tiles).

Bounds.  Gradient: relative to max(|g_k|, 1e-6 |g|_inf).  Until the first MI355X run the
bound stood at 4 x REL_ERR_BOUND of tests/test_chisq_grad_gpu.py = 2.34e-11 -- a reasoned
factor, not a measured one: the band adds nd <= 25 rounded products per pixel to sums of
hundreds of terms.  For the golden jobs under the spectra's own matrices it is now 10 x the
largest error of that run (MEASURED_GRAD_REL_ERR); the calls with other bands (a matrix on
one arm only, 151 and 939 diagonals), which that figure was not taken from, keep the
reasoned bound (BAND_GRAD_BOUND).  Fisher matrix: relative to sqrt(G_ii G_ll) as in
tests/test_chisq_fisher_gpu.py, whose bound (5.84e-12) stood until the first run; now 10 x
the largest error seen in this file (MEASURED_FISHER_REL_ERR).

Largest errors seen on an MI355X (first device run), DESIGN 4.18:
  gradient, golden jobs  1.35e-13 (npoly 5), 1.18e-13 (npoly 10), 2.33e-13 (npoly 16); the
           vsini component 5.4e-14; a matrix on the blue arm only 3.77e-12 (job 1; the
           other jobs <= 5.2e-13); 151 diagonals 2.16e-13; 939 diagonals 1.7e-12
  Fisher   golden jobs 1.47e-15 / 1.31e-15 / 1.54e-15; a matrix on the blue arm only
           1.75e-15; 151 diagonals 4.5e-16 -- the truth's own float64 rounding
  identity matrix (nd = 1, taps 1): value, gradient and Fisher matrix bit-equal to the
           entry points without a matrix at npoly 5 / 10 / 16
"""
import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG, gold_lib_dict
from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import chisq_grad_resol_truth as rtruth
from test_chisq_grad_gpu import REL_ERR_BOUND
from test_desi_gpu import CFG, COADD, RUNS, dcases, desi_libs  # noqa: F401

pytestmark = pytest.mark.gpu
NPOLY = [5, 10, 16]
J = len(truth.JOBS)
ND = 4
MEASURED_GRAD_REL_ERR = 2.33e-13
MEASURED_FISHER_REL_ERR = 1.75e-15
GRAD_BOUND = 10 * MEASURED_GRAD_REL_ERR
BAND_GRAD_BOUND = 4 * REL_ERR_BOUND
FISHER_BOUND = 10 * MEASURED_FISHER_REL_ERR


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
    cfg = dict(GOLD_CONFIG, template_lib='golden://', resol_gradient=True)
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, gold_lib_dict(n)), 'golden://')
    sds = truth.spectra(cases, spec_fit.SpecData)
    osds = truth.spectra(cases, orc.SpecData)
    # route one: every spectrum its own matrices (the package's and the oracle's
    # construct_resol_mat are the same function of lam and width)
    mats = [rtruth.matrices(sp, _job_of_spectrum(s), spec_fit)
            for s, sp in enumerate(sds)]
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


_truths = {}


def _truth(su, olibs, npoly):
    """[(value, grad, F, G, cond)] of JOBS under the spectra's own matrices, once"""
    if npoly not in _truths:
        out = []
        for j, (s, v, p, vs) in enumerate(truth.JOBS):
            val, g = rtruth.chisq_and_grad(su['osds'][s], olibs, su['omats'][s], v, p, vs,
                                           npoly=npoly)
            F, G, cond = rtruth.fisher(su['osds'][s], olibs, su['omats'][s], v, p, vs,
                                       npoly=npoly, key=('own', s))
            out.append((val, g, F, G, cond))
        _truths[npoly] = out
    return _truths[npoly]


def _engine_call(su, npoly, batch=None, resols=None, fisher=False, order=None,
                 resol_gradient=True, jobs=None):
    """engine.chisq_point_grad / _fisher and engine.chisq_point on JOBS (or `jobs`, a
    list of job numbers) of `batch`, with the same `resols`"""
    from rvspecfit_amd import engine
    batch = su['batch'] if batch is None else batch
    sel = list(range(J)) if jobs is None else list(jobs)
    if order is not None:
        sel = [sel[i] for i in order]
    sel = torch.tensor(sel, device=su['dev'])
    par, vs = su['par'][sel].contiguous(), su['vs'][sel].contiguous()
    libs = su['libs']
    cg, c0, og = [], [], []
    for arm in batch.arms:
        c, o = engine.build_templates(libs[arm.name], par, vs, tangents=True)
        cg.append(c)
        og.append(o)
        c0.append(engine.build_templates(libs[arm.name], par, vs)[0])
    js = su['idx'][sel].to(torch.int32).contiguous()
    vel = su['vel'][sel].contiguous()
    call = engine.chisq_point_fisher if fisher else engine.chisq_point_grad
    res = call(batch, libs, cg, og, vel, npoly, True, js, None, 0.0, True,
               resols=resols, resol_gradient=resol_gradient)
    ref, rst = engine.chisq_point(batch, libs, c0, og, vel, npoly=npoly, rbf=True,
                                  job_spec=js, resols=resols)
    return res, ref, rst


def _jobs(su, npoly, fisher=True, vsini_grad=False, order=None, batch=None, rp=None):
    from rvspecfit_amd import spec_fit
    sel = torch.tensor(list(range(J)) if order is None else order, device=su['dev'])
    f = spec_fit.chisq_fisher_jobs if fisher else spec_fit.chisq_grad_jobs
    return f(su['batch'] if batch is None else batch, su['idx'][sel], su['vel'][sel],
             su['par'][sel], su['vs'][sel], dict(npoly=npoly), su['cfg'],
             resol_params=rp, vsini_grad=vsini_grad)


def _rel(F, Ft, G):
    g = np.sqrt(np.diag(G))
    return np.abs(F - Ft) / (g[:, None] * g[None, :])


# ---- 1. the value ---------------------------------------------------------------------
@pytest.mark.parametrize('npoly', NPOLY)
def test_values_are_chisq_points(setup, npoly):
    (chi, grad, st), ref, rst = _engine_call(setup, npoly)
    assert torch.equal(st, rst)
    assert grad.shape == (J, 1 + ND)
    for j in range(J):
        a, b = chi[j].item(), ref[j].item()
        print('npoly %d job %d value %.15g chisq_point %.15g' % (npoly, j, a, b))
        assert abs(a - b) < 1e-11 * max(abs(b), 1e3), (j, a, b)
    (chi2, grad2, F, st2), _, _ = _engine_call(setup, npoly, fisher=True)
    assert torch.equal(chi2, chi) and torch.equal(grad2, grad) and torch.equal(st2, st)


# ---- 2. the gradient against the truth ------------------------------------------------
def _forward_difference(su, npoly):
    """scipy's forward difference, step 1.49e-8 * max(|x|, 1), of engine.chisq_point
    under the same matrices (templates rebuilt at every point)"""
    from rvspecfit_amd import engine
    b, libs = su['batch'], su['libs']
    x = torch.cat([su['vel'][:, None], su['par']], dim=1)
    h = 1.4901161193847656e-08 * torch.clamp(x.abs(), min=1.0)
    pts = x[:, None, :].repeat(1, 6, 1)
    for k in range(5):
        pts[:, 1 + k, k] += h[:, k]
    h = pts[:, 1:, :].diagonal(dim1=1, dim2=2) - x
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
def test_gradient_against_the_truth(setup, olibs, npoly):
    want = _truth(setup, olibs, npoly)
    (chi, grad, st), _, _ = _engine_call(setup, npoly)
    grad = grad.cpu().numpy()
    fd = _forward_difference(setup, npoly)
    worst, bad = 0.0, []
    for j in truth.INSIDE:
        val, g = want[j][:2]
        assert int(st[j].item()) == 0
        assert abs(chi[j].item() - val) <= 1e-11 * max(abs(val), 1e3)
        scale = np.maximum(np.abs(g), 1e-6 * np.abs(g).max())
        e_an, e_fd = np.abs(grad[j] - g), np.abs(fd[j] - g)
        for k in range(5):
            print('npoly %d job %d comp %d truth %.12g analytic err %.3g (rel %.3g) '
                  'forward-difference err %.3g' % (npoly, j, k, g[k], e_an[k],
                                                   e_an[k] / scale[k], e_fd[k]))
            if not (e_an[k] <= e_fd[k] and e_an[k] <= GRAD_BOUND * scale[k]):
                bad.append((j, k, e_an[k], e_fd[k], e_an[k] / scale[k]))
        worst = max(worst, float((e_an / scale).max()))
    print('npoly %d largest relative gradient error %.3g (bound %.3g)'
          % (npoly, worst, GRAD_BOUND))
    assert not bad, bad


# ---- 3. the Fisher matrix against the QR truth -------------------------------------------
@pytest.mark.parametrize('npoly', NPOLY)
def test_fisher_against_the_truth(setup, olibs, npoly):
    want = _truth(setup, olibs, npoly)
    chi, grad, F, st = _jobs(setup, npoly)
    assert F.shape == (J, 1 + ND, 1 + ND)
    assert torch.equal(F, F.transpose(-1, -2))
    F = F.cpu().numpy()
    worst = 0.0
    for j in truth.INSIDE:
        _, _, Ft, G, cond = want[j]
        ratio = (np.diag(Ft) / np.diag(G)).min()
        assert cond < 100 and ratio > 0.1, (j, cond, ratio)
        assert int(st[j].item()) == 0
        rel = _rel(F[j], Ft, G)
        ev = np.linalg.eigvalsh(F[j]).min()
        print('npoly %d job %d cond(A) %.3g min F_ii/G_ii %.3g largest error %.3g of '
              'sqrt(G_ii G_ll), smallest eigenvalue / trace %.3g'
              % (npoly, j, cond, ratio, rel.max(), ev / np.trace(F[j])))
        assert ev >= -1e-12 * np.trace(F[j])
        worst = max(worst, float(rel.max()))
    print('npoly %d largest Fisher error %.3g (bound %.3g)' % (npoly, worst, FISHER_BOUND))
    assert worst <= FISHER_BOUND


# ---- 4. both routes to a matrix ----------------------------------------------------------
def test_both_routes_and_a_mixed_call(setup, olibs):
    from rvspecfit_amd import spec_fit
    su = setup
    npoly = 10
    # the matrices of spectrum 0 on every spectrum: as SpecData.resolution (taps
    # [S, npix, nd]) and as resol_params (one matrix, taps_stride 0)
    same = _batch(su['sds'], [su['mats'][0]] * 3)
    rp = {x.name: R for x, R in zip(su['sds'][0], su['mats'][0])}
    a = _jobs(su, npoly, batch=same)
    b = _jobs(su, npoly, batch=su['plain'], rp=rp)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    with pytest.raises(ValueError, match='not allowed to set resol_param'):
        _jobs(su, npoly, batch=same, rp=rp)
    # one spectrum, public form: the batch's row
    s, vel, par, _ = truth.JOBS[1]
    c1, g1, F1 = spec_fit.get_chisq_fisher(
        [spec_fit.SpecData(x.name, x.lam, x.spec, x.espec, badmask=x.badmask)
         for x in su['sds'][s]], vel, par, options=dict(npoly=npoly), config=su['cfg'],
        resol_params=rp)
    assert c1 == b[0][1].item() and (g1 == b[1][1].cpu().numpy()).all()
    assert (F1 == b[2][1].cpu().numpy()).all()
    # a matrix on the blue arm only
    mixed = _batch(su['sds'], [[m[0], None] for m in su['mats']])
    chi, grad, F, st = _jobs(su, npoly, batch=mixed)
    grad, F = grad.cpu().numpy(), F.cpu().numpy()
    for j in truth.INSIDE:
        s, v, p, vs = truth.JOBS[j]
        mats = [su['omats'][s][0], None]
        val, g = rtruth.chisq_and_grad(su['osds'][s], olibs, mats, v, p, vs, npoly=npoly)
        Ft, G, _ = rtruth.fisher(su['osds'][s], olibs, mats, v, p, vs, npoly=npoly,
                                 key=('mixed', s))
        scale = np.maximum(np.abs(g), 1e-6 * np.abs(g).max())
        eg, ef = (np.abs(grad[j] - g) / scale).max(), _rel(F[j], Ft, G).max()
        print('mixed job %d gradient error %.3g Fisher error %.3g' % (j, eg, ef))
        assert abs(chi[j].item() - val) <= 1e-11 * max(abs(val), 1e3)
        assert eg <= BAND_GRAD_BOUND and ef <= FISHER_BOUND


# ---- 5. the identity matrix ---------------------------------------------------------------
def _ulps(a, b):
    a, b = a.cpu().numpy().ravel(), b.cpu().numpy().ravel()
    with np.errstate(invalid='ignore'):
        return np.where(a == b, 0.0, np.abs(a - b) / np.spacing(np.maximum(np.abs(a),
                                                                           np.abs(b))))


@pytest.mark.parametrize('npoly', NPOLY)
def test_identity_matrix_is_the_call_without(setup, npoly):
    from rvspecfit_amd import engine
    su = setup
    b = su['plain']
    ident = [engine.make_resol(np.ones((1, arm.npix, 1)), 1, b.S, su['dev'])
             for arm in b.arms]
    for fisher in (False, True):
        with_r, _, _ = _engine_call(su, npoly, batch=b, resols=ident, fisher=fisher)
        without, _, _ = _engine_call(su, npoly, batch=b, fisher=fisher,
                                     resol_gradient=False)
        assert torch.equal(with_r[-1], without[-1])
        for name, x, y in zip(('value', 'gradient', 'fisher'), with_r[:-1], without[:-1]):
            u = _ulps(x, y)
            print('npoly %d fisher=%s %s: bit-equal %s, largest difference %.1f ulp'
                  % (npoly, fisher, name, torch.equal(x, y), np.nanmax(u)))
            assert torch.equal(x.isnan(), y.isnan()) and np.nanmax(u) <= 4


# ---- 6. a band wider than a tile's halo, and the limit ------------------------------------
def test_wide_band_and_the_lds_limit(setup, olibs):
    from rvspecfit_amd import engine, spec_fit
    su = setup
    npoly, j = 10, 1
    s, v, p, vs = truth.JOBS[j]
    wide = [spec_fit.construct_resol_mat(x.lam, width=12.) for x in su['sds'][s]]
    nds = [rtruth.ndiag(R.mat) for R in wide]
    print('diagonals of the width = 12 matrices', nds)
    assert min(nds) > 129            # wider than half a tile on either side
    rp = {x.name: R for x, R in zip(su['sds'][s], wide)}
    chi, grad, F, st = _jobs(su, npoly, batch=su['plain'], rp=rp, order=[j])
    mats = [R.mat for R in wide]
    val, g = rtruth.chisq_and_grad(su['osds'][s], olibs, mats, v, p, vs, npoly=npoly)
    Ft, G, _ = rtruth.fisher(su['osds'][s], olibs, mats, v, p, vs, npoly=npoly)
    scale = np.maximum(np.abs(g), 1e-6 * np.abs(g).max())
    eg = (np.abs(grad[0].cpu().numpy() - g) / scale).max()
    ef = _rel(F[0].cpu().numpy(), Ft, G).max()
    print('wide band: value %.15g truth %.15g gradient error %.3g Fisher error %.3g'
          % (chi[0].item(), val, eg, ef))
    assert int(st[0].item()) == 0
    assert abs(chi[0].item() - val) <= 1e-11 * max(abs(val), 1e3)
    assert eg <= BAND_GRAD_BOUND and ef <= FISHER_BOUND
    # the widest band the tiles hold beside ntan = 4 tangents, and the next odd one
    b = su['plain']
    nd_max = engine.GRAD_RESOL_LDS_MAX // (8 * (2 + ND)) - 255
    nd_max -= 1 - nd_max % 2
    assert (2 + ND) * (255 + nd_max + 2) * 8 > engine.GRAD_RESOL_LDS_MAX
    rng = np.random.default_rng(11)

    def resols(nd):
        # smooth positive rows, normalised over the pixels inside the arm
        out, dense = [], []
        for arm in b.arms:
            m = (nd - 1) // 2
            off = np.arange(-m, m + 1)
            k = np.arange(arm.npix)
            w = np.exp(-0.5 * (off[None, :] / 40.)**2) * \
                (1 + 0.1 * rng.uniform(-1, 1, (arm.npix, nd)))
            q = k[:, None] + off[None, :]
            w = np.where((q >= 0) & (q < arm.npix), w, 0.0)
            w /= w.sum(axis=1)[:, None]
            R = np.zeros((arm.npix, arm.npix))
            ok = (q >= 0) & (q < arm.npix)
            R[np.broadcast_to(k[:, None], q.shape)[ok], q[ok]] = w[ok]
            out.append(engine.make_resol(w[None], nd, b.S, su['dev']))
            dense.append(R)
        return out, dense
    rs, dense = resols(nd_max)
    (chi, grad, st), ref, rst = _engine_call(su, npoly, batch=b, resols=rs, jobs=[j])
    import scipy.sparse
    val, g = rtruth.chisq_and_grad(su['osds'][s], olibs,
                                   [scipy.sparse.csr_matrix(R) for R in dense], v, p, vs,
                                   npoly=npoly)
    scale = np.maximum(np.abs(g), 1e-6 * np.abs(g).max())
    eg = (np.abs(grad[0].cpu().numpy() - g) / scale).max()
    print('nd = %d: value %.15g truth %.15g chisq_point %.15g gradient error %.3g'
          % (nd_max, chi[0].item(), val, ref[0].item(), eg))
    assert torch.equal(st, rst) and int(st[0].item()) == 0
    assert abs(chi[0].item() - val) <= 1e-11 * max(abs(val), 1e3)
    assert eg <= BAND_GRAD_BOUND
    rs, _ = resols(nd_max + 2)
    for fisher in (False, True):
        with pytest.raises(ValueError, match=r'limit is %d \(nd <= %d\)'
                           % (engine.GRAD_RESOL_LDS_MAX, nd_max)):
            _engine_call(su, npoly, batch=b, resols=rs, fisher=fisher, jobs=[j])


# ---- 7. determinism -----------------------------------------------------------------------
def test_determinism(setup):
    a = _jobs(setup, 10)
    b = _jobs(setup, 10)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    perm = [4, 2, 6, 0, 5, 1, 3]
    c = _jobs(setup, 10, order=perm)
    sel = torch.tensor(perm, device=setup['dev'])
    for x, y in zip(a, c):
        assert torch.equal(x[sel], y)
    g = _jobs(setup, 10, fisher=False)
    assert torch.equal(g[0], a[0]) and torch.equal(g[1], a[1]) and torch.equal(g[2], a[3])


# ---- 8. the jobs that are not inside a cell -----------------------------------------------
def test_penalties(setup, olibs):
    npoly = 10
    want = _truth(setup, olibs, npoly)
    (chi, grad, F, st), ref, _ = _engine_call(setup, npoly, fisher=True)
    grad, F = grad.cpu().numpy(), F.cpu().numpy()
    val, g, Ft, G, _ = want[5]
    assert abs(chi[5].item() - ref[5].item()) < 1e-11 * max(abs(ref[5].item()), 1e3)
    assert abs(chi[5].item() - val) <= 1e-11 * max(abs(val), 1e3)
    assert not grad[5, 1:].any() and not g[1:].any()
    print('outside job d/dvel %.12g truth %.12g' % (grad[5, 0], g[0]))
    assert abs(grad[5, 0] - g[0]) <= GRAD_BOUND * abs(g[0])
    assert F[5][0, 0] > 0 and not F[5][1:].any() and not F[5][:, 1:].any()
    assert abs(F[5][0, 0] - Ft[0, 0]) <= FISHER_BOUND * G[0, 0]
    assert chi[6].item() == 2 * 1000.0 * setup['batch'].badchi == want[6][0]
    assert not grad[6].any() and not F[6].any()


# ---- 9. vsini as one more parameter -------------------------------------------------------
def test_vsini_gradient(setup, olibs):
    su = setup
    npoly, j = 10, 3
    s, v, p, vs = truth.JOBS[j]
    chi, grad, F, st = _jobs(su, npoly, vsini_grad=True)
    chi0, grad0, F0, st0 = _jobs(su, npoly)
    assert grad.shape == (J, 2 + ND) and F.shape == (J, 2 + ND, 2 + ND)
    assert torch.equal(grad[:, :1 + ND], grad0) and torch.equal(chi, chi0)
    assert torch.equal(F[:, :1 + ND, :1 + ND], F0)
    assert torch.equal(F, F.transpose(-1, -2))
    val, g = rtruth.chisq_and_grad(su['osds'][s], olibs, su['omats'][s], v, p, vs,
                                   npoly=npoly, vsini_fit=True)
    got = grad[j].cpu().numpy()
    scale = np.maximum(np.abs(g), 1e-6 * np.abs(g).max())
    err = np.abs(got - g) / scale
    print('vsini component %.12g truth %.12g relative error %.3g (all %s)'
          % (got[-1], g[-1], err[-1], err))
    assert g[-1] != 0 and (err <= GRAD_BOUND).all()
    for jj in range(J):
        if truth.JOBS[jj][3] is None:
            assert grad[jj, -1].item() == 0 and not F[jj, -1].any()


# ---- 10. vel_fit -----------------------------------------------------------------------------
def test_fisher_uncertainties(setup, olibs):
    """the batch with its matrices and the priors of test_chisq_fisher_cpu.py's host part
    (teff sigma 150 / 100 / 50 K, feh sigma 0.3 dex): the covariance is the host inverse
    of the truth's F + priors to 1e-9 of sqrt(C_ii C_ll)"""
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.spec_inter import getSpecParams
    su = setup
    npoly = 10
    names = list(getSpecParams('gold_b', su['cfg']))
    want = _truth(su, olibs, npoly)
    sig = np.array([150.0, 100.0, 50.0])
    priors = {'teff': (np.full(3, 6000.0), sig), 'feh': (np.full(3, -0.5),
                                                         np.full(3, 0.3))}
    r = vel_fit.fisher_uncertainties(su['batch'], su['vel'][:3], su['par'][:3],
                                     options=dict(npoly=npoly), config=su['cfg'],
                                     priors=priors)
    assert r['names'] == ['vel'] + names and not r['bad_fisher'].any()
    it, ife = 1 + names.index('teff'), 1 + names.index('feh')
    for s in range(3):
        Ft = want[s][2].copy()
        Ft[it, it] += 1 / sig[s]**2
        Ft[ife, ife] += 1 / 0.3**2
        d = 1 / np.sqrt(np.diag(Ft))
        C = np.linalg.inv(Ft * d[:, None] * d[None, :]) * d[:, None] * d[None, :]
        sc = np.sqrt(np.diag(C))
        rel = np.abs(r['covar'][s] - C) / (sc[:, None] * sc[None, :])
        print('spectrum %d covar error %.3g cond(F) %.3g vel_err %.4g'
              % (s, rel.max(), np.linalg.cond(Ft), r['vel_err'][s]))
        assert rel.max() <= 1e-9
        assert np.isfinite(r['vel_err'][s]) and r['vel_err'][s] > 0
    with pytest.raises(ValueError, match='does not take a resolution matrix'):
        vel_fit.fisher_uncertainties(su['batch'], su['vel'][:3], su['par'][:3],
                                     options=dict(npoly=npoly),
                                     config=dict(su['cfg'], resol_gradient=False))


def test_process_with_the_lm_polish(setup, monkeypatch):
    """vel_fit.process on the three spectra with resolParams: the LM polish under
    config['resol_gradient'] ends no worse than the differenced polish (+ 1e-6 |chisq|,
    tests/test_bfgs_jac_gpu.py); rvs_lm_run's rounds are the host-driven machine's
    (lm.minimize_lockstep_native on GradChain(fisher=True).rows) bit for bit; without the
    key the call is refused as before"""
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.spec_inter import getSpecParams
    su = setup
    names = list(getSpecParams('gold_b', su['cfg']))
    batch = su['plain']
    rp = {x.name: R for x, R in zip(su['sds'][0], su['mats'][0])}
    pd0 = {k: np.array([truth.JOBS[j][2][i] for j in (0, 1, 2)])
           for i, k in enumerate(names)}
    opt = dict(npoly=10)
    lmk = dict(second_minimizer=True, second_minimizer_lm=True)
    plain_cfg = {k: v for k, v in su['cfg'].items() if k != 'resol_gradient'}
    with pytest.raises(ValueError, match=r"config\['second_minimizer_lm'\]: the analytic "
                       r"gradient does not take a resolution matrix \(arm gold_b\)"):
        vel_fit.process(batch, dict(pd0), options=opt, config=dict(plain_cfg, **lmk),
                        resolParams=rp)
    fd = vel_fit.process(batch, dict(pd0), options=opt,
                         config=dict(plain_cfg, second_minimizer=True), resolParams=rp)
    out = {}
    for name, flag in (('device', True), ('host', False)):
        monkeypatch.setattr(vel_fit, 'BFGS_ON_DEVICE', flag)
        out[name] = vel_fit.process(batch, dict(pd0), options=opt,
                                    config=dict(su['cfg'], **lmk), resolParams=rp)
    a, b = out['device'], out['host']
    assert a['lm']['device'] and not b['lm']['device'] and 'bfgs' not in a
    ca, cb = a['chisq'].cpu().numpy(), fd['chisq'].cpu().numpy()
    print('chisq lm', ca, 'differenced', cb, 'lm - differenced', ca - cb, 'nit',
          a['lm']['nit'], 'nfev', a['lm']['nfev'], 'status', a['lm']['status'])
    assert (ca <= cb + 1e-6 * np.abs(cb)).all(), ca - cb
    for k in ('nit', 'nfev', 'status', 'mu', 'fun'):
        assert np.array_equal(np.asarray(a['lm'][k]), np.asarray(b['lm'][k])), k
    assert b['lm']['rounds'] <= a['lm']['rounds'] < b['lm']['rounds'] + 4
    for k in ('vel', 'vel_err', 'chisq', 'vsini', 'nm_vel'):
        if k in a:
            assert torch.equal(a[k], b[k]), k
    for k in names:
        assert torch.equal(a['param'][k], b['param'][k]), k
    # the BFGS polish on the analytic gradient and the Fisher covariance take the key too
    monkeypatch.setattr(vel_fit, 'BFGS_ON_DEVICE', True)
    j = vel_fit.process(batch, dict(pd0), options=opt, resolParams=rp,
                        config=dict(su['cfg'], second_minimizer=True,
                                    second_minimizer_jac=True,
                                    fisher_uncertainties=True))
    cj = j['chisq'].cpu().numpy()
    print('chisq jac', cj, 'jac - differenced', cj - cb)
    assert j['bfgs']['jac'] is True and (cj <= cb + 1e-6 * np.abs(cb)).all()
    par = torch.stack([j['param'][k] for k in names], dim=1)
    fu = vel_fit.fisher_uncertainties(batch, j['vel'], par, options=opt,
                                      config=su['cfg'], resolParams=rp)
    assert np.array_equal(j['covar_fisher'], fu['covar'])
    assert np.isfinite(fu['vel_err']).all() and (fu['vel_err'] > 0).all()


# ---- 11. the DESI driver ---------------------------------------------------------------------
def test_proc_desi_with_resolution_matrices_and_the_keys(dcases, desi_libs, tmp_path):
    """proc_desi(use_resolution_matrix=True) -- the driver's --resolution_matrix -- with
    the LM polish, the Fisher covariance and config['resol_gradient'] handed through its
    config: the fibres of tests/test_desi_gpu.py's 'resol' run are fitted, and end where
    the reference's differenced fit ended or lower (that test's condition)"""
    from rvspecfit_amd import fits_min as F
    from rvspecfit_amd.desi import desi_fit as D
    cases = dcases
    tabf, modf = str(tmp_path / 'rvtab.fits'), str(tmp_path / 'rvmod.fits')
    cfg = dict(CFG, second_minimizer_lm=True, fisher_uncertainties=True,
               resol_gradient=True)
    n = D.proc_desi(COADD, tabf, modf, None, cfg, doplot=False, cmdline='golden resol',
                    **RUNS['resol']())
    assert n == int(cases['resol/nfit'])
    tab = F.open(tabf, verify_checksum=True)['RVTAB'].data
    chi, ref = tab['CHISQ_TOT'], cases['resol/tab/RVTAB/col/CHISQ_TOT']
    good = np.isfinite(ref)
    print('CHISQ_TOT', chi, 'reference', ref)
    assert np.array_equal(np.isfinite(chi), good)
    assert np.all(chi[good] <= ref[good] + 5e-3)
    with pytest.raises(ValueError, match='does not take a resolution matrix'):
        D.proc_desi(COADD, tabf, modf, None, dict(CFG, second_minimizer_lm=True),
                    doplot=False, cmdline='golden resol', **RUNS['resol']())
