"""rvs_chisq_point_fisher and the interfaces above it against tests/chisq_fisher_truth.py
(float64 torch / numpy on the CPU, itself pinned by test_chisq_fisher_cpu.py): the J = 7
jobs of chisq_grad_truth.JOBS over 3 spectra on the two golden arms at npoly 5, 10 and
16, the same jobs on the golden Delaunay libraries at npoly 10, and seeded smooth tangent
rows through engine.chisq_point_fisher for every basis size and tangent count.

The bound is the project's own for this chain of sums, 10 x MEASURED_REL_ERR of
tests/test_chisq_grad_gpu.py = 5.84e-12, relative to sqrt(G_ii G_ll), G = J^T J the
unprojected Gram matrix (the subtraction F = G - B^T B happens at that scale).

Largest |F_dev - F_truth|_il / sqrt(G_ii G_ll) seen on an MI355X (first device run):
  golden arms 1.49e-15 (npoly 5), 1.52e-15 (npoly 10), 1.80e-15 (npoly 16); Delaunay
  libraries 1.95e-15 (npoly 10); generic rows 2.16e-15 (200 px, one arm, over every
  ntan / npoly) -- the truth's own float64 rounding; the bound leaves three decades."""
import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG, gold_lib_dict
from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import chisq_fisher_truth as ftruth
from test_chisq_grad_gpu import MEASURED_REL_ERR

pytestmark = pytest.mark.gpu
J = len(truth.JOBS)
ND = 4
BOUND = 10 * MEASURED_REL_ERR
C_KMS = truth.C_KMS


def _make_setup(cases, tri):
    from rvspecfit_amd import _lib, spec_inter, spec_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    url = 'golden-tri://' if tri else 'golden://'
    cfg = dict(GOLD_CONFIG, template_lib=url)
    for n in ('gold_b', 'gold_r'):
        if tri:
            import tri_grad_truth as ttruth
            d = ttruth.tri_lib_dict(n)
        else:
            d = gold_lib_dict(n)
        spec_inter.register_library(TemplateLibrary(n, d), url)
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
def setup(cases):
    return _make_setup(cases, False)


@pytest.fixture(scope='module')
def setup_tri(cases):
    return _make_setup(cases, True)


@pytest.fixture(scope='module')
def olibs():
    return {n: orc.Library(gold_lib_dict(n)) for n in ('gold_b', 'gold_r')}


def _jobs(su, npoly, vsini_grad=False, order=None, fisher=True):
    from rvspecfit_amd import spec_fit
    sel = torch.tensor(list(range(J)) if order is None else order, device=su['dev'])
    f = spec_fit.chisq_fisher_jobs if fisher else spec_fit.chisq_grad_jobs
    return f(su['batch'], su['idx'][sel], su['vel'][sel], su['par'][sel], su['vs'][sel],
             dict(npoly=npoly), su['cfg'], vsini_grad=vsini_grad)


def _rel(F, Ft, G):
    g = np.sqrt(np.diag(G))
    return np.abs(F - Ft) / (g[:, None] * g[None, :])


# ---- 1. against the truth ------------------------------------------------------------
def _against_truth(su, want, inside, npoly, tag):
    chi, grad, F, st = _jobs(su, npoly)
    assert F.shape == (J, 1 + ND, 1 + ND)
    F = F.cpu().numpy()
    worst = 0.0
    for j in inside:
        Ft, G, cond = want[j]
        ratio = (np.diag(Ft) / np.diag(G)).min()
        # what keeps the bound meaningful, from the truth alone
        assert cond < 100 and ratio > 0.1, (j, cond, ratio)
        assert int(st[j].item()) == 0
        rel = _rel(F[j], Ft, G)
        print('%s npoly %d job %d cond(A) %.3g min F_ii/G_ii %.3g largest error %.3g of '
              'sqrt(G_ii G_ll)' % (tag, npoly, j, cond, ratio, rel.max()))
        worst = max(worst, float(rel.max()))
    print('%s npoly %d largest error %.3g (bound %.3g)' % (tag, npoly, worst, BOUND))
    assert worst <= BOUND
    return F


@pytest.mark.parametrize('npoly', [5, 10, 16])
def test_fisher_against_the_truth(cases, setup, olibs, npoly):
    want = ftruth.truth_jobs(cases, olibs, npoly)
    F = _against_truth(setup, want, truth.INSIDE, npoly, 'grid')
    # outside the grid: the velocity entry alone, and it is the truth's
    Ft, G, _ = want[5]
    assert abs(F[5][0, 0] - Ft[0, 0]) <= BOUND * G[0, 0]


def test_fisher_against_the_truth_delaunay(cases, setup_tri):
    """chisq_grad_truth.JOBS on the golden Delaunay libraries: the in-cell jobs that a
    simplex of the triangulation holds (both arms share it)"""
    import tri_grad_truth as ttruth
    tlibs = ttruth.oracle_libs()
    lib = tlibs['gold_b']
    inside = [j for j in truth.INSIDE
              if lib.find_simplex(lib.map_params(np.array(truth.JOBS[j][2]))) >= 0]
    print('jobs in a simplex:', inside)
    assert len(inside) >= 3
    want = ftruth.truth_jobs(cases, tlibs, 10, template_fn=ftruth.tri_template,
                             key='tri')
    _against_truth(setup_tri, want, inside, 10, 'delaunay')


# ---- 2. generic tangent rows through the engine ---------------------------------------
def _smooth_records(rng, knots, nrow):
    """[nrow, ntp, 4] form-1 records (value, b, c, d of ((d dl + c) dl + b) dl + value) of
    the C1 Hermite cubics through seeded sums of sinusoids in ln(lambda)"""
    u = np.log(knots / knots[0]) / np.log(knots[-1] / knots[0])
    rec = np.zeros((nrow, len(knots), 4))
    h = np.diff(knots)
    dudl = 1.0 / (knots * np.log(knots[-1] / knots[0]))
    for r in range(nrow):
        y, dy = np.zeros_like(u), np.zeros_like(u)
        for _ in range(4):
            a, w, ph = rng.normal(), rng.uniform(2, 60), rng.uniform(0, 2 * np.pi)
            y += a * np.sin(w * u + ph)
            dy += a * w * np.cos(w * u + ph) * dudl
        sl = np.diff(y) / h
        rec[r, :, 0] = y
        rec[r, :-1, 1] = dy[:-1]
        rec[r, :-1, 2] = (3 * sl - 2 * dy[:-1] - dy[1:]) / h
        rec[r, :-1, 3] = (dy[:-1] + dy[1:] - 2 * sl) / h**2
    return rec


def _numpy_fisher(arm, knots, rec, s, vel, Qt):
    """one arm: F and G in numpy float64 from the records the kernel reads"""
    lam = arm.lam.cpu().numpy().reshape(-1)
    D = arm.spec[s].cpu().numpy()
    e = arm.espec[s].cpu().numpy()
    b = vel / C_KMS
    f = np.sqrt((1 - b) / (1 + b))
    dfdv = -f / (C_KMS * (1 - b * b))
    x = lam * f
    pos = np.clip(np.searchsorted(knots, x, 'right') - 1, 0, len(knots) - 2)
    dl = x - knots[pos]
    ev = lambda c: ((c[pos, 3] * dl + c[pos, 2]) * dl + c[pos, 1]) * dl + c[pos, 0]  # noqa
    m = ev(rec[0])
    dm = (3 * rec[0][pos, 3] * dl + 2 * rec[0][pos, 2]) * dl + rec[0][pos, 1]
    tang = [dm * lam * dfdv] + [ev(rec[i]) for i in range(1, len(rec))]
    STt = Qt * (m / e)[:, None]
    U, R = np.linalg.qr(STt)
    c = np.linalg.solve(R, U.T @ (D / e))
    sfit = Qt @ c
    Jw = np.stack(tang, axis=1) * (sfit / e)[:, None]
    Jp = Jw - U @ (U.T @ Jw)
    return Jp.T @ Jp, Jw.T @ Jw


@pytest.mark.parametrize('narm', [1, 2])
@pytest.mark.parametrize('npix', [200, 257, None])
def test_generic_rows(cases, setup, npix, narm):
    """ntan 0, 1, 4, 6 (K = 7: the vsini position) x npoly 1, 5, 10, 16 on arms cut to 200
    pixels (idle lanes), 257 (one pixel in the second sweep) and the golden size, one and
    two arms; three jobs over two spectra through job_spec / job_templ"""
    from rvspecfit_amd import engine, spec_fit
    from rvspecfit_amd.engine import SpecBatch
    su = setup
    dev = su['dev']
    sds = [[spec_fit.SpecData(x.name, x.lam[:npix], x.spec[:npix], x.espec[:npix],
                              badmask=x.badmask[:npix]) for x in sp[:narm]]
           for sp in su['sds'][:2]]
    batch = SpecBatch.from_specdata(sds)
    libs = su['libs']
    js = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    jt = torch.tensor([0, 1, 1], dtype=torch.int32, device=dev)
    vels = [5.5, -212.7, 37.3]
    vel = torch.tensor(vels, dtype=torch.float64, device=dev)
    par = su['par'][:2].contiguous()
    rng = np.random.default_rng(1000 * narm + (npix or 0))
    worst = 0.0
    for ntan in (0, 1, 4, 6):
        coefs, outs, recs = [], [], []
        for arm in batch.arms:
            lib = libs[arm.name]
            c0, o = engine.build_templates(lib, par, None)
            knots = lib.knots.cpu().numpy()
            rec = np.concatenate([
                np.concatenate([c0[t].cpu().numpy().reshape(1, lib.ntp, 4),
                                _smooth_records(rng, knots, ntan)])[None]
                for t in range(2)])                               # [2, 1 + ntan, ntp, 4]
            recs.append(rec)
            coefs.append(torch.as_tensor(rec).to(dev).contiguous())
            outs.append(o)
        for npoly in (1, 5, 10, 16):
            chi, grad, F, st = engine.chisq_point_fisher(
                batch, libs, coefs, outs, vel, npoly, True, js, jt)
            chi2, grad2, st2 = engine.chisq_point_grad(
                batch, libs, coefs, outs, vel, npoly, True, js, jt)
            assert torch.equal(chi, chi2) and torch.equal(grad, grad2)
            assert torch.equal(st, st2) and not st.any()
            assert F.shape == (3, 1 + ntan, 1 + ntan)
            assert torch.equal(F, F.transpose(-1, -2))
            F = F.cpu().numpy()
            for j in range(3):
                Ft = np.zeros((1 + ntan, 1 + ntan))
                G = np.zeros_like(Ft)
                for ia, arm in enumerate(batch.arms):
                    # (one grid: [1, npix + 1, npoly], the pixels' rows first)
                    Qt = arm.basis_ortho(npoly, True)[0].cpu().numpy()
                    a, g = _numpy_fisher(arm, libs[arm.name].knots.cpu().numpy(),
                                         recs[ia][int(jt[j])], int(js[j]), vels[j],
                                         Qt.reshape(-1, npoly)[:arm.npix])
                    Ft += a
                    G += g
                rel = _rel(F[j], Ft, G).max()
                worst = max(worst, float(rel))
                assert rel <= BOUND, (ntan, npoly, j, rel)
    print('npix %s narm %d largest error %.3g of sqrt(G_ii G_ll) (bound %.3g)'
          % (npix, narm, worst, BOUND))


# ---- 3. nothing else moved -----------------------------------------------------------
@pytest.mark.parametrize('npoly', [5, 10, 16])
def test_value_and_gradient_are_the_gradient_calls(setup, npoly):
    chi, grad, F, st = _jobs(setup, npoly)
    chi0, grad0, st0 = _jobs(setup, npoly, fisher=False)
    assert torch.equal(chi, chi0) and torch.equal(grad, grad0) and torch.equal(st, st0)
    chi, grad, F, st = _jobs(setup, npoly, vsini_grad=True)
    chi0, grad0, st0 = _jobs(setup, npoly, vsini_grad=True, fisher=False)
    assert torch.equal(chi, chi0) and torch.equal(grad, grad0) and torch.equal(st, st0)


# ---- 4. exactness properties ---------------------------------------------------------
@pytest.mark.parametrize('which', ['grid', 'tri'])
def test_exactness_properties(setup, setup_tri, which):
    su = setup if which == 'grid' else setup_tri
    for npoly in (5, 10, 16):
        chi, grad, F, st = _jobs(su, npoly)
        assert torch.equal(F, F.transpose(-1, -2))
        Fv = _jobs(su, npoly, vsini_grad=True)[2]
        assert Fv.shape == (J, 2 + ND, 2 + ND)
        assert torch.equal(Fv, Fv.transpose(-1, -2))
        # the leading block: the bits of the call without vsini
        assert torch.equal(Fv[:, :1 + ND, :1 + ND], F)
        # vsini <= 0: the broadening is not applied, its row and column are exactly 0
        for j in range(J):
            if truth.JOBS[j][3] is None:
                assert not Fv[j, 1 + ND].any() and not Fv[j, :, 1 + ND].any()
        if which == 'grid':
            assert Fv[3, 1 + ND, 1 + ND].item() > 0
        Fn = F.cpu().numpy()
        if which == 'grid':
            for j in truth.INSIDE:
                d = np.sqrt(np.diag(Fn[j]))
                assert (d > 0).all()
                ev = np.linalg.eigvalsh(Fn[j] / (d[:, None] * d[None, :]))
                print('npoly %d job %d smallest scaled eigenvalue %.3g'
                      % (npoly, j, ev.min()))
                assert ev.min() >= -1e-11
            # job 5, outside the grid: the nearest node's template, no parameter rows
            assert Fn[5][0, 0] > 0 and not Fn[5][1:].any() and not Fn[5][:, 1:].any()
        # job 6, a non-finite parameter: every arm is skipped
        assert not Fn[6].any() and not Fv[6].any()


# ---- 5. determinism -------------------------------------------------------------------
def test_determinism(setup):
    for vg in (False, True):
        chi, grad, F, st = _jobs(setup, 10, vsini_grad=vg)
        chi2, grad2, F2, st2 = _jobs(setup, 10, vsini_grad=vg)
        assert torch.equal(F, F2) and torch.equal(grad, grad2) and torch.equal(chi, chi2)
        perm = [4, 2, 6, 0, 5, 1, 3]
        chi3, grad3, F3, st3 = _jobs(setup, 10, vsini_grad=vg, order=perm)
        sel = torch.tensor(perm, device=setup['dev'])
        assert torch.equal(F3, F[sel]) and torch.equal(grad3, grad[sel])
        assert torch.equal(chi3, chi[sel]) and torch.equal(st3, st[sel])


# ---- 6. the public layer ---------------------------------------------------------------
def test_single_spectrum_is_the_batch_row(setup):
    from rvspecfit_amd import spec_fit
    su = setup
    opt = dict(npoly=10)
    chi, grad, F, st = _jobs(su, 10)
    cb, gb, Fb = spec_fit.get_chisq_fisher(su['batch'], su['vel'][:3], su['par'][:3],
                                           options=opt, config=su['cfg'])
    assert cb.shape == (3, ) and gb.shape == (3, 1 + ND) and Fb.shape == (3, 5, 5)
    assert torch.equal(Fb, F[:3]) and torch.equal(gb, grad[:3])
    c0, g0 = spec_fit.get_chisq_grad(su['batch'], su['vel'][:3], su['par'][:3],
                                     options=opt, config=su['cfg'])
    assert torch.equal(c0, cb) and torch.equal(g0, gb)
    for s in range(3):
        _, vel, par, _ = truth.JOBS[s]
        c1, g1, F1 = spec_fit.get_chisq_fisher(su['sds'][s], vel, par, options=opt,
                                               config=su['cfg'])
        assert isinstance(c1, float) and g1.shape == (5, ) and F1.shape == (5, 5)
        assert c1 == cb[s].item() and (g1 == gb[s].cpu().numpy()).all()
        assert (F1 == Fb[s].cpu().numpy()).all()
    _, vel, par, vs = truth.JOBS[3]
    c3, g3, F3 = spec_fit.get_chisq_fisher(su['sds'][0], vel, par, (vs, ), options=opt,
                                           config=su['cfg'])
    assert c3 == chi[3].item() and (F3 == F[3].cpu().numpy()).all()
    Fv = _jobs(su, 10, vsini_grad=True)[2]
    c3, g3, F3 = spec_fit.get_chisq_fisher(su['sds'][0], vel, par, (vs, ), options=opt,
                                           config=su['cfg'], vsini_grad=True)
    assert F3.shape == (6, 6) and (F3 == Fv[3].cpu().numpy()).all()
    with pytest.raises(ValueError, match='rot_params'):
        spec_fit.get_chisq_fisher(su['sds'][0], vel, par, options=opt, config=su['cfg'],
                                  vsini_grad=True)


def test_fisher_uncertainties(cases, setup, olibs):
    """the covariance is the float64 host inverse of the truth's F to 1e-8 of
    sqrt(C_ii C_ll): the inversion's conditioning (1e8 ... 1e10 unscaled) times 1e-16,
    two decades of margin; finite positive errors where the exact Hessian is indefinite
    (jobs 0, 2, 3)"""
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.spec_inter import getSpecParams
    su = setup
    opt = dict(npoly=10)
    names = list(getSpecParams('gold_b', su['cfg']))
    want = ftruth.truth_jobs(cases, olibs, 10)
    for j in truth.INSIDE:
        s, vel, par, vs = truth.JOBS[j]
        r = vel_fit.fisher_uncertainties(su['sds'][s], vel, par, vsini=vs, options=opt,
                                         config=su['cfg'])
        assert r['names'] == ['vel'] + names and r['bad_fisher'] is False
        Ft = want[j][0]
        d = 1 / np.sqrt(np.diag(Ft))
        C = np.linalg.inv(Ft * d[:, None] * d[None, :]) * d[:, None] * d[None, :]
        sc = np.sqrt(np.diag(C))
        rel = np.abs(r['covar'] - C) / (sc[:, None] * sc[None, :])
        Cp = np.linalg.inv((Ft * d[:, None] * d[None, :])[1:, 1:]) * \
            d[1:, None] * d[None, 1:]
        relp = np.abs(r['param_covar'] - Cp) / np.sqrt(np.outer(np.diag(Cp), np.diag(Cp)))
        print('job %d covar err %.3g param_covar err %.3g cond(F) %.3g vel_err %.4g'
              % (j, rel.max(), relp.max(), np.linalg.cond(Ft), r['vel_err']))
        assert rel.max() <= 1e-8 and relp.max() <= 1e-8
        errs = np.array([r['vel_err']] + [r['err'][k] for k in names] +
                        [r['param_err'][k] for k in names])
        assert np.isfinite(errs).all() and (errs > 0).all()
        assert r['vel_err'] == r['err']['vel']
        for k in names:     # marginal >= conditional
            assert r['err'][k] >= r['param_err'][k] * (1 - 1e-9)
    # the batch form, a prior and a fixed parameter
    rb = vel_fit.fisher_uncertainties(su['batch'], su['vel'][:3], su['par'][:3],
                                      options=opt, config=su['cfg'])
    r1 = vel_fit.fisher_uncertainties(su['sds'][1], truth.JOBS[1][1], truth.JOBS[1][2],
                                      options=opt, config=su['cfg'])
    assert np.array_equal(rb['fisher'][1], r1['fisher'])
    assert np.array_equal(rb['covar'][1], r1['covar'])
    assert rb['vel_err'][1] == r1['vel_err'] and not rb['bad_fisher'].any()
    rp = vel_fit.fisher_uncertainties(su['sds'][1], truth.JOBS[1][1], truth.JOBS[1][2],
                                      options=opt, config=su['cfg'],
                                      priors={'teff': (6000.0, 120.0)}, fixParam=['feh'])
    it = names.index('teff')
    assert rp['names'] == ['vel'] + [k for k in names if k != 'feh']
    keep = [i for i, k in enumerate(['vel'] + names) if k != 'feh']
    wantF = r1['fisher'].copy()
    wantF[1 + it, 1 + it] += 1 / 120.0**2
    assert np.array_equal(rp['fisher'], wantF[keep][:, keep])
    assert rp['err']['teff'] < r1['err']['teff']
    # outside the grid: zero parameter rows make the entry bad, nothing raises
    s, vel, par, vs = truth.JOBS[5]
    ro = vel_fit.fisher_uncertainties(su['sds'][s], vel, par, options=opt,
                                      config=su['cfg'])
    assert ro['bad_fisher'] is True and np.isfinite(ro['vel_err']) and ro['vel_err'] > 0


def test_process_option(setup):
    """config['fisher_uncertainties']: every existing key keeps its bits, the new keys are
    fisher_uncertainties at the returned optimum"""
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.spec_inter import getSpecParams
    su = setup
    names = list(getSpecParams('gold_b', su['cfg']))
    batch = SpecBatch.from_specdata(su['sds'][:2])
    pd0 = {k: np.array([truth.JOBS[j][2][i] for j in (0, 1)])
           for i, k in enumerate(names)}
    opt = dict(npoly=10)
    cfg = dict(su['cfg'], second_minimizer=False)
    r0 = vel_fit.process(batch, dict(pd0), config=cfg, options=opt)
    r1 = vel_fit.process(batch, dict(pd0), options=opt,
                         config=dict(cfg, fisher_uncertainties=True))
    new = {'covar_fisher', 'names_fisher', 'vel_err_fisher', 'param_err_fisher'}
    assert set(r1) - set(r0) == new and set(r0) <= set(r1)

    def same(a, b):
        if isinstance(a, dict):
            return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        if isinstance(a, torch.Tensor):
            return torch.equal(a, b)
        if isinstance(a, np.ndarray):
            return np.array_equal(a, b, equal_nan=True)
        return a == b
    for k in r0:
        assert same(r0[k], r1[k]), k
    par = torch.stack([r1['param'][k] for k in names], dim=1)
    fu = vel_fit.fisher_uncertainties(batch, r1['vel'], par, options=opt, config=cfg)
    assert r1['names_fisher'] == fu['names'] == ['vel'] + names
    assert np.array_equal(r1['covar_fisher'], fu['covar'])
    assert np.array_equal(r1['vel_err_fisher'].cpu().numpy(), fu['vel_err'])
    assert same(r1['param_err_fisher'], fu['param_err'])
    assert np.isfinite(fu['vel_err']).all() and (fu['vel_err'] > 0).all()
    # one spectrum: the reference's dict with floats, the numbers of the batch's row
    one = vel_fit.process(su['sds'][1], {k: float(v[1]) for k, v in pd0.items()},
                          options=opt, config=dict(cfg, fisher_uncertainties=True))
    assert one['names_fisher'] == fu['names']
    assert isinstance(one['vel_err_fisher'], float) and one['vel_err_fisher'] > 0
    assert one['covar_fisher'].shape == (5, 5)
    assert set(one['param_err_fisher']) == set(names)
    if one['vel'] == r1['vel'][1].item() and all(
            one['param'][k] == r1['param'][k][1].item() for k in names):
        assert np.array_equal(one['covar_fisher'], r1['covar_fisher'][1])
        assert one['vel_err_fisher'] == r1['vel_err_fisher'][1].item()
    with pytest.raises(ValueError, match=r'fisher_uncertainties.*npoly'):
        vel_fit.process(batch, dict(pd0), options=dict(npoly=17),
                        config=dict(cfg, fisher_uncertainties=True))


def test_unsupported_options_raise(cases, setup):
    """what the kernel does not cover is refused by name"""
    import os
    from conftest import GOLD
    from rvspecfit_amd import spec_fit, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    su = setup
    _, vel, par, _ = truth.JOBS[0]
    sd = su['sds'][0]
    kw = dict(config=su['cfg'])
    with pytest.raises(ValueError, match='npoly'):
        spec_fit.get_chisq_fisher(sd, vel, par, options=dict(npoly=17), **kw)
    with pytest.raises(ValueError, match='fast_interp'):
        spec_fit.get_chisq_fisher(sd, vel, par, options=dict(npoly=10),
                                  fast_interp=True, **kw)
    rp = {x.name: spec_fit.construct_resol_mat(x.lam, width=0.5) for x in sd}
    with pytest.raises(ValueError, match='resolution'):
        spec_fit.get_chisq_fisher(sd, vel, par, options=dict(npoly=10),
                                  resol_params=rp, **kw)
    other = [spec_fit.SpecData(x.name, x.lam[:-3], x.spec[:-3], x.espec[:-3],
                               badmask=x.badmask[:-3]) for x in su['sds'][1]]
    gs = SpecBatch.from_specdata([sd, other])
    with pytest.raises(ValueError, match='grid set'):
        spec_fit.get_chisq_fisher(gs, [vel, vel], par, options=dict(npoly=10), **kw)
    d = dict(np.load(os.path.join(GOLD, 'nn_case.npz')))
    lam = np.exp(np.linspace(np.log(4350.), np.log(4800.), int(d['dims'][-1])))
    dd = dict(lam=lam, log_step=np.array(True), log_ids=np.array([0]),
              parnames=np.array(['teff', 'logg', 'feh', 'alpha']),
              nn_dims=d['dims'], nn_M=d['M'], nn_S=d['S'], nn_pts=d['pts'])
    for i in range(len(d['dims']) - 1):
        dd['nn_W%d' % i] = d['W%d' % i]
        dd['nn_b%d' % i] = d['b%d' % i]
    spec_inter.register_library(TemplateLibrary('gold_b', dd), 'golden-nn-fisher://')
    b1 = SpecBatch.from_specdata([sd[:1]])
    with pytest.raises(ValueError, match='regular-grid'):
        spec_fit.get_chisq_fisher(b1, vel, par, options=dict(npoly=10),
                                  config=dict(su['cfg'],
                                              template_lib='golden-nn-fisher://'))
