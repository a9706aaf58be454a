"""CCF template sets built on the device (make_ccf.build_ccf_set, rvs_ccf_models_build)
against the sets the reference made for the committed libraries, against numpy's
transforms, and through fitter_ccf.fit / pipeline.fit_batch."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
LIBS = ('lib_gold_b', 'lib_gold_r', 'lib_desi_b', 'lib_desi_r', 'lib_desi_z')
CFG = dict(min_vel=-1000, max_vel=1000, min_vel_step=0.2, vel_step0=5, min_vsini=0.1,
           max_vsini=500, template_lib='golden://')


def _gold(name):
    return dict(np.load(os.path.join(GOLD, name + '.npz')))


def _conf(d, pre='ccf_'):
    cc = dict(logl0=float(d[pre + 'logl0']), logl1=float(d[pre + 'logl1']),
              npoints=int(d[pre + 'npoints']), continuum=bool(d[pre + 'continuum']),
              maxcontpts=int(d[pre + 'maxcontpts']))
    if cc['continuum']:
        cc['splinestep'] = float(d[pre + 'splinestep'])
    return cc


@pytest.mark.parametrize('name', LIBS)
def test_continuum_normalised_sets_against_the_reference(name):
    """ccf_mod / ccf_fft / ccf_fft2 of rvs_make_ccf --every 20 --vsinis 0,100.  The
    reference's own fit moves by 6e-6 between its stopping rules: 2e-5 of the scale."""
    from rvspecfit_amd import make_ccf
    d = _gold(name)
    s = make_ccf.build_ccf_set(d, _conf(d), every=20, vsinis=[0., 100.])
    assert set(s) == {k for k in d if k.startswith('ccf_')}
    scale = np.max(np.abs(d['ccf_mod']))
    err = np.max(np.abs(s['ccf_mod'] - d['ccf_mod'])) / scale
    print('%s: ccf_mod max deviation %.2e of the scale' % (name, err))
    assert err < 2e-5
    assert np.allclose(s['ccf_params'], d['ccf_params'], rtol=1e-13, atol=0)
    assert np.array_equal(s['ccf_vsinis'], d['ccf_vsinis'])
    for k in ('ccf_fft', 'ccf_fft2'):
        nrm = np.linalg.norm(d[k], axis=1).max()
        assert np.max(np.abs(s[k] - d[k])) < 2e-5 * nrm


@pytest.mark.parametrize('arm', ['b', 'r'])
def test_non_normalised_sets_against_the_reference(arm):
    """--nocontinuum: no fit, only numpy's float32 exp, the vsini kernel and interp1d
    (whose y_hi - y_lo is a float32 difference on an unbroadened row): 1e-12"""
    from rvspecfit_amd import make_ccf
    d = _gold('lib_gold_' + arm)
    n = _gold('lib_nocont_gold_' + arm)
    s = make_ccf.build_ccf_set(d, _conf(n, 'ccfnc_'), every=20, vsinis=[0., 100.])
    assert set(s) == set(n)
    err = np.max(np.abs(s['ccfnc_mod'] - n['ccfnc_mod'])) / np.max(np.abs(n['ccfnc_mod']))
    print('nocont %s: max deviation %.2e' % (arm, err))
    assert err < 1e-12


@pytest.mark.parametrize('nfft', [1024, 2048, 4096, 8192, 16384])
@pytest.mark.parametrize('M', [1, 7])
def test_transforms_against_numpy(nfft, M):
    import torch
    from rvspecfit_amd import make_ccf
    rng = np.random.default_rng(nfft + M)
    lam = 4000 * np.exp(np.arange(700) * 2e-4)
    cc = dict(logl0=np.log(lam[3]), logl1=np.log(lam[-4]), npoints=nfft,
              continuum=False, maxcontpts=20)
    rows = torch.as_tensor(1 + 0.3 * rng.normal(size=(M, 700))).to('cuda')
    r = make_ccf.models_build(lam, rows, cc)
    mod = r['model'].cpu().numpy()
    for k, x in (('fft', mod), ('fft2', mod**2)):
        want = np.fft.rfft(x, axis=1)
        got = r[k].cpu().numpy()
        assert got.shape == want.shape
        err = np.max(np.abs(got - want), axis=1) / np.linalg.norm(want, axis=1)
        assert err.max() < 1e-13, (k, err.max())


def _golden_batch(tag):
    from rvspecfit_amd import spec_fit
    cases = dict(np.load(os.path.join(GOLD, 'cases.npz')))
    names = [str(_) for _ in cases[tag + '/names']]
    return [spec_fit.SpecData(n, cases['%s/%s/lam' % (tag, n)],
                              cases['%s/%s/spec' % (tag, n)],
                              cases['%s/%s/espec' % (tag, n)],
                              badmask=cases['%s/%s/badmask' % (tag, n)]) for n in names]


def test_built_set_through_fit_and_fit_batch():
    """every golden object of cases.npz with the device-built set attached by
    add_ccf_set in place of the reference's: same template, same velocity, same CCF
    surface.  The two kinds of library live under roots of their own."""
    import torch
    from rvspecfit_amd import fitter_ccf, make_ccf, pipeline, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    roots = {False: 'ccfset-reference://', True: 'ccfset-built://'}
    for built, root in roots.items():
        for n in ('gold_b', 'gold_r'):
            d = _gold('lib_' + n)
            lib = TemplateLibrary(n, d)
            if built:
                v0 = lib.ccf_version
                lib.add_ccf_set(make_ccf.build_ccf_set(lib, _conf(d), every=20,
                                                       vsinis=[0., 100.]))
                assert lib.ccf_version == v0 + 1
            spec_inter.register_library(lib, root)
    for tag in ('c0', 'c1', 'c2', 'c3'):
        sds = _golden_batch(tag)
        res = {}
        for built, root in roots.items():
            cfg = dict(CFG, template_lib=root)
            f = fitter_ccf.fit(sds, cfg)
            rec = pipeline.fit_batch(SpecBatch.from_specdata([sds]), cfg,
                                     options=dict(npoly=10)).cpu().numpy()[0]
            torch.cuda.synchronize()
            res[built] = (f, rec)
        (f0, r0), (f1, r1) = res[False], res[True]
        assert f0['best_par'].keys() == f1['best_par'].keys()
        for k in f0['best_par']:
            assert abs(f0['best_par'][k] - f1['best_par'][k]) <= \
                1e-12 * abs(f0['best_par'][k]), (tag, k)
        assert abs(f0['best_vel'] - f1['best_vel']) < 0.01, tag
        sc = np.max(np.abs(f0['best_ccf']))
        assert np.max(np.abs(f0['best_ccf'] - f1['best_ccf'])) < 2e-5 * sc, tag
        assert int(r0[0]) == int(r1[0]) and abs(r0[1] - r1[1]) < 0.01, tag


def test_get_ccf_info_follows_add_ccf_set():
    """fitter_ccf.get_ccf_info caches by setup; a replaced set is handed out at once"""
    from rvspecfit_amd import fitter_ccf, make_ccf, spec_inter
    from rvspecfit_amd.library import TemplateLibrary
    d = _gold('lib_gold_b')
    d['ccf_parnames'] = d['parnames']
    name, cfg = 'ccfinfo_b', dict(CFG, template_lib='ccfset-info://')
    lib = TemplateLibrary(name, d)
    spec_inter.register_library(lib, cfg['template_lib'])
    fft, fft2, mod, info = fitter_ccf.get_ccf_info(name, cfg)
    assert fft.shape == (26, 513) and np.array_equal(mod, d['ccf_mod'])
    s = make_ccf.build_ccf_set(lib, _conf(d), every=50, vsinis=[0., 50., 200.])
    lib.add_ccf_set(s)
    fft, fft2, mod, info = fitter_ccf.get_ccf_info(name, cfg)
    assert fft.shape == (len(s['ccf_vsinis']), 513) and fft.shape[0] != 26
    assert np.array_equal(fft, s['ccf_fft']) and np.array_equal(fft2, s['ccf_fft2'])
    assert np.array_equal(mod, s['ccf_mod'])
    assert np.array_equal(info['vsinis'], s['ccf_vsinis'])
    assert np.array_equal(info['params'], s['ccf_params'])
    fitter_ccf.CCFCache.forget(name)


def test_set_round_trips_through_npz(tmp_path):
    from rvspecfit_amd import make_ccf
    from rvspecfit_amd.library import TemplateLibrary
    d = _gold('lib_gold_b')
    base = {k: v for k, v in d.items() if not k.startswith('ccf_')}
    lib = TemplateLibrary('gold_b', base)
    with pytest.raises(RuntimeError):
        lib.ccf_set({})
    s = make_ccf.build_ccf_set(lib, _conf(d), every=20, vsinis=None)
    assert np.all(np.isnan(s['ccf_vsinis'])) and len(s['ccf_vsinis']) == 13
    lib.add_ccf_set(s)
    p = str(tmp_path / 'lib.npz')
    np.savez(p, **base, **s)
    lib2 = TemplateLibrary.from_npz('gold_b', p)
    a, b = lib.ccf_set({}), lib2.ccf_set({})
    assert a['T'] == b['T'] == 13 and np.array_equal(a['mod'], b['mod'])
    assert np.array_equal(a['fft'].cpu().numpy(), b['fft'].cpu().numpy())
    # vsini None and 0 leave the row alone: the same models
    s0 = make_ccf.build_ccf_set(lib, _conf(d), every=20, vsinis=[0.])
    assert np.array_equal(s0['ccf_mod'], s['ccf_mod'])


def test_rows_do_not_depend_on_the_launch():
    """subset and permutation: bit-identical rows"""
    import torch
    from rvspecfit_amd import make_ccf
    d = _gold('lib_desi_b')
    cc = _conf(d)
    rows = torch.as_tensor(np.exp(d['dats'][:40].astype(np.float64))).to('cuda')
    full = make_ccf.models_build(d['lam'], rows, cc, details=True)
    perm = np.random.default_rng(1).permutation(40)[:17]
    sub = make_ccf.models_build(d['lam'], rows[torch.as_tensor(perm).to('cuda')], cc,
                                details=True)
    for k in ('model', 'fft', 'fft2', 'cont', 'pfit'):
        assert torch.equal(full[k][torch.as_tensor(perm).to('cuda')], sub[k]), k


def test_reference_names_and_edges():
    import torch
    from rvspecfit_amd import _lib, make_ccf
    d = _gold('lib_desi_r')
    lam, cc = d['lam'], _conf(d)
    flux = np.exp(d['dats'][:3])                       # float32, as the reference's
    logl = np.linspace(cc['logl0'], cc['logl1'], cc['npoints'])
    # preprocess_model_list == preprocess_model row by row; order: model, then vsini
    mods, par, vs = make_ccf.preprocess_model_list(lam, flux, d['vec'].T[:3], cc,
                                                   vsinis=[None, 150.], nthreads=4)
    assert mods.shape == (6, cc['npoints']) and vs == [None, 150.] * 3
    assert np.array_equal(par[::2], d['vec'].T[:3]) and np.array_equal(par[::2], par[1::2])
    one = make_ccf.preprocess_model(logl, lam, flux[1], vsini=150., ccfconf=cc)
    assert np.array_equal(one, mods[3])
    m1, _, v1 = make_ccf.preprocess_model_list(lam, flux[:1], d['vec'].T[:1], cc)
    assert v1 == [None] and np.array_equal(m1[0], mods[0])
    # get_continuum with preprocess_model's errors: model = m / max(cont, 1e-2 median)
    m = flux[0]
    es = np.maximum(m * 1e-5, 1e-2 * np.median(m))
    cont = make_ccf.get_continuum(lam, m, es, cc)
    assert cont.shape == m.shape and np.all(cont > 0)
    cfl = np.maximum(cont, 1e-2 * np.median(cont))
    want = np.interp(logl, np.log(lam), m / cfl, left=1., right=1.)
    assert np.max(np.abs(want - mods[0])) < 1e-9
    # a requested range wider than the row: 1 outside
    wide = dict(cc, logl0=np.log(lam[0]) - 0.01, logl1=np.log(lam[-1]) + 0.01)
    mw = make_ccf.preprocess_model(np.linspace(wide['logl0'], wide['logl1'], 1024), lam,
                                   flux[0], ccfconf=wide)
    lg = np.linspace(wide['logl0'], wide['logl1'], 1024)
    out = (lg < np.log(lam[0])) | (lg > np.log(lam[-1]))
    assert out.sum() > 10 and np.all(mw[out] == 1.0) and np.all(mw[~out] != 1.0)
    # a row with a non-positive median: flagged, nothing aborts, the others untouched
    rows = torch.as_tensor(flux.astype(np.float64)).to('cuda')
    rows[1] = -rows[1]
    r = make_ccf.models_build(lam, rows, cc, f32row=[1, 1, 1], details=True)
    st = r['status'].cpu().numpy()
    assert st[1] == _lib.ST_NONPOS_MEDIAN and st[0] == 0 and st[2] == 0
    # the flagged row starts from log(1e-3 |median|) in every bin (make_ccf.py:133-143)
    # and a continuum can only be pushed down from there: finite, not above the start
    med = abs(float(np.median(flux[1])))
    pf, ct = r['pfit'][1].cpu().numpy(), r['cont'][1].cpu().numpy()
    assert np.all(np.isfinite(pf)) and np.all(np.isfinite(ct))
    assert np.all(np.isfinite(r['model'][1].cpu().numpy()))
    assert np.all(ct <= 1e-3 * med * (1 + 1e-9))
    assert np.array_equal(r['model'][0].cpu().numpy(), mods[0])


@pytest.mark.parametrize('ntp', [9216, 4999])
def test_long_rows_and_forty_nodes(ntp):
    """ntp at the limit (and one not a multiple of 64), 40 continuum nodes: a smooth
    known continuum times lines comes back"""
    import torch
    from rvspecfit_amd import make_ccf
    step = 1000.
    lam = 4000 * np.exp(np.linspace(0, 39.5 * np.log(1 + step / 3e5), ntp))
    cc = dict(logl0=np.log(lam[50]), logl1=np.log(lam[-50]), npoints=8192,
              continuum=True, splinestep=step, maxcontpts=20)
    assert make_ccf.model_tables(lam, cc)['nnode'] == 40
    rng = np.random.default_rng(ntp)
    x = (lam - lam[0]) / (lam[-1] - lam[0])
    cont = np.exp(0.8 * np.sin(3 * x) + 0.5 * x)
    lines = 1 - 0.5 * np.exp(-0.5 * ((lam[None, :] - rng.uniform(lam[0], lam[-1], (25, 1)))
                                     / 0.25)**2).max(axis=0)
    rows = torch.as_tensor(np.stack([cont * lines, 2 * cont * lines])).to('cuda')
    r = make_ccf.models_build(lam, rows, cc, details=True)
    c = r['cont'].cpu().numpy()
    assert np.max(np.abs(c[0] / cont - 1)) < 2e-2
    # accuracy at 40 nodes: scipy's least_squares on the same objective (the spline as
    # a matrix in the node values), from the binned-median start, run to 1e-14
    import scipy.optimize
    import scipy.stats
    from rvspecfit_amd import ccf_tables
    nodes, edges = ccf_tables.continuum_nodes(lam, step)
    E = ccf_tables.interp_spline_design(nodes, lam)
    m = rows[0].cpu().numpy()
    e = np.maximum(m * 1e-5, 1e-2 * np.median(m))
    model = lambda p: np.exp(np.clip(E @ p, -100, 100))
    stat = scipy.stats.binned_statistic(lam, m, 'median', bins=edges).statistic
    p0 = np.log(np.maximum(stat, 1e-3 * np.median(m)))
    fit = scipy.optimize.least_squares(
        lambda p: (model(p) - m) / e, p0, jac=lambda p: (model(p) / e)[:, None] * E,
        loss='soft_l1', xtol=1e-14, ftol=1e-14, gtol=1e-14)
    err = np.max(np.abs(c[0] / model(fit.x) - 1))
    print('40 nodes, %d pixels: continuum against least_squares %.2e' % (ntp, err))
    assert err < 2e-5
    assert np.max(np.abs(c[1] / c[0] - 2)) < 1e-6
    assert np.all(np.isfinite(r['model'].cpu().numpy()))
    if ntp == 9216:      # one past the limit: an error before any launch
        with pytest.raises(ValueError):
            make_ccf.models_build(
                np.append(lam, lam[-1] * 1.0001),
                torch.ones((1, ntp + 1), dtype=torch.float64, device='cuda'), cc)


def test_t512_set_with_fitted_continuum_through_fit_batch():
    """a set of 534 templates (every 9th of a 7^4 grid x 2 vsini), its continuum
    FITTED, on a synthetic three-arm library; pipeline.fit_batch on 2000 spectra; the
    oracle's ccf_fit and chi^2 grid on a sample of 64; a subset of the batch gives the
    same records bit for bit"""
    import torch
    from oracle import rvs_oracle as orc
    from rvspecfit_amd import engine, make_ccf, pipeline, spec_inter, synth
    from rvspecfit_amd.library import TemplateLibrary
    arms = {'t5b': (3600., 5800.), 't5r': (5760., 7620.), 't5z': (7520., 9824.)}
    cfg = dict(CFG, template_lib='t512://')
    S = 2000
    rng = np.random.RandomState(3)
    teff, logg = rng.uniform(3800, 11000, S), rng.uniform(0.5, 4.5, S)
    feh, alpha = rng.uniform(-1.8, -0.2, S), rng.uniform(0.1, 0.9, S)
    vel, snr = rng.normal(0, 100, S), 10**rng.uniform(1.3, 2.3, S)
    olibs, obs, T = {}, [], None
    for a, (l0, l1) in arms.items():
        lib = synth.make_interp_library_fast(a, l0, l1, 0.8, resol=3000., device='cuda')
        d = synth.library_as_npz_dict(lib, None)
        tl = TemplateLibrary(a, d)
        npoints = make_ccf.to_power_two(int((l1 - l0) / 0.8))
        cc = make_ccf.get_ccf_config(np.log(l0), np.log(l1), npoints)
        s = make_ccf.build_ccf_set(tl, cc, every=9, vsinis=[0., 300.])
        T = len(s['ccf_vsinis'])
        assert T >= 512
        tl.add_ccf_set(s)
        spec_inter.register_library(tl, cfg['template_lib'])
        hd = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v)
              for k, v in d.items()}
        olibs[a] = orc.Library(dict(hd, **s))
        lam = np.arange(l0 + 40, l1 - 40, 1.6)
        sp0 = synth.spectra_batch(lam, teff, logg, feh, alpha, vel=vel,
                                  wresol=0.5 * (l0 + l1) / 3000. / 2.35)
        es = sp0 / snr[:, None]
        obs.append((a, lam, sp0 + es * rng.normal(size=sp0.shape), es))
    mk = lambda idx: engine.SpecBatch([engine.ArmData(a, lam, sp[idx], es[idx])
                                       for a, lam, sp, es in obs])
    rec = pipeline.fit_batch(mk(slice(None)), cfg, options=dict(npoly=10)).cpu().numpy()
    assert rec.shape[0] == S and np.all(rec[:, 0] >= 0) and np.all(rec[:, 0] < T)
    assert np.median(np.abs(rec[:, 7] - vel)) < 5.0
    idx = np.arange(0, S, S // 64)[:64]
    sub = pipeline.fit_batch(mk(idx), cfg, options=dict(npoly=10)).cpu().numpy()
    assert np.array_equal(sub, rec[idx], equal_nan=True)
    # the oracle on the same set: the CCF stage, then the chi^2 grid at its template
    vg = np.arange(cfg['min_vel'], cfg['max_vel'], cfg['vel_step0'])
    for i in idx:
        osd = [orc.SpecData(a, lam, sp[i], es[i]) for a, lam, sp, es in obs]
        o = orc.ccf_fit(osd, cfg, olibs)
        assert int(rec[i, 0]) == o['best_id'], (i, rec[i, 0], o['best_id'])
        assert abs(rec[i, 1] - o['best_vel']) < 0.01
        rot = None if np.isnan(o['best_vsini']) else (o['best_vsini'], )
        grid = orc.chisq_grid_fast(osd, vg, o['best_par'], rot, dict(npoly=10), cfg,
                                   olibs)
        g = orc.grid_summary(vg, grid[:, None])
        assert abs(rec[i, 7] - g['best_vel']) < 0.01, i
        assert abs(rec[i, 11] - g['best_chi']) <= 1e-6 * abs(g['best_chi']), i
