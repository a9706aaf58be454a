"""Template libraries built on the device from high-resolution models
(make_interpol.build_specs, make_nd.regular_library, TemplateLibrary.from_models)
against the libraries the reference's rvs_make_interpol + rvs_make_nd made from the
same models (tests/golden/lib_*.npz), the kernels against tests/rebin_truth.py, and
through fitter_ccf.fit / vel_fit.process."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rebin_truth  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
GRID4 = dict(nteff=4, nlogg=4, nfeh=4, nalpha=4, teff_range=(3500., 7500.),
             logg_range=(1., 4.), feh_range=(-2., 0.), alpha_range=(0., 0.4))
GRID3 = dict(nteff=3, nlogg=3, nfeh=3, nalpha=3, teff_range=(4000., 7000.),
             logg_range=(1., 5.), feh_range=(-2., 0.), alpha_range=(0., 0.4))
HOLES = (37, 207)
# name -> (grid, holes, high-resolution wavelengths, --lambda0 --lambda1 --step): what
# tests/golden/make_golden.py, make_golden_desi.py and make_golden_sdss.py wrote and
# passed to rvs_make_interpol (--resol 2000, vacuum, log step, linear_continuum, 32 bit)
SETUPS = {
    'gold_b': (GRID4, HOLES, ('linspace', 4300, 5040, 37001), (4380., 4740., 0.4)),
    'gold_r': (GRID4, HOLES, ('linspace', 4300, 5040, 37001), (4680., 4960., 0.4)),
    'desi_b': (GRID4, HOLES, ('linspace', 4200, 5140, 47001), (4255., 4600., 0.4)),
    'desi_r': (GRID4, HOLES, ('linspace', 4200, 5140, 47001), (4495., 4840., 0.4)),
    'desi_z': (GRID4, HOLES, ('linspace', 4200, 5140, 47001), (4735., 5080., 0.4)),
    'sdss1': (GRID3, (), ('arange', 3700., 9400., 0.1), (3750., 9300., 1.0)),
}
_MODELS = {}


def _models(name):
    """the high-resolution rows the golden scripts wrote as FITS files, in the order of
    the parameters (synth.regular_grid's own), holes left out"""
    from rvspecfit_amd import synth
    grid, holes, lh, _ = SETUPS[name]
    key = (id(grid), holes, lh)
    if key not in _MODELS:
        lam_hr = getattr(np, lh[0])(*lh[1:])
        _, vec = synth.regular_grid(**grid)
        keep = [i for i in range(vec.shape[1]) if i not in holes]
        vec = vec[:, keep]
        rows = np.array([synth.spectrum(lam_hr, *vec[:, i]) for i in range(vec.shape[1])])
        _MODELS.clear()          # one grid of models at a time
        _MODELS[key] = (lam_hr, rows, vec)
    return _MODELS[key]


def _ordered(a):
    """float32 -> integers whose differences count representable values"""
    v = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(v < 0, -(v & 0x7fffffff), v)


@pytest.mark.parametrize('name', list(SETUPS))
def test_libraries_against_the_reference(name):
    """build_specs + regular_library against rvs_make_interpol + rvs_make_nd
    --regulargrid.  dats holds float32 LOGARITHMS of continuum-normalised flux, many of
    them within 1e-3 of zero, where a float32 ulp (1e-10 and less) is no larger than
    the float64 rounding of the reference's own weights.  How large that is the
    float64 cases of tests/golden/interpol_cases.npz show (test_options_against_the_
    reference; tests/test_make_interpol_cpu.py::test_reference_float64_case_against_
    the_quadrature): the reference's logarithms lie 8.5e-12 from the quadrature of
    tests/rebin_truth.py, this code's formulas 5e-15.  So: 2 ulp, or 2e-11 absolute."""
    from rvspecfit_amd import make_interpol, make_nd
    d = np.load(os.path.join(GOLD, 'lib_%s.npz' % name))
    lam_hr, rows, vec = _models(name)
    l0, l1, st = SETUPS[name][3]
    S = make_interpol.build_specs(
        lam_hr, rows, vec, (name, l0, l1, make_interpol.Resolution(resol=2000.), st, True))
    assert S['specs'].is_cuda and S['log_spec'] is True and np.all(S['lognorms'] == 0)
    lib = make_nd.regular_library(S)
    assert np.max(np.abs(lib['lam'] / d['lam'] - 1)) < 1e-15
    assert np.allclose(lib['vec'], d['vec'], rtol=1e-12, atol=0)
    assert np.array_equal(lib['idgrid'], d['idgrid'])
    for i in range(4):
        assert np.allclose(lib['uvec%d' % i], d['uvec%d' % i], rtol=1e-12, atol=1e-15)
    got = lib['dats'].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == d['dats'].shape
    ulp = np.abs(_ordered(got) - _ordered(d['dats']))
    dev = np.abs(got.astype(np.float64) - d['dats'].astype(np.float64))
    print('%s: %d x %d values, bit-equal %.6f, one ulp %.2e, more %d, max |diff| %.2e'
          % (name, got.shape[0], got.shape[1], np.mean(ulp == 0), np.mean(ulp == 1),
             int(np.sum(ulp > 1)), dev.max()))
    assert np.all((ulp <= 2) | (dev <= 2e-11))
    assert np.mean(ulp == 0) > 0.97


@pytest.mark.parametrize('case', ['air', 'resol_func', 'fixed_fwhm', 'median', 'none',
                                  'nolog', 'f64', 'air_median_f64'])
def test_options_against_the_reference(case):
    """the options the committed libraries do not use, against the reference's runs in
    tests/golden/interpol_cases.npz.  The float64 cases show at full precision where
    the reference sits: within 2e-11 of this code, not within 1e-12, because its weights
    are sums of cancelling terms (tests/test_make_interpol_cpu.py holds the same fixture
    against the quadrature of tests/rebin_truth.py: 8.5e-12 there, 5e-15 for this
    code's formulas).  air_median_f64 pins which wavelengths the photon factor takes:
    the air ones would move lognorms by 2.8e-4."""
    from rvspecfit_amd import make_interpol, make_nd
    g = dict(np.load(os.path.join(GOLD, 'interpol_cases.npz')))
    o = rebin_truth.case_options(g[case + '/args'])
    lam_hr, rows, vec = rebin_truth.case_models(g)
    R = make_interpol.resolution_from_args(o['resol'], o['resol_func'], o['fixed_fwhm'],
                                           o['lambda0'], o['lambda1'])
    S = make_interpol.build_specs(
        lam_hr, rows, vec, (case, o['lambda0'], o['lambda1'], R, o['step'], o['log_step']),
        air=o['air'], normalize=o['normalize'], float_bits=o['float_bits'])
    lib = make_nd.regular_library(S)
    want = g[case + '/dats']
    assert np.max(np.abs(lib['lam'] / g[case + '/lam'] - 1)) < 1e-15
    assert bool(lib['log_step']) == bool(g[case + '/log_step']) == o['log_step']
    assert np.allclose(lib['vec'], g[case + '/vec'], rtol=1e-12, atol=0)
    assert np.array_equal(lib['idgrid'], g[case + '/idgrid'])
    for i in range(4):
        assert np.allclose(lib['uvec%d' % i], g[case + '/uvec%d' % i], rtol=1e-12)
    dl = np.max(np.abs(lib['lognorms'] - g[case + '/lognorms']))
    assert dl < 2e-11
    assert (o['normalize'] == 'median') == bool(np.any(g[case + '/lognorms'] != 0))
    got = lib['dats'].cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape
    dev = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if o['float_bits'] == 64:
        print('%s: float64, max |diff| %.2e, lognorms %.2e' % (case, dev.max(), dl))
        assert dev.max() < 2e-11
    else:
        ulp = np.abs(_ordered(got) - _ordered(want))
        print('%s: bit-equal %.6f, one ulp %.2e, more %d, max |diff| %.2e, lognorms %.2e'
              % (case, np.mean(ulp == 0), np.mean(ulp == 1), int(np.sum(ulp > 1)),
                 dev.max(), dl))
        assert np.all((ulp <= 2) | (dev <= 2e-11))
        assert np.mean(ulp == 0) > 0.97


def _weights_case(kind):
    from rvspecfit_amd import make_interpol
    R = make_interpol.Resolution(resol=2000.)
    lam0 = np.linspace(4988., 5032., 4401)
    lam = np.exp(np.arange(np.log(5000.), np.log(5020.), 8e-5))
    toair, warn = False, False
    if kind == 'resol_func':
        R = make_interpol.Resolution(resol_func='1500+0.2*x')
    elif kind == 'fixed_fwhm':
        R = make_interpol.resolution_from_args(resol=2000., fixed_fwhm=True,
                                               lambda0=5000., lambda1=5020.)
    elif kind == 'air':
        toair = True
        lam0 = lam0 + 1.4
    elif kind == 'linear':
        lam = np.arange(5000., 5020., 0.37)
    elif kind == 'two_steps':
        lam0 = np.concatenate([np.arange(4988., 5010., 0.006),
                               np.arange(5010., 5032., 0.012)])
    elif kind == 'narrow':
        lam0 = np.linspace(4999.5, 5032., 3251)
        warn = True
    elif kind == 'coarse':      # input step above sigma: the closed form
        lam0 = np.linspace(4988., 5032., 23)
    elif kind == 'very_coarse':  # segments of 6 to 40 sigma: pixels deep inside one,
        # across a sample, and segments wholly on one side of both edges
        lam0 = np.array([4900., 4960., 4993., 5003.5, 5010.2, 5017., 5060., 5100.])
    return lam0, lam, R, toair, warn


@pytest.mark.parametrize('kind', ['constant', 'resol_func', 'fixed_fwhm', 'air', 'linear',
                                  'two_steps', 'narrow', 'coarse', 'very_coarse'])
def test_weights_against_the_truth(kind):
    from rvspecfit_amd import read_grid
    lam0, lam, R, toair, warn = _weights_case(kind)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        mat = read_grid.make_rebinner(lam0, lam, R, resolution0=100000, toair=toair)
    assert any('not wide enough' in str(w.message) for w in rec) == warn
    got = mat.toarray()
    assert got.shape == (len(lam0), len(lam))
    lam0a = read_grid.to_air(lam0) if toair else lam0
    sigs = read_grid.rebinner_sigmas(lam, R, 100000)
    want = rebin_truth.rebin_matrix(lam0a, lam, sigs)
    sums = want.sum(axis=0)
    err = np.max(np.abs(got - want) / sums[None, :])
    print('%s: windows of %d .. %d input pixels, max deviation %.2e of the row sum'
          % (kind, int((want != 0).sum(axis=0).min()), int((want != 0).sum(axis=0).max()),
             err))
    assert err < 1e-12
    if not warn:
        assert np.max(np.abs(got.sum(axis=0) - 1)) < 1e-5
    else:
        assert got.sum(axis=0)[0] < 0.9 and abs(got.sum(axis=0)[-1] - 1) < 1e-5


def test_resolution_not_below_the_input_is_refused():
    from rvspecfit_amd import make_interpol, read_grid
    with pytest.raises(AssertionError):
        read_grid.make_rebinner(np.linspace(4990., 5030., 400), np.linspace(5000., 5020., 9),
                                make_interpol.Resolution(resol=3e5), resolution0=100000)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('T', [1, 7, 300])
def test_apply_against_numpy(dtype, T):
    import torch
    from rvspecfit_amd import make_interpol, read_grid
    lam0 = np.concatenate([np.arange(4980., 5010., 0.01), np.arange(5010., 5045., 0.02)])
    lam = np.exp(np.arange(np.log(4990.), np.log(5035.), 8e-5))     # 113 pixels
    mat = read_grid.make_rebinner(lam0, lam, make_interpol.Resolution(resol=2000.),
                                  resolution0=100000, toair=False)
    rng = np.random.default_rng(T)
    rows = (1 + 0.5 * rng.normal(size=(T, len(lam0)))).astype(dtype)
    M = mat.toarray()
    want = rows.astype(np.float64) @ M
    scale = np.abs(rows.astype(np.float64)) @ np.abs(M)
    d_rows = torch.as_tensor(rows).to('cuda')
    got = read_grid.apply_rebinner(mat, d_rows)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (T, len(lam))
    assert np.max(np.abs(got.cpu().numpy() - want) / scale) < 1e-13
    # the same bits however the models are split into calls
    parts = torch.cat([read_grid.apply_rebinner(mat, d_rows[a:a + 37])
                       for a in range(0, T, 37)])
    assert torch.equal(parts, got)
    # numpy in, numpy out; one spectrum in, one out
    one = read_grid.apply_rebinner(mat, rows[0])
    assert isinstance(one, np.ndarray) and one.shape == (len(lam), )
    assert np.array_equal(one, got[0].cpu().numpy())
    # photons in, per wavelength out: the form build_specs uses
    assert mat.lam_phot is mat.lam0        # no air conversion: one wavelength vector
    ph = read_grid.apply_band(mat, d_rows[:, mat.col0:mat.col1], True).cpu().numpy()
    want = ((rows.astype(np.float64) * lam0[None, :]) @ M) / lam[None, :]
    assert np.max(np.abs(ph - want) / (scale * lam0.max() / lam.min())) < 1e-13


@pytest.mark.parametrize('npix', [2, 3, 100, 101, 4097, 9216])
@pytest.mark.parametrize('mode', ['linear_continuum', 'median', 'none'])
def test_normalize_against_np_median(npix, mode):
    import torch
    from rvspecfit_amd import make_interpol
    rng = np.random.default_rng(npix)
    lam = np.exp(np.linspace(np.log(4000.), np.log(5000.), npix))
    rows = np.exp(0.3 * rng.normal(size=(5, npix))) * np.linspace(1, 3, npix)[None, :]
    rows[1, :npix // 2] = rows[1, 0]          # ties around the median
    d_rows = torch.as_tensor(rows).to('cuda')
    for log_spec in (True, False):
        want, wl = rebin_truth.normalize(rows, lam, mode, log_spec)
        for bits in (32, 64):
            got, ln, st = make_interpol.normalize_rows(d_rows, lam, mode, log_spec, bits)
            assert got.dtype == (torch.float32 if bits == 32 else torch.float64)
            assert not st.any()
            assert np.allclose(ln.cpu().numpy(), wl, rtol=0, atol=1e-15)
            g = got.cpu().numpy()
            if bits == 64:
                assert np.max(np.abs(g - want)) < 1e-13 * max(1, np.abs(want).max())
            else:
                assert np.allclose(g, want.astype(np.float32), rtol=2.5e-7, atol=1e-12)
    if mode == 'median':
        assert np.allclose(ln.cpu().numpy(), np.log(np.median(rows, axis=1)), rtol=0,
                           atol=1e-15)


def test_rows_beyond_the_limit_are_refused():
    import torch
    from rvspecfit_amd import make_interpol
    with pytest.raises(ValueError, match='9216'):
        make_interpol.normalize_rows(torch.ones((1, 9217), dtype=torch.float64,
                                                device='cuda'), np.arange(9217.) + 1)


@pytest.mark.parametrize('bad', [0.0, -1.0, np.nan])
def test_non_finite_spectrum_names_the_parameters(bad):
    from rvspecfit_amd import make_interpol
    lam_hr = np.linspace(4900., 5100., 20001)
    rows = 1 + 0.1 * np.sin(lam_hr / 3.)[None, :] * np.ones((3, 1))
    rows[1, 9000:11000] = bad
    vec = np.array([[4000., 5000., 6000.], [1., 2., 3.], [0., -1., -2.], [0., 0.2, 0.4]])
    S = ('t', 4950., 5050., make_interpol.Resolution(resol=2000.), 0.5, True)
    with pytest.raises(RuntimeError) as e:
        make_interpol.build_specs(lam_hr, rows, vec, S)
    msg = str(e.value)
    assert msg.startswith('The spectrum is not finite (has nans or infs) at parameter')
    assert "'teff'" in msg and '5000.0' in msg and "'alpha'" in msg and '0.2' in msg
    rows[1] = rows[0]
    out = make_interpol.build_specs(lam_hr, rows, vec, S, normalize='median',
                                    float_bits=64)
    assert out['specs'].dtype.itemsize == 8 and out['lognorms'].shape == (3, )
    assert np.allclose(out['lognorms'], 0, atol=0.11) and np.all(out['lognorms'] != 0)


def test_models_as_chunks_and_device_tensors_give_the_same_rows():
    import torch
    from rvspecfit_amd import make_interpol
    lam_hr = np.linspace(4900., 5100., 20001)
    rng = np.random.default_rng(8)
    rows = 1 + 0.1 * rng.uniform(size=(70, len(lam_hr)))
    vec = np.array([np.linspace(4000., 6000., 70), np.zeros(70), np.zeros(70),
                    np.zeros(70)])
    S = ('t', 4950., 5050., make_interpol.Resolution(resol=2000.), 0.5, False)
    a = make_interpol.build_specs(lam_hr, rows, vec, S)
    b = make_interpol.build_specs(lam_hr, torch.as_tensor(rows).to('cuda'), vec, S,
                                  chunk=33)
    c = make_interpol.build_specs(lam_hr, (rows[i:i + 9] for i in range(0, 70, 9)), vec, S)
    assert torch.equal(a['specs'], b['specs']) and torch.equal(a['specs'], c['specs'])
    assert a['log_step'] is False and np.allclose(np.diff(a['lam']), 0.5)
    f = make_interpol.build_specs(lam_hr, rows.astype(np.float32), vec, S)
    assert np.allclose(f['specs'].cpu().numpy(), a['specs'].cpu().numpy(), atol=1e-6)
    with pytest.raises(ValueError, match='rows'):
        make_interpol.build_specs(lam_hr, rows[:69], vec, S)


def _conf(d):
    return dict(logl0=float(d['ccf_logl0']), logl1=float(d['ccf_logl1']),
                npoints=int(d['ccf_npoints']), continuum=True,
                maxcontpts=int(d['ccf_maxcontpts']),
                splinestep=float(d['ccf_splinestep']))


def test_from_models_through_ccf_fit_and_process():
    """libraries made in one call from model spectra, CCF sets included, in place of
    the committed ones: the golden case c1 through fitter_ccf.fit and vel_fit.process,
    at the tolerances the golden tests ask of the committed libraries"""
    from conftest import GOLD_CONFIG, gold_specdata
    from rvspecfit_amd import fitter_ccf, make_interpol, spec_fit, spec_inter, vel_fit
    from rvspecfit_amd.library import TemplateLibrary
    root = 'from-models://'
    for n in ('gold_b', 'gold_r'):
        d = np.load(os.path.join(GOLD, 'lib_%s.npz' % n))
        lam_hr, rows, vec = _models(n)
        l0, l1, st = SETUPS[n][3]
        lib = TemplateLibrary.from_models(
            n, lam_hr, rows, vec, (n, l0, l1, make_interpol.Resolution(resol=2000.), st,
                                   True),
            ccf=dict(ccfconf=_conf(d), every=20, vsinis=[0., 100.]))
        assert lib.kind == 'regulargrid' and lib.ccf is not None
        assert lib.ccf['T'] == d['ccf_fft'].shape[0]
        spec_inter.register_library(lib, root)
    cfg = dict(GOLD_CONFIG, template_lib=root)
    cases = dict(np.load(os.path.join(GOLD, 'cases.npz')))
    g = dict(np.load(os.path.join(GOLD, 'process_cases.npz')))
    sds = gold_specdata(cases, 'c1', spec_fit.SpecData)
    r = fitter_ccf.fit(sds, cfg)
    np.testing.assert_allclose([r['best_par'][k] for k in ('teff', 'logg', 'feh', 'alpha')],
                               cases['c1/ccf/best_par'])
    assert abs(r['best_vel'] - cases['c1/ccf/best_vel']) < 0.01
    want = cases['c1/ccf/best_ccf']
    assert np.max(np.abs(r['best_ccf'] - want)) < 2e-5 * np.max(np.abs(want))
    assert r['best_vsini'] == float(cases['c1/ccf/best_vsini'])
    ts = [t for t in ('p0', 'p1', 'p2', 'p3') if str(g[t + '/case']) == 'c1']
    assert ts
    for t in ts:
        pd0 = dict(zip([str(_) for _ in g[t + '/start_keys']],
                       [float(_) for _ in g[t + '/start_vals']]))
        fix = [str(_) for _ in g[t + '/fix']]
        pri = None
        if t + '/prior_keys' in g:
            pri = {str(k): tuple(v) for k, v in zip(g[t + '/prior_keys'],
                                                    g[t + '/prior_vals'])}
        c2 = dict(cfg, second_minimizer=False)
        res = vel_fit.process(sds, pd0, fixParam=fix, options=dict(npoly=10), config=c2,
                              priors=pri)
        assert abs(res['vel'] - g[t + '/vel']) < 0.01
        assert abs(res['chisq'] / g[t + '/chisq'] - 1) < 1e-6
        assert abs(res['chisq'] - g[t + '/chisq']) < 2e-3


def test_synthetic_library_through_the_convolution():
    """synth.make_interp_library_convolved: a library of the generator's spectra made
    by the new path is a library TemplateLibrary takes, close to the analytic-width one
    (same model, the LSF applied to the lines' widths instead)"""
    from rvspecfit_amd import synth
    from rvspecfit_amd.library import TemplateLibrary
    kw = dict(nteff=3, nlogg=2, nfeh=2, nalpha=2)
    a = synth.make_interp_library_convolved('cv', 4500., 4600., 0.4, grid_kw=kw)
    b = synth.make_interp_library('cv', 4500., 4600., 0.4, grid_kw=kw, resol=2000.)
    assert a['dats'].is_cuda and tuple(a['dats'].shape) == b['dats'].shape
    assert np.array_equal(a['idgrid'], b['idgrid']) and np.allclose(a['vec'], b['vec'])
    assert np.max(np.abs(a['lam'] / b['lam'] - 1)) < 1e-15
    lib = TemplateLibrary('cv', synth.library_as_npz_dict(a))
    assert lib.ntp == len(b['lam']) and lib.ngrid == 24
    # the analytic library keeps the continuum; take its line through the halves out
    got = a['dats'].cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)) and np.abs(np.median(got, axis=1)).max() < 0.05
    assert got.min() < -0.05          # there are lines


def test_command_line_writes_a_library(tmp_path):
    """python -m rvspecfit_amd.make_interpol on a directory of FITS models: the same
    rows as build_specs on the arrays, in a file TemplateLibrary.from_npz reads"""
    from rvspecfit_amd import fits_min, make_interpol, synth
    from rvspecfit_amd.library import TemplateLibrary
    pre = str(tmp_path) + '/'
    os.makedirs(pre + 'specs')
    lam_hr = np.linspace(4400., 4700., 15001)
    _, vec = synth.regular_grid(nteff=2, nlogg=2, nfeh=2, nalpha=2)
    order = np.random.default_rng(4).permutation(vec.shape[1])   # files in any order
    rows = np.array([synth.spectrum(lam_hr, *vec[:, i]) for i in range(vec.shape[1])])
    for k, i in enumerate(order):
        h = fits_min.Header()
        for key, v in zip(('PHXTEFF', 'PHXLOGG', 'PHXM_H', 'PHXALPHA'), vec[:, i]):
            h[key] = float(v)
        fits_min.HDUList([fits_min.PrimaryHDU(rows[i].astype(np.float32), h)]).writeto(
            pre + 'specs/m%03d.fits' % k)
    fits_min.HDUList([fits_min.PrimaryHDU(lam_hr)]).writeto(pre + 'wave.fits')
    fname = make_interpol.main([
        '--setup', 'cl', '--lambda0', '4500', '--lambda1', '4600', '--step', '0.4',
        '--resol', '2000', '--templprefix', pre, '--mask', 'specs/*.fits', '--wavefile',
        pre + 'wave.fits', '--oprefix', pre + 'out', '--air'])
    assert fname == os.path.join(pre + 'out', 'lib_cl.npz')
    lib = TemplateLibrary.from_npz('cl', fname)
    assert lib.ngrid == 16 and lib.kind == 'regulargrid' and lib.log_step
    S = make_interpol.build_specs(
        lam_hr, rows.astype(np.float32), vec,
        ('cl', 4500., 4600., make_interpol.Resolution(resol=2000.), 0.4, True), air=True)
    import torch
    assert torch.equal(lib.dats, S['specs'])
    assert np.array_equal(lib.lam, S['lam'])


def test_rebin_one_spectrum():
    """read_grid.rebin: make_rebinner + apply_rebinner in one call, the resolution a
    function or a number, the input's resolution an argument"""
    from rvspecfit_amd import read_grid
    lam0 = np.linspace(4980., 5040., 6001)
    spec = 1 + 0.2 * np.sin(lam0 / 1.7)
    newlam = np.linspace(5000., 5020., 41)
    a = read_grid.rebin(lam0, spec, newlam, 2000., toair=False)
    mat = read_grid.make_rebinner(lam0, newlam, lambda x: 2000., resolution0=100000,
                                  toair=False)
    assert a.shape == (41, ) and np.array_equal(a, read_grid.apply_rebinner(mat, spec))
    assert np.allclose(a, spec @ rebin_truth.rebin_matrix(
        lam0, newlam, read_grid.rebinner_sigmas(newlam, lambda x: 2000., 100000)),
        rtol=1e-13)
    b = read_grid.rebin(lam0 + 1.4, spec, newlam, lambda x: 2000. + 0 * x)
    assert np.allclose(a, b, rtol=1e-3) and not np.array_equal(a, b)   # air by default
    with pytest.raises(AssertionError):
        read_grid.rebin(lam0, spec, newlam, 2000., resolution0=1500.)
