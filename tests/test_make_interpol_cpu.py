"""Host side of building template libraries from high-resolution models
(read_grid, make_interpol, make_nd): the output grid against the committed libraries'
`lam`, regular_library against their idgrid / uvecs, scan_grid on files written with
fits_min, Resolution, argument validation of the three entry points without a device,
and the truth of the GPU tests (tests/rebin_truth.py) against an analytic case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rebin_truth  # noqa: E402

from rvspecfit_amd import make_interpol, make_nd, read_grid, synth  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
# what tests/golden/make_golden*.py passed to rvs_make_interpol
TEMPL = dict(gold_b=(4380., 4740., 0.4), gold_r=(4680., 4960., 0.4),
             desi_b=(4255., 4600., 0.4), desi_r=(4495., 4840., 0.4),
             desi_z=(4735., 5080., 0.4), sdss1=(3750., 9300., 1.0))
GRID_KW = dict(nteff=4, nlogg=4, nfeh=4, nalpha=4, teff_range=(3500., 7500.),
               logg_range=(1., 4.), feh_range=(-2., 0.), alpha_range=(0., 0.4))
HOLES = (37, 207)


@pytest.mark.parametrize('name', sorted(TEMPL))
def test_output_grid_is_the_committed_lam(name):
    d = np.load(os.path.join(GOLD, 'lib_%s.npz' % name))
    l0, l1, st = TEMPL[name]
    lam = make_interpol.output_grid(l0, l1, st, True)
    assert lam.shape == d['lam'].shape
    assert np.max(np.abs(lam / d['lam'] - 1)) < 1e-15


def test_output_grid_linear_and_errors():
    lam = make_interpol.output_grid(5000., 5100., 0.5, False)
    fac = 1 + 1000. / 299792.458
    assert lam[0] == 5000. / fac and np.allclose(np.diff(lam), 0.5, rtol=0, atol=1e-9)
    assert lam[-1] < 5100.5 * fac <= lam[-1] + 0.5 + 1e-9
    with pytest.raises(RuntimeError, match='incorrectly specify'):
        make_interpol.output_grid(5000., 4000., 0.5, True)


def test_regular_library_on_a_grid_with_holes():
    d = np.load(os.path.join(GOLD, 'lib_gold_b.npz'))
    _, vec = synth.regular_grid(**GRID_KW)
    keep = np.ones(vec.shape[1], dtype=bool)
    keep[list(HOLES)] = False
    vec = vec[:, keep]
    n = vec.shape[1]
    specs = np.zeros((n, 3), dtype=np.float32)
    lib = make_nd.regular_library(dict(
        specs=specs, vec=vec, lam=np.arange(3.) + 1, parnames=synth.PARNAMES,
        mapper_args=((0, ), ), lognorms=np.zeros(n), log_step=True, log_spec=True))
    assert np.array_equal(lib['idgrid'], d['idgrid'])
    assert (lib['idgrid'] == -1).sum() == 2
    assert np.allclose(lib['vec'], d['vec'], rtol=1e-12, atol=0)
    for i in range(4):
        assert np.allclose(lib['uvec%d' % i], d['uvec%d' % i], rtol=1e-12, atol=1e-15)
    assert lib['dats'] is specs and bool(lib['log_step']) and list(lib['log_ids']) == [0]
    assert [str(_) for _ in lib['parnames']] == [str(_) for _ in d['parnames']]
    bad = vec.copy()
    bad[0, 0] = -1.
    with pytest.raises(RuntimeError, match='not finite'), np.errstate(all='ignore'):
        make_nd.regular_library(dict(specs=specs, vec=bad, lam=np.arange(3.),
                                     parnames=synth.PARNAMES, mapper_args=((0, ), ),
                                     lognorms=np.zeros(n), log_step=True))


def test_log_param_mapper():
    m = read_grid.LogParamMapper([0])
    v = np.array([[4000., 5000.], [1., 2.]])
    f = m.forward(v)
    assert np.array_equal(f[0], np.log10(v[0])) and np.array_equal(f[1], v[1])
    assert np.allclose(m.inverse(f), v, rtol=1e-14)
    assert v[0, 0] == 4000.


def _write(path, data, **cards):
    from rvspecfit_amd import fits_min
    h = fits_min.Header()
    for k, v in cards.items():
        h[k] = v
    fits_min.HDUList([fits_min.PrimaryHDU(np.asarray(data), h)]).writeto(path)


def test_scan_grid_orders_by_parameters(tmp_path):
    pre = str(tmp_path) + '/'
    os.makedirs(pre + 'specs')
    pars = [(5000., 2., -1., 0.4), (4000., 3., 0., 0.), (5000., 2., -1., 0.),
            (4000., 1., -2., 0.2), (5000., 1., 0., 0.)]
    for k, (t, g, f, a) in enumerate(pars):
        _write(pre + 'specs/m_%02d.fits' % k, np.full(6, float(k)), PHXTEFF=t, PHXLOGG=g,
               PHXM_H=f, PHXALPHA=a)
    g = read_grid.scan_grid(pre, 'specs/*.fits')
    want = sorted(range(5), key=lambda k: pars[k])
    assert list(g.file_ids) == want
    assert g.filenames == ['specs/m_%02d.fits' % k for k in want]
    assert np.array_equal(g.vec, np.array([pars[k] for k in want]).T)
    assert g.parnames == ('teff', 'logg', 'feh', 'alpha')
    chunks = list(g.read(chunk=2))
    assert [c.shape for c in chunks] == [(2, 6), (2, 6), (1, 6)]
    assert np.array_equal(np.concatenate(chunks)[:, 0], np.array(want, dtype=float))
    # another order of the names orders the rows by them
    g2 = read_grid.scan_grid(pre, 'specs/*.fits', parnames=['logg', 'teff', 'feh', 'alpha'])
    assert list(g2.file_ids) == sorted(range(5), key=lambda k: (pars[k][1], pars[k][0],
                                                               pars[k][2], pars[k][3]))
    _write(pre + 'specs/m_99.fits', np.zeros(6), PHXTEFF=1., PHXLOGG=1., PHXM_H=0.)
    with pytest.raises(Exception, match='Keyword for alpha PHXALPHA not found'):
        read_grid.scan_grid(pre, 'specs/*.fits')
    with pytest.raises(Exception, match='No FITS templates found'):
        read_grid.scan_grid(pre, 'nothing/*.fits')


def test_resolution():
    x = np.array([4000., 5000.])
    assert make_interpol.Resolution(resol=2000.)(x) == 2000.
    assert np.array_equal(make_interpol.Resolution(resol_func='1000+2*x')(x),
                          1000 + 2 * x)
    assert np.array_equal(make_interpol.Resolution(resol_func='np.sqrt(x)')(x),
                          np.sqrt(x))
    with pytest.raises(AssertionError):
        make_interpol.Resolution()
    # --fixed_fwhm: R grows with the wavelength so that lam / R stays what it is in
    # the middle of the range
    r = make_interpol.resolution_from_args(resol=2000., fixed_fwhm=True, lambda0=4000.,
                                           lambda1=5000.)
    assert np.allclose(x / r(x), 4500. / 2000., rtol=1e-6)
    sig = read_grid.rebinner_sigmas(x, make_interpol.Resolution(resol=2000.), 100000)
    assert np.allclose(sig, x * np.sqrt(2000.**-2 - 1e-10) / 2.3548200450309493)
    with pytest.raises(AssertionError):
        read_grid.rebinner_sigmas(x, make_interpol.Resolution(resol=2e5), 100000)


def test_build_specs_refuses_before_any_device_work():
    lam_hr = np.linspace(4000., 5000., 1001)
    vec = np.array([[5000.], [2.], [0.], [0.]])
    S = lambda a, b, r=2000.: ('x', a, b, make_interpol.Resolution(resol=r), 0.5, True)
    m = np.ones((1, 1001))
    with pytest.raises(ValueError, match='normalize must be one of'):
        make_interpol.build_specs(lam_hr, m, vec, S(4200., 4800.), normalize='mean')
    with pytest.raises(RuntimeError, match='does not cover'):
        make_interpol.build_specs(lam_hr, m, vec, S(3900., 4800.))
    with pytest.raises(RuntimeError, match='incorrectly specify'):
        make_interpol.build_specs(lam_hr, m, vec, S(4800., 4200.))
    with pytest.raises(AssertionError):
        make_interpol.build_specs(lam_hr, m, vec, S(4200., 4800., 2e5))
    with pytest.raises(ValueError, match='float_bits'):
        make_interpol.build_specs(lam_hr, m, vec, S(4200., 4800.), float_bits=16)
    with pytest.warns(DeprecationWarning), pytest.raises(RuntimeError):
        make_interpol.build_specs(lam_hr, m, vec, S(3900., 4800.), normalize=True)


def test_command_line_options():
    p = make_interpol.make_parser()
    a = p.parse_args(['--setup', 's', '--lambda0', '4000', '--lambda1', '5000', '--step',
                      '0.5', '--templprefix', 'x/', '--wavefile', 'w.fits', '--resol',
                      '2000', '--no-log', '--air', '--float_bits', '64', '--normalize',
                      'median', '--fixed_fwhm'])
    assert (a.log, a.air, a.float_bits, a.normalize, a.fixed_fwhm) == (
        False, True, 64, 'median', True)
    assert a.resolution0 == 100000 and a.log_parameters == '0'
    assert a.parameter_names == 'teff,logg,feh,alpha'
    with pytest.raises(SystemExit):
        make_interpol.main(['--setup', 's', '--lambda0', '4000', '--lambda1', '5000',
                            '--step', '0.5', '--templprefix', 'x/', '--wavefile', 'w'])


def test_entry_points_validate_without_a_device():
    from rvspecfit_amd import _lib
    L = _lib.lib()
    one = np.ones(8)
    p = one.ctypes.data
    ip = np.zeros(8, dtype=np.int32).ctypes.data
    assert L.rvs_rebin_weights(None, 10, p, p, ip, ip, 4, 4, p, None) == -1
    assert L.rvs_rebin_weights(p, 1, p, p, ip, ip, 4, 4, p, None) == -1
    assert L.rvs_rebin_weights(p, 8, p, p, ip, ip, 1, 4, p, None) == -1
    assert L.rvs_rebin_weights(p, 8, p, p, ip, ip, 70000, 4, p, None) == -1
    assert L.rvs_rebin_apply(None, 0, 8, 1, 8, p, p, 4, ip, ip, p, 4, 1, p, None) == -1
    assert L.rvs_rebin_apply(p, 0, 7, 1, 8, p, p, 4, ip, ip, p, 4, 1, p, None) == -1
    assert L.rvs_rebin_apply(p, 0, 8, 0, 8, p, p, 4, ip, ip, p, 4, 1, p, None) == -1
    assert L.rvs_rebin_apply(p, 0, 8, 1, 8, None, p, 4, ip, ip, p, 4, 1, p, None) == -1
    assert L.rvs_template_normalize(p, 1, 9217, p, 2, 1., 2., 1, 32, p, p, ip, None) == -1
    assert L.rvs_template_normalize(p, 1, 1, p, 2, 1., 2., 1, 32, p, p, ip, None) == -1
    assert L.rvs_template_normalize(p, 1, 8, p, 3, 1., 2., 1, 32, p, p, ip, None) == -1
    assert L.rvs_template_normalize(p, 1, 8, p, 2, 2., 2., 1, 32, p, p, ip, None) == -1
    assert L.rvs_template_normalize(p, 1, 8, p, 2, 1., 2., 1, 16, p, p, ip, None) == -1
    assert L.rvs_template_normalize(p, 0, 8, p, 0, 1., 2., 1, 64, p, p, ip, None) == -1
    assert make_interpol.MAX_NPIX == 9216


def test_truth_in_the_narrow_lsf_limit():
    """sigma = 1e-5 of the input step: the weights are the plain pixel averages of the
    linear interpolant (the kinks at the samples add s^2 / h)"""
    rng = np.random.default_rng(3)
    lam0 = np.cumsum(rng.uniform(0.8, 1.2, size=40)) + 5000.
    lam = np.array([5010.3, 5012.1, 5013.0, 5015.7, 5016.2])
    sigs = np.full(len(lam), 1e-5)
    # (the 5 sigma window of such an LSF does not span the pixel: give it the grid)
    left, right = np.zeros(5, dtype=int), np.full(5, len(lam0) - 2)
    got = np.zeros((len(lam0), len(lam)))
    for i in range(len(lam)):
        ls = 0.5 * (lam[i] - lam[i - 1]) if i else 0.5 * (lam[1] - lam[0])
        rs = 0.5 * (lam[i + 1] - lam[i]) if i < 4 else ls
        seg = np.arange(left[i], right[i] + 1)
        c1, c2 = rebin_truth.segment_coefficients(lam0[seg], lam0[seg + 1],
                                                  lam[i] - ls, lam[i] + rs, sigs[i])
        got[seg, i] += c1 / (ls + rs)
        got[seg + 1, i] += c2 / (ls + rs)
    want = rebin_truth.pixel_average_matrix(lam0, lam)
    assert np.max(np.abs(got - want)) < 1e-8
    assert np.allclose(got.sum(axis=0), 1, rtol=0, atol=1e-12)


@pytest.mark.parametrize('ratio', [0.02, 0.5, 3.0])
def test_closed_form_against_quadrature(ratio):
    """read_grid.pix_integrator (the numpy statement of the kernel's formulas) against
    the quadrature, from input steps far below the LSF width to above it"""
    s = 1.0
    lam0 = 5000. + np.arange(-400, 401) * ratio * s * (1 + 0.1 * np.sin(np.arange(801)))
    lam0 = np.sort(lam0)
    for l1, l2 in ((4999.7, 5000.4), (5003.1, 5003.3), (4990., 4990.9)):
        keep = (lam0[1:] > l1 - 6 * s) & (lam0[:-1] < l2 + 6 * s)
        x1, x2 = lam0[:-1][keep], lam0[1:][keep]
        c1, c2 = read_grid.pix_integrator(x1, x2, l1, l2, s)
        t1, t2 = rebin_truth.segment_coefficients(x1, x2, l1, l2, s)
        scale = (l2 - l1)
        assert np.max(np.abs(c1 - t1)) < 1e-12 * scale, ratio
        assert np.max(np.abs(c2 - t2)) < 1e-12 * scale, ratio


@pytest.mark.parametrize('ratio', [1.0001, 3.0, 17.0, 200.0])
def test_closed_form_with_long_segments(ratio):
    """segments much longer than sigma: edges deep inside a segment, across a sample
    and far outside -- all three polynomial branches of the closed form"""
    s = 0.7
    lam0 = 5000. + (np.arange(-6, 7) + 0.3) * ratio * s
    for l1, l2 in ((4999.7, 5000.4), (5000.1, 5000.3), (5000.2 - ratio, 5000.9 - ratio),
                   (4990., 5011.)):
        c1, c2 = read_grid.pix_integrator(lam0[:-1], lam0[1:], l1, l2, s)
        t1, t2 = rebin_truth.segment_coefficients(lam0[:-1], lam0[1:], l1, l2, s)
        assert np.max(np.abs(c1 - t1)) < 1e-12 * (l2 - l1), ratio
        assert np.max(np.abs(c2 - t2)) < 1e-12 * (l2 - l1), ratio


def _host_case(g, case, truth):
    """a case of interpol_cases.npz in numpy: the weights from the quadrature (truth)
    or from read_grid.pix_integrator, the normalisation with np.median"""
    o = rebin_truth.case_options(g[case + '/args'])
    lam_hr, rows, vec = rebin_truth.case_models(g)
    lam = make_interpol.output_grid(o['lambda0'], o['lambda1'], o['step'], o['log_step'])
    R = make_interpol.resolution_from_args(o['resol'], o['resol_func'], o['fixed_fwhm'],
                                           o['lambda0'], o['lambda1'])
    lam0 = read_grid.to_air(lam_hr) if o['air'] else lam_hr
    sigs = read_grid.rebinner_sigmas(lam, R, 100000)
    if truth:
        M = rebin_truth.rebin_matrix(lam0, lam, sigs)
    else:
        left, right, _ = read_grid.rebinner_windows(lam0, lam, sigs)
        M = np.zeros((len(lam0), len(lam)))
        for i in range(len(lam)):
            ls = 0.5 * (lam[i] - lam[i - 1]) if i else 0.5 * (lam[1] - lam[0])
            rs = 0.5 * (lam[i + 1] - lam[i]) if i < len(lam) - 1 else ls
            seg = np.arange(left[i], right[i] + 1)
            c1, c2 = read_grid.pix_integrator(lam0[seg], lam0[seg + 1], lam[i] - ls,
                                              lam[i] + rs, sigs[i])
            M[seg, i] += c1 / (ls + rs)
            M[seg + 1, i] += c2 / (ls + rs)
    # photons in (the wavelengths as given, not the air ones), per wavelength out
    return rebin_truth.normalize(((rows * lam_hr) @ M) / lam, lam, o['normalize'], True)


@pytest.mark.parametrize('case', ['f64', 'air_median_f64'])
def test_reference_float64_case_against_the_quadrature(case):
    """Where the reference's float64 output sits: 8.5e-12 from the quadrature (its
    weights are sums of sixteen cancelling terms), while the formulas the kernel uses
    are within 1e-13 of it.  This is why libraries are compared with the reference's at
    2e-11 and not at 1e-12."""
    g = dict(np.load(os.path.join(GOLD, 'interpol_cases.npz')))
    want, wl = _host_case(g, case, True)
    twin, tl = _host_case(g, case, False)
    ref, rl = g[case + '/dats'], g[case + '/lognorms']
    d_ref, d_twin = np.max(np.abs(ref - want)), np.max(np.abs(twin - want))
    print('%s: reference - quadrature %.2e, closed form - quadrature %.2e'
          % (case, d_ref, d_twin))
    assert d_twin < 1e-13 and np.max(np.abs(tl - wl)) < 1e-13
    assert 1e-12 < d_ref < 2e-11 and np.max(np.abs(rl - wl)) < 2e-11
    if case == 'air_median_f64':
        # the photon factor with the air wavelengths would sit 2.8e-4 away
        assert np.all(np.abs(rl - wl - np.log(1.00028)) > 1e-4)


def test_normalize_truth_is_np_median():
    lam = np.linspace(5000., 5100., 7)
    rows = np.array([[1., 2., 4., 3., 5., 9., 7.]])
    out, ln = rebin_truth.normalize(rows, lam, 'median', log_spec=False)
    assert np.array_equal(out, rows / 4.) and ln[0] == np.log(4.)
    out, ln = rebin_truth.normalize(rows, lam, 'linear_continuum', log_spec=False)
    # halves [1, 2, 4] at lam[1] and [3, 5, 9, 7] at (lam[4] + lam[5]) / 2
    x1, x2 = lam[1], 0.5 * (lam[4] + lam[5])
    cont = np.exp(np.log(2.) + (np.log(6.) - np.log(2.)) * (lam - x1) / (x2 - x1))
    assert np.allclose(out[0], rows[0] / cont, rtol=1e-15) and ln[0] == 0
    assert np.allclose(make_interpol.get_line_continuum(lam, rows[0]), cont, rtol=1e-14)
