"""The reference's make_interpol under its names: high-resolution model spectra ->
the rows of a template library (convolved to the arm's LSF, integrated over the output
pixels, divided by a continuum, logged), on the device.

build_specs is process_all's body (make_interpol.py:237-389) without its files: it
returns the dictionary specs_<setup>.h5 holds.  make_nd.regular_library turns that into
a library; TemplateLibrary.from_models does both.
"""
import argparse
import sys
import warnings

import numpy as np
import torch

from . import _lib, read_grid

SPEED_OF_LIGHT = 299792.458     # scipy.constants.speed_of_light / 1e3
MAX_NPIX = 9216                 # RVS_REBIN_MAX_NPIX
NORM_MODES = {'none': 0, 'median': 1, 'linear_continuum': 2}


class Resolution:
    """The resolving power R = lambda / FWHM as a function of wavelength, under the
    reference's name and attributes (make_interpol.py:175-190): either the constant
    `resol`, which wins when both are given, or `resol_func`, an expression in the
    wavelength array `x` (numpy is available to it as `np`)."""

    def __init__(self, resol=None, resol_func=None):
        assert resol is not None or resol_func is not None
        self.resol, self.resol_func = resol, resol_func

    def __call__(self, x):
        if self.resol is not None:
            return self.resol
        return eval(self.resol_func, {'x': x, 'np': np})


def resolution_from_args(resol=None, resol_func=None, fixed_fwhm=False, lambda0=None,
                         lambda1=None):
    """the Resolution main builds from --resol / --resol_func / --fixed_fwhm
    (make_interpol.py:546-554)"""
    if resol is not None:
        if fixed_fwhm:
            lam_mid = (lambda0 + lambda1) * .5
            return Resolution(resol_func='x/%f*%f' % (lam_mid, resol))
        return Resolution(resol=resol)
    return Resolution(resol_func=resol_func)


def half_medians(lam):
    """the two wavelengths get_line_continuum anchors its line at"""
    npix2 = len(lam) // 2
    return float(np.median(lam[:npix2])), float(np.median(lam[npix2:]))


def get_line_continuum(lam, spec):
    """The linear-in-log continuum of make_interpol.py:47-75 for one spectrum on the
    host (numpy): the line through the medians of the two halves, extrapolated, in the
    degree-one B-spline's form.  rvs_template_normalize does this per row."""
    lam = np.asarray(lam, dtype=np.float64)
    spec = np.asarray(spec, dtype=np.float64)
    npix2 = len(lam) // 2
    lam1, lam2 = half_medians(lam)
    y1, y2 = np.log(np.median(spec[:npix2])), np.log(np.median(spec[npix2:]))
    f = 1.0 / (lam2 - lam1)
    return np.exp(y1 * (f * (lam2 - lam)) + y2 * (f * (lam - lam1)))


def _check_normalize(normalize):
    """the mode's name; True / False are still taken (with the reference's warning) as
    'linear_continuum' / 'none', anything else raises its ValueError"""
    if normalize is True or normalize is False:
        warnings.warn('Passing a boolean for normalize is deprecated. '
                      "Use 'linear_continuum', 'median', or 'none' instead.",
                      DeprecationWarning, stacklevel=3)
        return 'linear_continuum' if normalize else 'none'
    if normalize in NORM_MODES:
        return normalize
    raise ValueError('normalize must be one of %r, got %r'
                     % (('none', 'median', 'linear_continuum'), normalize))


def normalize_rows(rows, lam, normalize='linear_continuum', log_spec=True,
                   float_bits=32, out=None, lognorms=None, status=None, lam_dev=None):
    """extract_spectrum's steps after the rebin (make_interpol.py:156-172) on rows
    [T, npix] (float64 device tensor): (specs [T, npix] float32 / float64, lognorms [T],
    status int32 [T]; bit RVS_ST_NONFINITE where the reference raises), on the device.
    out / lognorms / status: buffers to fill (rows of larger arrays); lam_dev: `lam`
    where it is on the device already -- a loop over chunks then uploads nothing."""
    normalize = _check_normalize(normalize)
    _lib.require_gpu()
    T, npix = rows.shape
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    rows = rows.to(torch.float64).contiguous()
    dev = rows.device
    if out is None:
        out = torch.empty((T, npix), device=dev,
                          dtype=torch.float32 if float_bits == 32 else torch.float64)
    if lognorms is None:
        lognorms = torch.empty(T, dtype=torch.float64, device=dev)
    if status is None:
        status = torch.empty(T, dtype=torch.int32, device=dev)
    lam1, lam2 = half_medians(lam) if npix >= 2 else (0., 1.)
    d_lam = torch.as_tensor(lam).to(dev) if lam_dev is None else lam_dev
    rc = _lib.lib().rvs_template_normalize(
        _lib.ptr(rows), T, npix, _lib.ptr(d_lam), NORM_MODES[normalize], lam1, lam2,
        int(bool(log_spec)), int(float_bits), _lib.ptr(out), _lib.ptr(lognorms),
        _lib.ptr(status), _lib.stream())
    if rc == -1:
        raise ValueError('rvs_template_normalize: bad argument (rows of %d pixels, at '
                         'most %d; float_bits %s)' % (npix, MAX_NPIX, float_bits))
    _lib.check(rc, 'rvs_template_normalize')
    return out, lognorms, status


def output_grid(lamleft, lamright, step, log_step):
    """the library's wavelength grid (make_interpol.py:313-329): 1000 km/s of padding
    on both sides; the logarithmic step is the one that equals `step` in the middle of
    the range"""
    deltav = 1000.
    fac1 = (1 + deltav / SPEED_OF_LIGHT)
    if not log_step:
        lamgrid = np.arange(lamleft / fac1, (lamright + step) * fac1, step)
    else:
        log_step_val = np.log(1 + step / (0.5 * (lamleft + lamright)))
        lamgrid = np.exp(
            np.arange(np.log(lamleft / fac1), np.log(lamright * fac1), log_step_val))
    if len(lamgrid) <= 1:
        raise RuntimeError(
            'Did you incorrectly specify wavelength range or step ? ')
    return lamgrid


def _chunks(models, chunk):
    if isinstance(models, (np.ndarray, torch.Tensor)):
        if models.ndim != 2:
            raise ValueError('models: [T, len(lam_hr)] expected')
        for a in range(0, models.shape[0], chunk):
            yield models[a:a + chunk]
    else:
        for m in models:
            yield m if m.ndim == 2 else m[None, :]


def build_specs(lam_hr, models, vec, setupInfo, parnames=('teff', 'logg', 'feh', 'alpha'),
                air=False, resolution0=100000, normalize='linear_continuum',
                float_bits=32, log_parameters=(0, ), chunk=256, device='cuda'):
    """process_all (make_interpol.py:237-389) on the device.
    lam_hr [N]: the models' wavelengths; models: [T, N] host array or device tensor
    (float32 or float64), or an iterable of such chunks in row order (a grid larger than
    the device memory streams through: only the columns the windows use are uploaded);
    vec [npar, T]: the models' parameters, physical units;
    setupInfo = (setup, lambda0, lambda1, resolution function, step, log_step).
    Returns the contents of specs_<setup>.h5: specs (a DEVICE tensor [T, npix], float32
    or float64), vec, lam, parnames, lognorms, log_step, log_spec, mapper_*."""
    normalize = _check_normalize(normalize)
    if float_bits not in (32, 64):
        raise ValueError('float_bits must be 32 or 64')
    lam_hr = np.asarray(lam_hr, dtype=np.float64)
    vec = np.asarray(vec, dtype=np.float64)
    nspec = vec.shape[1]
    log_spec = True
    HR, lamleft, lamright, resol_function, step, log_step = setupInfo
    if lam_hr.min() > lamleft or lam_hr.max() < lamright:
        raise RuntimeError(f'''Cannot generate the spectra as the wavelength
        range in the library does not cover the requested wavelengths
        {lamleft} {lamright} {lam_hr.min()} {lam_hr.max()}
        ''')
    lamgrid = output_grid(lamleft, lamright, step, log_step)
    if len(lamgrid) > MAX_NPIX:
        raise ValueError('a library grid of %d pixels; at most %d' % (len(lamgrid),
                                                                     MAX_NPIX))
    mat = read_grid.make_rebinner(lam_hr, lamgrid, resol_function, toair=air,
                                  resolution0=resolution0, device=device)
    specs = torch.empty((nspec, len(lamgrid)), device=device,
                        dtype=torch.float32 if float_bits == 32 else torch.float64)
    lognorms = torch.zeros(nspec, dtype=torch.float64, device=device)
    status = torch.zeros(nspec, dtype=torch.int32, device=device)
    done = 0
    for m in _chunks(models, chunk):
        n = m.shape[0]
        if m.shape[1] != len(lam_hr) or done + n > nspec:
            raise ValueError('models: rows of %d pixels (%d expected), %d rows for %d '
                             'parameter vectors' % (m.shape[1], len(lam_hr), done + n,
                                                    nspec))
        m = m[:, mat.col0:mat.col1]
        if not isinstance(m, torch.Tensor):
            if m.dtype != np.float32:
                m = np.asarray(m, dtype=np.float64)
            m = torch.as_tensor(np.ascontiguousarray(m))
        rows = read_grid.apply_band(mat, m.to(device), True)
        normalize_rows(rows, lamgrid, normalize, log_spec, float_bits,
                       out=specs[done:done + n], lognorms=lognorms[done:done + n],
                       status=status[done:done + n], lam_dev=mat.lam)
        done += n
    if done != nspec:
        raise ValueError('models: %d rows for %d parameter vectors' % (done, nspec))
    bad = np.nonzero(status.cpu().numpy() & _lib.ST_NONFINITE)[0]
    if len(bad):
        param = dict(zip(parnames, vec.T[bad[0]]))
        raise RuntimeError('The spectrum is not finite (has nans or infs) at '
                           'parameter values: %s' % str(param))
    return dict(specs=specs, vec=vec, lam=lamgrid, parnames=tuple(parnames),
                mapper_module='rvspecfit.read_grid', mapper_class_name='LogParamMapper',
                mapper_args=(tuple(log_parameters or ()), ),
                lognorms=lognorms.cpu().numpy(), log_step=bool(log_step),
                log_spec=log_spec)


def add_bool_arg(parser, name, default=False, help=None):
    """the switch pair --NAME / --no-NAME, of which at most one may be given"""
    pair = parser.add_mutually_exclusive_group()
    for flag, value in (('--' + name, True), ('--no-' + name, False)):
        pair.add_argument(flag, dest=name, action='store_const', const=value,
                          default=default,
                          help=help if value else 'Invert the ' + name + ' option')


def make_parser():
    """the reference's options (make_interpol.py:412-527); the sqlite catalogue
    (--templdb) is replaced by a file mask and the header keywords"""
    p = argparse.ArgumentParser(
        description='Create interpolated and convolved spectra from the input grid.')
    p.add_argument('--setup', type=str, required=True,
                   help='Name of the spectral configuration')
    p.add_argument('--lambda0', type=float, required=True,
                   help='Start wavelength of the new grid')
    p.add_argument('--lambda1', type=float, required=True,
                   help='End wavelength of the new grid')
    p.add_argument('--resol', type=float,
                   help='Constant spectral resolution of the new grid')
    p.add_argument('--float_bits', type=int, default=32, choices=[32, 64],
                   help='Cast spectra to 32 or 64 bits')
    p.add_argument('--revision', type=str, default='',
                   help='The revision of the templates')
    p.add_argument('--parameter_names', type=str, default='teff,logg,feh,alpha',
                   help='comma separated list of parameters to make the interpolator')
    p.add_argument('--log_parameters', type=str, default='0',
                   help='Which parameters we are taking the log() of when interpolating')
    p.add_argument('--resol_func', type=str,
                   help='Spectral resolution function of the new grid, a function of '
                   'the wavelength x in angstrom, i.e. 1000+2*x')
    p.add_argument('--step', type=float, required=True,
                   help='Pixel size in angstrom of the templates in the grid')
    add_bool_arg(p, 'log', default=True,
                 help='Generate the spectra in log-wavelength scale')
    p.add_argument('--normalize', type=str, default='linear_continuum',
                   choices=['none', 'median', 'linear_continuum'],
                   help='Normalization mode for spectra')
    p.add_argument('--no-normalize', dest='_no_normalize', action='store_true',
                   default=False, help=argparse.SUPPRESS)
    p.add_argument('--templprefix', type=str, required=True,
                   help='The path to the templates')
    p.add_argument('--mask', type=str, default='*/*fits',
                   help='Which files under --templprefix are model spectra')
    p.add_argument('--keywords', type=str, default='PHXTEFF,PHXLOGG,PHXM_H,PHXALPHA',
                   help='Header keywords of the parameters, in --parameter_names order')
    p.add_argument('--air', action='store_true', default=False,
                   help='Generate spectra in the air (rather than vacuum) frame')
    p.add_argument('--oprefix', type=str, default='templ_data/',
                   help='The path where the library will be created')
    p.add_argument('--wavefile', type=str, required=True,
                   help='The fits file with the wavelength grid of templates')
    p.add_argument('--resolution0', type=float, default=100000,
                   help='The resolution of the input grid')
    p.add_argument('--nthreads', type=int, default=8, help='ignored')
    p.add_argument('--fixed_fwhm', action='store_true', default=False,
                   help='Keep the FWHM of the LSF constant rather than R')
    p.add_argument('--save_specs', action='store_true', default=False,
                   help='also write specs_<setup>.npz, the rows '
                   'rvspecfit_amd.nn.train_interpolator trains on')
    p.add_argument('--regularize', action='store_true', default=False,
                   help='Fill the gaps of the grid and resample its feh and alpha axes '
                   '(rvs_regularize_grid) before the library is made')
    for name, default, text in (('max_feh', 1.2, 'Max feh'), ('min_feh', -4, 'Min feh'),
                                ('max_alpha', 1.2, 'Max alpha'),
                                ('min_alpha', -.4, 'Min alpha'),
                                ('step_feh', .25, 'step feh'),
                                ('step_alpha', .2, 'step alpha'),
                                ('smooth', 0., 'smoothing Parameter')):
        p.add_argument('--' + name, type=float, default=default,
                       help=text + ' (with --regularize)')
    return p


def main(args=None):
    """rvs_make_interpol (+ rvs_regularize_grid with --regularize) + rvs_make_nd
    --regulargrid: writes <oprefix>/lib_<setup>.npz, which TemplateLibrary.from_npz
    reads."""
    import os
    from . import fits_min, make_nd
    parser = make_parser()
    args = parser.parse_args(sys.argv[1:] if args is None else args)
    if args._no_normalize:
        warnings.warn("--no-normalize is deprecated. Use '--normalize none' instead.",
                      DeprecationWarning, stacklevel=2)
        args.normalize = 'none'
    given = (args.resol is not None) + (args.resol_func is not None)
    if given == 0:
        parser.error('Either --resol or --resol_func is required')
    if given == 2:
        parser.error('Either --resol or --resol_func is required, not both')
    if args.fixed_fwhm and args.resol is None:
        parser.error('Either --resol_func is incompatible with --fixed_fwhm')
    resol_func = resolution_from_args(args.resol, args.resol_func, args.fixed_fwhm,
                                      args.lambda0, args.lambda1)
    log_parameters = [int(_) for _ in args.log_parameters.split(',')]
    parnames = args.parameter_names.split(',')
    keys = args.keywords.split(',')
    if len(keys) != len(parnames):
        parser.error('--keywords and --parameter_names differ in length')
    grid = read_grid.scan_grid(args.templprefix, args.mask, dict(zip(parnames, keys)))
    lam_hr = np.asarray(fits_min.open(args.wavefile)[0].data, dtype=np.float64)
    D = build_specs(lam_hr, grid.read(), grid.vec,
                    (args.setup, args.lambda0, args.lambda1, resol_func, args.step,
                     args.log), parnames=parnames, air=args.air,
                    resolution0=args.resolution0, normalize=args.normalize,
                    float_bits=args.float_bits, log_parameters=log_parameters)
    if args.regularize:
        from . import regularize_grid
        D = regularize_grid.regularize(
            D, smooth=args.smooth, min_feh=args.min_feh, max_feh=args.max_feh,
            step_feh=args.step_feh, min_alpha=args.min_alpha, max_alpha=args.max_alpha,
            step_alpha=args.step_alpha)
    lib = make_nd.regular_library(D)
    lib['dats'] = lib['dats'].cpu().numpy()
    lib['revision'] = np.array(args.revision)
    os.makedirs(args.oprefix, exist_ok=True)
    if args.save_specs:
        np.savez(os.path.join(args.oprefix, 'specs_%s.npz' % args.setup),
                 specs=torch.as_tensor(D['specs']).cpu().numpy(), vec=D['vec'], lam=D['lam'],
                 parnames=np.array(D['parnames']), lognorms=D['lognorms'],
                 log_step=np.array(D['log_step']), log_spec=np.array(D['log_spec']),
                 log_ids=np.array(log_parameters, dtype=np.int64))
    fname = os.path.join(args.oprefix, 'lib_%s.npz' % args.setup)
    np.savez(fname, **lib)
    return fname


if __name__ == '__main__':
    main()
