"""The reference's read_grid under its names: the parameter mapper, the rebinner that
takes a high-resolution model to an instrument's resolution and pixels, and the scan
of a directory of model files.

make_rebinner builds the band of the reference's sparse matrix on the device
(rvs_rebin_weights); apply_rebinner multiplies it with model spectra there
(rvs_rebin_apply).  The weights are integrals of the Gaussian-convolved linear
interpolant over the output pixels, evaluated from the antiderivatives of Phi(u) and
u Phi(u) (pix_integrator below states them in numpy; csrc/rebin.hip on the device).
"""
import ctypes
import glob
import warnings

import numpy as np
import torch

from . import _lib

THRESH = 5          # window half width in sigma (read_grid.py:401)
FWHM_TO_SIG = 2 * np.sqrt(2 * np.log(2))


class LogParamMapper:
    """Maps stellar parameters to the space the grid is interpolated in: log10 of the
    parameters numbered in log_ids (read_grid.py:114-167)."""

    def __init__(self, log_ids):
        self.log_ids = log_ids

    def forward(self, vec):
        vec1 = np.array(vec, dtype=np.float64)
        for i in self.log_ids:
            vec1[i] = np.log10(vec1[i])
        return vec1

    def inverse(self, vec):
        vec1 = np.array(vec, dtype=np.float64)
        for i in self.log_ids:
            vec1[i] = 10**(vec1[i])
        return vec1


def _tails(u):
    """(G0, H1) of csrc/rebin.hip: the parts of int Phi and int u Phi that decay"""
    from scipy.special import erfc
    t = np.abs(u)
    q = 0.5 * erfc(t / np.sqrt(2))
    p = np.exp(-0.5 * t * t) / np.sqrt(2 * np.pi)
    e = 0.5 * ((t * t - 1) * q - t * p)
    return p - t * q, np.where(u > 0, -e, e)


def _edge(c, r):
    d = c - r
    g0c, h1c = _tails(c)
    g0d, h1d = _tails(d)
    p0 = np.where(d > 0, r, np.where(c > 0, c, 0.))
    p1 = np.where(d > 0, 0.5 * r * r, np.where(c > 0, 0.5 * c * c + 0.5, 0.))
    dg = g0c - g0d
    return dg + p0, c * dg - (h1c - h1d) + p1


def _kernel(a, b):
    """Phi(b) - Phi(a), the difference taken where it does not cancel"""
    from scipy.special import erfc
    q = np.sqrt(0.5)
    with np.errstate(all='ignore'):
        return np.where(a > 0, 0.5 * (erfc(a * q) - erfc(b * q)),
                        np.where(b < 0, 0.5 * (erfc(-b * q) - erfc(-a * q)),
                                 1.0 - 0.5 * erfc(b * q) - 0.5 * erfc(-a * q)))


_GL8 = np.polynomial.legendre.leggauss(8)


def pix_integrator(x1, x2, l1, l2, s):
    """Weights (c1, c2) of the values at x1, x2 of a linearly interpolated spectrum in
    the flux that a Gaussian LSF of sigma s puts into the pixel [l1, l2]
    (read_grid.py:75-111).  Host statement of what rvs_rebin_weights evaluates: the
    closed form where the input step exceeds sigma, 8-point Gauss-Legendre along the
    segment (all terms positive) where it does not."""
    x1, x2, l1, l2, s = np.broadcast_arrays(*[np.asarray(_, dtype=np.float64)
                                              for _ in (x1, x2, l1, l2, s)])
    r = (x2 - x1) / s
    ca, cb = (l1 - x1) / s, (l2 - x1) / s
    a0, a1 = _edge(ca, r)
    b0, b1 = _edge(cb, r)
    c2 = s * (b1 - a1) / r
    c1 = s * (b0 - a0) - c2
    t = 0.5 * (_GL8[0] + 1)
    k = _GL8[1] * _kernel(ca[..., None] - t * r[..., None], cb[..., None] - t * r[..., None])
    g1 = 0.5 * (x2 - x1) * np.sum((1 - t) * k, axis=-1)
    g2 = 0.5 * (x2 - x1) * np.sum(t * k, axis=-1)
    return np.where(r <= 1, g1, c1), np.where(r <= 1, g2, c2)


class Rebinner:
    """The band of make_rebinner's matrix on the device: W [npix, K] float64, left /
    right int32 [npix] (relative to `col0`, the first input pixel any window uses),
    lam0 [col1 - col0] the (air-converted) input wavelengths of those columns,
    lam [npix]; lam_phot: the wavelengths as given, which extract_spectrum multiplies
    the models by (get_spec's, make_interpol.py:152: not air-converted)."""

    def __init__(self, W, left, right, lam0, lam, col0, n_in, lam_phot=None):
        self.W, self.left, self.right, self.lam0, self.lam = W, left, right, lam0, lam
        self.lam_phot = lam0 if lam_phot is None else lam_phot
        self.col0, self.col1, self.n_in = col0, col0 + lam0.shape[0], n_in
        self.shape = (n_in, lam.shape[0])

    def toarray(self):
        """dense [len(lam0), len(lam)] numpy matrix, as the reference's .toarray()"""
        W = self.W.cpu().numpy()
        left = self.left.cpu().numpy()
        n = self.right.cpu().numpy() - left + 2
        out = np.zeros(self.shape)
        for i in range(self.shape[1]):
            if n[i] > 0:
                out[self.col0 + left[i]:self.col0 + left[i] + n[i], i] = W[i, :n[i]]
        return out


def rebinner_windows(lam0, lam, sigs):
    """(left, right, warn): the segments left[i] .. right[i] of the input grid that
    pixel i integrates (read_grid.py:417-430), clamped; warn: a clamp was needed"""
    n0 = len(lam0)
    left = np.searchsorted(lam0, lam - THRESH * sigs) - 1
    right = np.searchsorted(lam0, lam + THRESH * sigs)
    warn = bool((left < 0).any() or (right > n0 - 2).any())
    return np.clip(left, 0, None), np.clip(right, None, n0 - 2), warn


def rebinner_sigmas(lam, resolution_function, resolution0):
    """LSF sigma per output pixel (read_grid.py:394-400)"""
    R = np.broadcast_to(np.asarray(resolution_function(lam), dtype=np.float64), lam.shape)
    # the LSF to add is what the target lacks over the input; a target at or above the
    # input's resolution is the reference's AssertionError
    assert R.max() < resolution0
    return np.sqrt((lam / R)**2 - (lam / resolution0)**2) / FWHM_TO_SIG


def to_air(lam00):
    """vacuum -> air (read_grid.py:388-390)"""
    return lam00 / (1.0 + 2.735182E-4 + 131.4182 / lam00**2 + 2.76249E8 / lam00**4)


def make_rebinner(lam00, lam, resolution_function, resolution0=None, toair=True,
                  device='cuda'):
    """read_grid.make_rebinner (read_grid.py:360-466): the operator that convolves a
    spectrum on the grid lam00 to the resolution resolution_function(lam) (R = l/dl;
    the input has resolution0) and integrates it over the pixels of lam.  Returns a
    Rebinner (the matrix's band on the device) instead of a scipy sparse matrix."""
    lam00 = np.asarray(lam00, dtype=np.float64)
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    lam0 = to_air(lam00) if toair else lam00
    sigs = rebinner_sigmas(lam, resolution_function, resolution0)
    _lib.require_gpu()
    n0 = len(lam0)
    left, right, warn = rebinner_windows(lam0, lam, sigs)
    if warn:
        warnings.warn('The input spectrum is not wide enough to do LSF convolution. '
                      'The edges of the spectrum will be corrupted.')
    col0 = int(min(left.min(), n0 - 2))
    col1 = int(max(right.max() + 2, col0 + 2))
    K = int(max((right - left + 2).max(), 2))
    up = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dtype=dt)).to(device)
    d_lam0 = up(lam0[col0:col1], np.float64)
    d_lam, d_sig = up(lam, np.float64), up(sigs, np.float64)
    d_left, d_right = up(left - col0, np.int32), up(right - col0, np.int32)
    W = torch.empty((len(lam), K), dtype=torch.float64, device=device)
    rc = _lib.lib().rvs_rebin_weights(_lib.ptr(d_lam0), col1 - col0, _lib.ptr(d_lam),
                                      _lib.ptr(d_sig), _lib.ptr(d_left),
                                      _lib.ptr(d_right), len(lam), K, _lib.ptr(W),
                                      _lib.stream())
    if rc == -1:
        raise ValueError('rvs_rebin_weights: bad argument (%d input, %d output pixels)'
                         % (n0, len(lam)))
    _lib.check(rc, 'rvs_rebin_weights')
    return Rebinner(W, d_left, d_right, d_lam0, d_lam, col0, n0,
                    up(lam00[col0:col1], np.float64) if toair else None)


def apply_band(mat, hr, photons, out=None):
    """rvs_rebin_apply: hr, a float32 / float64 device tensor [T, col1 - col0] holding
    the columns mat.col0 .. mat.col1 - 1 (rows may be strided) -> float64 [T, npix].
    photons: multiply by the input wavelengths (as given: mat.lam_phot) before and
    divide by the output wavelengths after the product (make_interpol.py:152-154)."""
    T, npix = hr.shape[0], mat.lam.shape[0]
    if hr.shape[1] != mat.lam0.shape[0]:
        raise ValueError('%d columns for a band over %d' % (hr.shape[1],
                                                           mat.lam0.shape[0]))
    if hr.dtype not in (torch.float32, torch.float64):
        hr = hr.to(torch.float64)
    if hr.stride(1) != 1 or (T > 1 and hr.stride(0) < hr.shape[1]):
        hr = hr.contiguous()
    if out is None:
        out = torch.empty((T, npix), dtype=torch.float64, device=hr.device)
    step = 32 * 65535
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for a in range(0, T, step):
        part = hr[a:a + step]
        rc = _lib.lib().rvs_rebin_apply(
            p(part), int(hr.dtype == torch.float32), max(part.stride(0), part.shape[1]),
            part.shape[0], mat.lam0.shape[0], _lib.ptr(mat.lam_phot), _lib.ptr(mat.W),
            mat.W.shape[1], _lib.ptr(mat.left), _lib.ptr(mat.right), _lib.ptr(mat.lam),
            npix, int(bool(photons)), p(out[a:a + step]), _lib.stream())
        if rc == -1:
            raise ValueError('rvs_rebin_apply: bad argument')
        _lib.check(rc, 'rvs_rebin_apply')
    return out


def apply_rebinner(mat, spec0):
    """spec0 @ matrix (read_grid.py:469-471).  A numpy spectrum [n_in] or stack
    [T, n_in] returns numpy; a device tensor returns a device tensor."""
    dev = isinstance(spec0, torch.Tensor)
    a = spec0 if dev else np.asarray(spec0)
    if a.shape[-1] != mat.n_in:
        raise ValueError('spectra of %d pixels for a rebinner of %d'
                         % (a.shape[-1], mat.n_in))
    rows = a.reshape(-1, mat.n_in)[:, mat.col0:mat.col1]
    if not dev:
        if rows.dtype != np.float32:
            rows = rows.astype(np.float64)
        rows = torch.as_tensor(np.ascontiguousarray(rows)).to(mat.W.device)
    ret = apply_band(mat, rows, False)
    ret = ret[0] if a.ndim == 1 else ret
    return ret if dev else ret.cpu().numpy()


def rebin(lam0, spec0, newlam, resolution, resolution0=100000, toair=True):
    """Rebin the spectrum (lam0, spec0) to the wavelengths newlam at `resolution`, a
    function of wavelength or a number (read_grid.py:474-503).  The reference's rebin
    leaves make_rebinner's resolution0 unset and cannot run; here it is an argument with
    rvs_make_interpol's default, and toair make_rebinner's."""
    if not callable(resolution):
        R = float(resolution)
        resolution = lambda x: R
    mat = make_rebinner(lam0, newlam, resolution, resolution0=resolution0, toair=toair)
    return apply_rebinner(mat, spec0)


class GridFiles:
    """What read_grid.makedb (read_grid.py:170-292) extracts from a directory of model
    spectra, without the sqlite file: `filenames` (relative to prefix), `vec`
    [npar, nfiles] and `file_ids` (position in the sorted file list) in the order of
    make_interpol._fetch_all_parameters' `order by` (make_interpol.py:230-235): by the
    parameters, first name first."""

    def __init__(self, prefix, filenames, parnames, vec, file_ids):
        self.prefix, self.filenames, self.parnames = prefix, filenames, tuple(parnames)
        self.vec, self.file_ids = vec, file_ids

    def read(self, chunk=64):
        """the data of the files' first HDUs in row order, `chunk` rows at a time"""
        from . import fits_min
        for a in range(0, len(self.filenames), chunk):
            yield np.stack([np.asarray(fits_min.open(self.prefix + f)[0].data)
                            for f in self.filenames[a:a + chunk]])


def scan_grid(prefix, mask='*/*fits', keywords=None, parnames=None):
    """The sorted list of files prefix + mask, their parameters read from the header
    keywords (`keywords`: parameter name -> keyword; default the PHOENIX ones), rows
    ordered by `parnames` (default: the keywords' order).  A file without one of the
    keywords raises as makedb does."""
    from . import fits_min
    if keywords is None:
        keywords = dict(teff='PHXTEFF', logg='PHXLOGG', feh='PHXM_H', alpha='PHXALPHA')
    fs = sorted(glob.glob(prefix + mask))
    if len(fs) == 0:
        raise Exception(
            "No FITS templates found in the directory specified (using mask %s" % mask)
    parnames = list(keywords.keys()) if parnames is None else list(parnames)
    pars = []
    for f in fs:
        hdr = fits_min.open(f)[0].header
        cur = {}
        for param, curkey in keywords.items():
            if curkey not in hdr:
                raise Exception(f"Keyword for {param} {curkey} not found in {f}")
            cur[param] = float(hdr[curkey])
        pars.append([cur[p] for p in parnames])
    vec = np.array(pars, dtype=np.float64).T
    order = np.lexsort(vec[::-1])
    return GridFiles(prefix, [fs[i].replace(prefix, '') for i in order], parnames,
                     vec[:, order], np.asarray(order))
