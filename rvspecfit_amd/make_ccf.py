"""CCF pre-processing -- API mirror of py/rvspecfit/make_ccf.py on the MI355X kernels.

The data side (what fitter_ccf.fit calls per spectrum and arm):
preprocess_data, one block per spectrum of rvs_ccf_preprocess.

The template side (make_ccf.py:39-64, 105-285, 415-493): get_mortoncurve_id and the
[::every] selection on the host (integer work); get_continuum, preprocess_model,
preprocess_model_list and build_ccf_set -- ccf_executor without its files -- on the
device: one block per model row (template x vsini) of rvs_ccf_models_build fits the
robust continuum with the Levenberg-Marquardt of the data kernel, divides it out and
puts the row on the FFT grid; the same call transforms the models and their squares.
TemplateLibrary.add_ccf_set attaches the result to a loaded library.  Not rebuilt: the
HDF5 / npy files ccf_executor writes and the rvs_make_ccf command line (main).
"""
import types

import numpy as np
import torch

from . import _lib
from . import ccf_tables
from . import engine


def get_continuum_prefix(continuum):
    """make_ccf.py:19-24"""
    return '' if continuum else 'nocont_'


def get_ccf_info_name(spec_setup, continuum=True):
    return 'ccf_' + get_continuum_prefix(continuum) + '%s.h5' % spec_setup


def get_ccf_dat_name(spec_setup, continuum=True):
    return 'ccfdat_' + get_continuum_prefix(continuum) + '%s.npz' % spec_setup


def get_ccf_mod_name(spec_setup, continuum=True):
    return 'ccfmod_' + get_continuum_prefix(continuum) + '%s.npy' % spec_setup


def get_ccf_config(logl0=None, logl1=None, npoints=None, splinestep=1000,
                   maxcontpts=20):
    """make_ccf.get_ccf_config (make_ccf.py:66-102): the dictionary that describes
    a cross-correlation set-up -- FFT grid log(lambda) logl0..logl1 in `npoints`
    steps, continuum nodes every `splinestep` km/s but at most `maxcontpts` of them
    (splinestep None: no continuum normalisation)."""
    conf = dict(logl0=logl0, logl1=logl1, npoints=npoints, continuum=True,
                maxcontpts=maxcontpts)
    if splinestep is None:
        conf['continuum'] = False
    else:
        widest = 3e5 * (np.exp((logl1 - logl0) / maxcontpts) - 1)
        conf['splinestep'] = max(splinestep, widest)
    return conf


def to_power_two(i):
    """make_ccf.to_power_two (make_ccf.py:496-497): the next power of two >= i"""
    return 2**(int(np.ceil(np.log(i) / np.log(2))))


def interp_masker(lam, spec, badmask):
    """make_ccf.interp_masker (make_ccf.py:288-327): the spectrum with its masked
    pixels filled -- linearly in wavelength between the nearest good neighbours, with
    the nearest good value beyond the first / last good pixel; everything masked: the
    spectrum itself with non-finite values set to 1.  Host arithmetic on one spectrum
    (index work; preprocess_data does the same inside its kernel for a batch)."""
    lam = np.asarray(lam)
    spec = np.asarray(spec)
    bad = np.asarray(badmask, dtype=bool)
    out = spec * 1
    good_ix = np.flatnonzero(~bad)
    if good_ix.size == 0:
        import logging
        logging.warning('All the pixels are masked for the ccf determination')
        out[~np.isfinite(out)] = 1
        return out
    bad_ix = np.flatnonzero(bad)
    nxt = np.searchsorted(good_ix, bad_ix)      # first good pixel behind each bad one
    left, right = nxt == 0, nxt == good_ix.size
    inner = ~(left | right)
    out[bad_ix[left]] = spec[good_ix[0]]
    out[bad_ix[right]] = spec[good_ix[-1]]
    a, b = good_ix[nxt[inner] - 1], good_ix[nxt[inner]]
    l0 = lam[bad_ix[inner]]
    out[bad_ix[inner]] = (-(lam[a] - l0) * spec[b] + (lam[b] - l0) * spec[a]) / \
        (lam[b] - lam[a])
    return out


class _ConfLib:
    """what ArmData.ccf_tables reads of a template library: the CCF set-up"""

    def __init__(self, ccfconf):
        self.name = 'ccfconf'
        self._cc = dict(ccfconf)
        self._cc.setdefault('maxcontpts', 20)

    def ccf_set(self, config):
        return self._cc


def preprocess_data(lam, spec0, espec, ccfconf=None, badmask=None, maxerr=10):
    """make_ccf.preprocess_data (make_ccf.py:330-414): the spectrum as the CCF
    templates were prepared -- median filter and masks (error above maxerr medians,
    non-positive filtered flux, the caller's badmask), gaps filled linearly, the
    robust continuum exp(spline) divided out, rebinned onto the FFT grid with the
    inverse variance of the rebinned pixel.  Returns (spec [npoints], ivar
    [npoints]) as numpy; 2-D spec0 / espec / badmask [S, npix] give [S, npoints]
    device tensors.  One block per spectrum of rvs_ccf_preprocess (csrc/ccf.hip)."""
    _lib.require_gpu()
    single = np.ndim(spec0) == 1
    arm = engine.ArmData('ccfconf', np.asarray(lam, dtype=np.float64), spec0,
                         espec, badmask)
    pre = engine.ccf_preprocess(arm, _ConfLib(ccfconf), {}, maxerr=float(maxerr))
    if single:
        return (pre['proc_spec'][0].cpu().numpy(),
                pre['proc_ivar'][0].cpu().numpy())
    return pre['proc_spec'], pre['proc_ivar']


# ---------------------------------------------------------------------------
# the template side
# ---------------------------------------------------------------------------
def interleave_bits(X):
    """make_ccf.interleave_bits (make_ccf.py:39-55): the z-curve (Morton) number of
    the points X [nsamp, ndim] of the unit cube.  A coordinate is cut to b = 64 // ndim
    bits (1.0 falls into the last cell) and bit j of coordinate i becomes bit
    j ndim + i of the number.  All points at once: the bits as an [nsamp, ndim, b]
    array against the table of their places, summed without carries.  With ndim a
    divisor of 64 the top place is the sign bit of the int64 result, as it is in the
    reference, whose order np.argsort then follows.  (One dimension: 52 bits, all a
    double carries -- the reference's 64 overflow its int64 cast.)"""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2 or X.min() < 0 or X.max() > 1:
        raise ValueError('interleave_bits: points [nsamp, ndim] of the unit cube expected')
    ndim = X.shape[1]
    b = min(64 // ndim, 52)
    cell = np.minimum(np.floor(np.ldexp(X, b)), 2.0**b - 1).astype(np.uint64)
    j = np.arange(b, dtype=np.uint64)
    place = j[None, :] * np.uint64(ndim) + np.arange(ndim, dtype=np.uint64)[:, None]
    bits = (cell[:, :, None] >> j[None, None, :]) & np.uint64(1)
    return (bits << place[None, :, :]).sum(axis=(1, 2), dtype=np.uint64).view(np.int64)


def get_mortoncurve_id(X):
    """make_ccf.get_mortoncurve_id (make_ccf.py:58-63): Morton number of the rows of
    X [nsamp, ndim] after replacing every column by its dense ranks scaled to [0, 1].
    Only the order of the values of a column enters, so the mapped parameters of a
    library (log10 Teff) give the numbers of the physical ones.  A column with a
    single value is 0 / 0 in the reference (a NaN cast to an integer): ValueError."""
    X = np.asarray(X)
    Xr = np.array([np.unique(c, return_inverse=True)[1].reshape(-1) for c in X.T]).T
    top = Xr.max(axis=0)
    if np.any(top == 0):
        raise ValueError(
            'get_mortoncurve_id: parameter column(s) %s hold a single value; their '
            'scaled rank is 0 / 0 (make_ccf.py:62)' % (np.nonzero(top == 0)[0].tolist(), ))
    return interleave_bits(Xr / top)


def select_templates(vec, every):
    """row numbers of the templates of a set: every `every`-th along the Morton curve
    (make_ccf.py:457-460); vec [ndim, nspec] as the library stores it"""
    return np.argsort(get_mortoncurve_id(np.asarray(vec).T))[::every]


def model_tables(lam, ccfconf):
    """What rvs_ccf_models_build reads of a template grid and a CCF set-up (host, once
    per library; ccf_tables.py): ln(lam), the FFT grid, interp1d's bracketing index
    (-1 outside the row) and, with continuum, the spline and bin tables of the nodes
    the reference takes from the row's own wavelength range."""
    lam = np.ascontiguousarray(lam, dtype=np.float64)
    ntp = len(lam)
    if ntp > MODEL_MAX_NTP:
        raise ValueError('model rows of %d pixels: rvs_ccf_models_build takes at most '
                         '%d' % (ntp, MODEL_MAX_NTP))
    lnlam = np.log(lam)
    logl = np.linspace(ccfconf['logl0'], ccfconf['logl1'], ccfconf['npoints'])
    ihi = np.clip(np.searchsorted(lnlam, logl), 1, ntp - 1).astype(np.int32)
    ihi[(logl < lnlam[0]) | (logl > lnlam[-1])] = -1
    T = dict(ntp=ntp, lnlam=lnlam, logl=logl, ihi=ihi, nnode=0,
             continuum=bool(ccfconf['continuum']))
    if T['continuum']:
        nodes, edges = ccf_tables.continuum_nodes(lam, ccfconf['splinestep'])
        if len(nodes) > MODEL_MAX_NODE or len(nodes) < 3:
            raise ValueError('%d continuum nodes: rvs_ccf_models_build takes 3 to %d'
                             % (len(nodes), MODEL_MAX_NODE))
        Eb, El, Cinv, istart = ccf_tables.interp_spline_tables(nodes, lam)
        T.update(nodes=nodes, nnode=len(nodes), Eb=Eb, El=El, istart=istart,
                 Cinv=np.stack([Cinv, np.linalg.inv(Cinv)]),
                 bin_start=ccf_tables.bin_ranges(lam, edges))
    return T


MODEL_MAX_NTP = 9216    # RVS_CCF_MODEL_MAX_NTP
MODEL_MAX_NODE = 48


def models_build(lam, rows, ccfconf, f32row=None, erows=None, transforms=True,
                 details=False):
    """rvs_ccf_models_build on rows [M, ntp] (float64 device tensor): dict(model
    [M, npoints], fft / fft2 complex128 [M, npoints/2 + 1] when `transforms`, status
    int32 [M]; details: cont [M, ntp], pfit [M, nnode]), all on the device."""
    _lib.require_gpu()
    T = model_tables(lam, ccfconf)
    dev = rows.device
    M, ntp = rows.shape
    if ntp != T['ntp']:
        raise ValueError('rows of %d pixels on a grid of %d' % (ntp, T['ntp']))
    rows = rows.to(torch.float64).contiguous()
    npoints = int(ccfconf['npoints'])
    up = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev)
    cont = T['continuum']
    tabs = {k: up(T.get(k)) for k in ('Eb', 'El', 'Cinv', 'istart', 'bin_start',
                                      'lnlam', 'logl', 'ihi')}
    f32 = None if f32row is None else up(np.asarray(f32row, dtype=np.uint8))
    out = dict(model=torch.empty((M, npoints), dtype=torch.float64, device=dev),
               status=torch.zeros(M, dtype=torch.int32, device=dev))
    twid = None
    if transforms:
        if npoints < 64 or npoints > 16384 or npoints & (npoints - 1):
            raise ValueError('npoints = %d: the transforms take a power of two, 64 to '
                             '16384' % npoints)
        for k in ('fft', 'fft2'):
            out[k] = torch.empty((M, npoints // 2 + 1), dtype=torch.complex128,
                                 device=dev)
        twid = up(np.exp(2j * np.pi * np.arange(npoints // 2) / npoints).view(np.float64))
    if details and cont:
        out['cont'] = torch.empty((M, ntp), dtype=torch.float64, device=dev)
        out['pfit'] = torch.empty((M, T['nnode']), dtype=torch.float64, device=dev)
    rc = _lib.lib().rvs_ccf_models_build(
        _lib.ptr(rows), _lib.ptr(f32), _lib.ptr(erows), ntp, M, int(cont),
        _lib.ptr(tabs['Eb']), _lib.ptr(tabs['El']), _lib.ptr(tabs['Cinv']),
        _lib.ptr(tabs['istart']), T['nnode'], _lib.ptr(tabs['bin_start']),
        _lib.ptr(tabs['lnlam']), _lib.ptr(tabs['logl']), _lib.ptr(tabs['ihi']), npoints,
        _lib.ptr(twid), _lib.ptr(out['model']), _lib.ptr(out.get('fft')),
        _lib.ptr(out.get('fft2')), _lib.ptr(out.get('cont')), _lib.ptr(out.get('pfit')),
        _lib.ptr(out['status']), _lib.stream())
    if rc == -1:
        raise ValueError('rvs_ccf_models_build: bad argument (rows of %d pixels, %d '
                         'nodes, %d points)' % (ntp, T['nnode'], npoints))
    _lib.check(rc, 'rvs_ccf_models_build')
    return out


def _as_rows(a):
    """(float64 device rows [M, ntp], float32 flag) of a host / device array"""
    f32 = (a.dtype == torch.float32) if isinstance(a, torch.Tensor) else \
        (np.asarray(a).dtype == np.float32)
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a))
    return torch.atleast_2d(t).to('cuda', torch.float64).contiguous(), bool(f32)


def get_continuum(lam0, spec0, espec0, ccfconf=None):
    """make_ccf.get_continuum (make_ccf.py:105-152): the continuum exp(spline) of a
    spectrum by the robust (soft-L1) fit of its node values, on the device.  1-D
    spec0 / espec0: numpy [npix]; 2-D [M, npix]: a device tensor, one launch."""
    _lib.require_gpu()
    single = np.ndim(spec0) == 1
    rows, f32 = _as_rows(spec0)
    erows, _ = _as_rows(espec0)
    cc = dict(ccfconf, continuum=True)
    if cc.get('npoints') is None:      # (the FFT grid plays no part here)
        cc.update(logl0=float(np.log(np.min(lam0))), logl1=float(np.log(np.max(lam0))),
                  npoints=2)
    res = models_build(lam0, rows, cc, f32row=[f32] * rows.shape[0], erows=erows,
                       transforms=False, details=True)
    return res['cont'][0].cpu().numpy() if single else res['cont']


def _broadened_rows(lam, rows, f32, vsinis):
    """the rows of preprocess_model_list's double loop -- for model, for vsini -- with
    spec_fit.convolve_vsini applied where vsini is neither None nor 0
    (make_ccf.py:189-192); returns rows [M * V, ntp], the float32 flags"""
    M, ntp = rows.shape
    V = len(vsinis)
    out = rows[:, None, :].repeat(1, V, 1)
    flags = np.zeros((M, V), dtype=np.uint8)
    for j, vs in enumerate(vsinis):
        if vs is not None and vs != 0:
            vv = torch.full((M, ), float(vs), dtype=torch.float64, device=rows.device)
            out[:, j, :] = engine.convolve_vsini(lam, rows, vv)
        else:
            flags[:, j] = f32
    return out.reshape(M * V, ntp).contiguous(), flags.reshape(-1)


def preprocess_model(logl, lammodel, model0, vsini=None, ccfconf=None):
    """make_ccf.preprocess_model (make_ccf.py:167-221): the model on the FFT grid
    `logl` (= linspace(logl0, logl1, npoints) of ccfconf), broadened, its continuum
    divided out, 1 outside the model's range.  numpy [npoints]."""
    import logging
    lnl = np.log(np.asarray(lammodel, dtype=np.float64))
    if not (lnl[0] <= logl[0] <= lnl[-1]) or not (lnl[0] <= logl[-1] <= lnl[-1]):
        logging.warning('The required wavelength range is bigger than the template '
                        'wavelengths')
    rows, f32 = _as_rows(model0)
    rows, flags = _broadened_rows(np.asarray(lammodel), rows, f32, [vsini])
    cc = dict(ccfconf, logl0=float(logl[0]), logl1=float(logl[-1]), npoints=len(logl))
    return models_build(lammodel, rows, cc, f32row=flags,
                        transforms=False)['model'][0].cpu().numpy()


def preprocess_model_list(lammodels, models, params, ccfconf, vsinis=None, nthreads=1):
    """make_ccf.preprocess_model_list (make_ccf.py:224-285): every model at every
    vsini (order: for model, for vsini; vsinis None: [None]) in one launch.  Returns
    (models [M * V, npoints] numpy, params [M * V, ndim], the vsini of every row);
    `nthreads` is accepted and ignored."""
    if vsinis is None:
        vsinis = [None]
    vsinis = list(vsinis)
    rows, f32 = _as_rows(models)
    rows, flags = _broadened_rows(np.asarray(lammodels), rows, f32, vsinis)
    retparams = np.repeat(np.asarray(params), len(vsinis), axis=0)
    vlist = vsinis * (rows.shape[0] // len(vsinis))
    res = models_build(lammodels, rows, ccfconf, f32row=flags, transforms=False)
    return res['model'].cpu().numpy(), retparams, vlist


def build_ccf_set(source, ccfconf, every=30, vsinis=None):
    """make_ccf.ccf_executor (make_ccf.py:415-493) without its files: the CCF template
    set of a library -- every `every`-th template along the Morton curve of the
    parameters, at every vsini -- as a dictionary in the converted artefact's keys
    (ccf_fft, ccf_fft2, ccf_mod, ccf_params, ccf_vsinis [NaN = None], ccf_parnames,
    ccf_logl0, ccf_logl1, ccf_npoints, ccf_continuum, ccf_maxcontpts, ccf_splinestep;
    prefix ccfnc_ without continuum normalisation): what TemplateLibrary.add_ccf_set,
    TemplateLibrary(name, {**library, **set}) and the oracle's Library read.
    source: a regular-grid TemplateLibrary (or its npz dictionary: rows `dats`,
    parameters 10**vec where the mapper took log10), or the contents of a
    specs_<setup>.h5 (lam, specs, vec, parnames, log_spec) in physical units."""
    _lib.require_gpu()
    L = _lib.lib()
    from .library import TemplateLibrary
    if isinstance(source, TemplateLibrary):
        if source.kind != 'regulargrid':
            raise ValueError('build_ccf_set: a %s library carries no plain list of '
                             'its templates; pass the contents of specs_<setup>.h5'
                             % source.kind)
        lam, dats, vec = source.lam, source.dats, source.vec
        log_spec, log_ids, parnames = bool(source.exp_flag), source.log_ids, source.parnames
    else:
        src = dict(source)
        lam = np.asarray(src['lam'], dtype=np.float64)
        parnames = tuple(str(_) for _ in src['parnames'])
        vec = np.asarray(src['vec'], dtype=np.float64)
        log_spec = bool(src.get('log_spec', True))
        if 'specs' in src:
            dats, log_ids = src['specs'], ()
        else:
            if 'simplices' in src or 'idgrid' not in src:
                raise ValueError('build_ccf_set: only regular-grid libraries list '
                                 'their templates; pass the contents of specs_<setup>.h5')
            dats = src['dats']
            log_ids = [int(_) for _ in np.atleast_1d(src.get('log_ids', [0]))]
    inds = select_templates(vec, every)
    params = vec.T[inds, :].copy()
    for i in log_ids:                      # LogParamMapper.inverse (read_grid.py)
        params[:, i] = 10**params[:, i]
    ntp = len(lam)
    host = not isinstance(dats, torch.Tensor)
    if host and np.asarray(dats).dtype != np.float32:
        # float64 rows: no float32 step anywhere
        rows = torch.as_tensor(np.ascontiguousarray(np.asarray(dats)[inds],
                                                    dtype=np.float64)).to('cuda')
        rows = rows.exp() if log_spec else rows
        f32 = False
    else:
        if host:    # only the chosen rows travel
            dats = torch.as_tensor(np.ascontiguousarray(np.asarray(dats)[inds])).to('cuda')
            sel = np.arange(len(inds))
        else:
            sel = inds
        if dats.dtype != torch.float32 or dats.dim() != 2 or dats.shape[1] != ntp:
            raise ValueError('build_ccf_set: float32 rows [n, %d] expected' % ntp)
        dats = dats.contiguous()
        sel = torch.as_tensor(np.ascontiguousarray(sel), dtype=torch.int64).to(dats.device)
        rows = torch.empty((len(inds), ntp), dtype=torch.float64, device=dats.device)
        rc = L.rvs_ccf_model_rows(_lib.ptr(dats), dats.shape[0], _lib.ptr(sel),
                                  int(log_spec), ntp, len(inds), _lib.ptr(rows),
                                  _lib.stream())
        _lib.check(rc, 'rvs_ccf_model_rows')
        f32 = True
    vs_in = [None] if vsinis is None else list(vsinis)
    rows, flags = _broadened_rows(lam, rows, f32, vs_in)
    res = models_build(lam, rows, ccfconf, f32row=flags, transforms=True)
    pre = 'ccf_' if ccfconf['continuum'] else 'ccfnc_'
    V = len(vs_in)
    d = {pre + 'fft': res['fft'].cpu().numpy(), pre + 'fft2': res['fft2'].cpu().numpy(),
         pre + 'mod': res['model'].cpu().numpy(),
         pre + 'params': np.repeat(params, V, axis=0),
         pre + 'vsinis': np.array([np.nan if v is None else float(v) for v in vs_in] *
                                  len(inds), dtype=np.float64),
         pre + 'parnames': np.array(parnames),
         pre + 'logl0': np.float64(ccfconf['logl0']),
         pre + 'logl1': np.float64(ccfconf['logl1']),
         pre + 'npoints': np.int64(ccfconf['npoints']),
         pre + 'continuum': np.bool_(ccfconf['continuum']),
         pre + 'maxcontpts': np.int64(ccfconf.get('maxcontpts', 20))}
    if ccfconf['continuum']:
        d[pre + 'splinestep'] = np.float64(ccfconf['splinestep'])
    return d
