"""Exact truth of the velocity-grid chi^2 under a banded resolution matrix
(rvs_chisq_grid_resol: chisq_grid_resol_pipe_kernel<P, 11> and
chisq_grid_resol_kernel<P>, csrc/chisq.hip), in plain numpy, no device.

What the kernels are given and what they compute:

  * spline records in power form, coef[t, i] = {y, b, c, d}: on knot interval i
    the template is y + b dl + c dl^2 + d dl^3, dl = x - knots[i] (form 1 of
    rvs_spline_construct);
  * x = lam * sqrt((1 - beta) / (1 + beta)), beta = v / c.  The shifted
    wavelength is a float64 number in the reference too (spec_fit.py:707-727) and
    is formed here with the same correctly rounded float64 operations; everything
    behind it runs in np.longdouble;
  * the band: model_k = sum_d taps[k, d] raw[k - m + d], m = (nd - 1) / 2, columns
    outside [0, npix) contribute nothing;
  * the value: chisq_truth.chisq0_longdouble(spec, model, polys, espec) on the RAW
    continuum basis (Householder QR in 80-bit arithmetic).  chisq0_longdouble_batch
    is that function for a stack of models; test_chisq_grid_resol_cpu.py holds it
    to the one-model function.

Range rule of the kernels (the reference's evaler, spliner.c:78-83): a velocity is
out of range when the FIRST or the LAST shifted pixel is < knots[0] or
>= knots[-1]; the job then carries RVS_ST_SPLINE_RANGE and the entry is not finite.

The interval of x comes from searchsorted: the spline is continuous, so at a knot
either neighbour gives the same value and the kernels' (int) index need not be
mimicked.

orthonormal_f64_form() is the float64 statement of what the device computes (the
same model through chisq_truth.chisq0_orthonormal_f64).  Its worst distance from the
truth over the inputs of sweeps A-F (cases()) is EMULATION_WORST, the number the
device bound of tests/test_chisq_grid_resol_gpu.py rests on.
"""
import os

import numpy as np

from chisq_truth import chisq0_orthonormal_f64

LD = np.longdouble
C_KMS = 299792.458
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# Worst |orthonormal_f64_form - truth| / max(|truth|, npix) over every job and
# velocity of cases() (sweeps A-F), spline records from power_form() of the oracle's
# template.  Produced by
#     python -c "import sys; sys.path[:0] = ['.', 'tests']; \
#         import chisq_grid_resol_truth as t; print(t.emulation_worst())"
EMULATION_WORST = 2.28e-12      # (case C-2-rbf; every other case <= 9.1e-13)
# (the kernels themselves, measured on an MI355X against the same truth: 4.03e-12 on
# C-2-rbf, <= 1.23e-12 on every other case; the device bound is 10 x the constant
# above, whatever the kernels show)
# the same figure per ill-conditioned case of sweep H (h_cases()): key (snr, masked
# fraction, inflation, npoly, nd) -> worst error over the four velocities, from
#     python -c "import sys; sys.path[:0] = ['.', 'tests']; \
#         import chisq_grid_resol_truth as t; print(t.h_emulation_errors())"
H_EMULATION = {
    (30.0, 0.5, 1e4, 10, 11): 3.40e-11, (30.0, 0.5, 1e6, 10, 11): 8.77e-07,
    (30.0, 0.7, 1e4, 10, 11): 1.38e-11, (30.0, 0.3, 1e6, 10, 11): 2.46e-09,
    (1000.0, 0.5, 1e4, 10, 11): 1.34e-09, (1000.0, 0.5, 1e6, 10, 11): 6.99e-07,
    (1000.0, 0.7, 1e4, 10, 11): 6.34e-09, (1000.0, 0.3, 1e6, 10, 11): 2.28e-08,
    (30.0, 0.5, 1e4, 15, 11): 7.13e-11, (30.0, 0.5, 1e6, 15, 11): 1.16e-06,
    (30.0, 0.7, 1e4, 15, 11): 2.78e-11, (30.0, 0.3, 1e6, 15, 11): 3.03e-07,
    (1000.0, 0.5, 1e4, 15, 11): 1.38e-09, (1000.0, 0.5, 1e6, 15, 11): 1.80e-06,
    (1000.0, 0.7, 1e4, 15, 11): 7.24e-09, (1000.0, 0.3, 1e6, 15, 11): 2.75e-06,
    (30.0, 0.5, 1e4, 10, 13): 5.88e-11, (30.0, 0.5, 1e6, 10, 13): 8.29e-07,
    (30.0, 0.7, 1e4, 10, 13): 3.18e-11, (30.0, 0.3, 1e6, 10, 13): 8.20e-09,
    (1000.0, 0.5, 1e4, 10, 13): 1.35e-09, (1000.0, 0.5, 1e6, 10, 13): 7.13e-07,
    (1000.0, 0.7, 1e4, 10, 13): 6.34e-09, (1000.0, 0.3, 1e6, 10, 13): 3.82e-08,
    (30.0, 0.5, 1e4, 15, 13): 6.40e-11, (30.0, 0.5, 1e6, 15, 13): 1.10e-06,
    (30.0, 0.7, 1e4, 15, 13): 3.77e-11, (30.0, 0.3, 1e6, 15, 13): 6.66e-07,
    (1000.0, 0.5, 1e4, 15, 13): 1.38e-09, (1000.0, 0.5, 1e6, 15, 13): 1.95e-06,
    (1000.0, 0.7, 1e4, 15, 13): 7.23e-09, (1000.0, 0.3, 1e6, 15, 13): 4.07e-06,
}
H_FLAG_ABOVE = 5e-8     # cases above it are the ones the device must flag


# --------------------------------------------------------------------------
# the truth
# --------------------------------------------------------------------------
def doppler(vels):
    """the kernels' factor, float64 operation for operation"""
    bb = np.asarray(vels, dtype=np.float64) / C_KMS
    return np.sqrt((1.0 - bb) / (1.0 + bb))


def in_range(knots, lam, vels):
    """bool [Nv]: the range rule of the kernels"""
    f = np.atleast_1d(doppler(vels))
    xa, xb = lam[0] * f, lam[-1] * f
    x0, xl = knots[0], knots[-1]
    return ~((xa < x0) | (xb < x0) | (xa >= xl) | (xb >= xl))


def raw_template(coef, knots, lam, vels):
    """the cubic of the records at the shifted pixels: longdouble [Nv, npix]"""
    knots = np.asarray(knots, dtype=np.float64)
    x = np.asarray(lam, dtype=np.float64)[None, :] * np.atleast_1d(doppler(vels))[:, None]
    i = np.clip(np.searchsorted(knots, x, 'right') - 1, 0, len(knots) - 2)
    dl = x.astype(LD) - knots.astype(LD)[i]
    c = np.asarray(coef, dtype=np.float64).astype(LD)[i]
    return ((c[..., 3] * dl + c[..., 2]) * dl + c[..., 1]) * dl + c[..., 0]


def apply_band(taps, raw):
    """model[v, k] = sum_d taps[k, d] raw[v, k - m + d]; taps [npix, nd]"""
    taps = np.asarray(taps)
    npix, nd = taps.shape
    m = (nd - 1) // 2
    out = np.zeros(raw.shape, dtype=raw.dtype)
    for d in range(nd):
        o = d - m
        k0, k1 = max(0, -o), min(npix, npix - o)
        if k1 > k0:
            out[:, k0:k1] += taps[k0:k1, d].astype(raw.dtype)[None, :] * \
                raw[:, k0 + o:k1 + o]
    return out


def chisq0_longdouble_batch(spec, models, polys, espec):
    """chisq_truth.chisq0_longdouble for models [Nv, npix] at once"""
    e = np.asarray(espec, dtype=LD)
    D = np.asarray(spec, dtype=LD) / e
    models = np.asarray(models, dtype=LD)
    out = np.empty(len(models), dtype=LD)
    PT = np.asarray(polys, dtype=LD).T
    p = PT.shape[1]
    for a in range(0, len(models), 128):
        mm = models[a:a + 128]
        A = PT[None, :, :] * (mm / e)[:, :, None]
        y = np.repeat(D[None, :], len(mm), axis=0)
        logdet = np.zeros(len(mm), dtype=LD)
        for k in range(p):
            x = A[:, k:, k]
            nx = np.sqrt(np.sum(x * x, axis=1))
            alpha = np.where(x[:, 0] > 0, -nx, nx)
            v = x.copy()
            v[:, 0] -= alpha
            vv = np.sum(v * v, axis=1)
            ok = vv > 0
            g = np.where(ok, 2 / np.where(ok, vv, 1), 0)
            A[:, k:, k:] -= v[:, :, None] * (
                g[:, None] * np.sum(v[:, :, None] * A[:, k:, k:], axis=1))[:, None, :]
            y[:, k:] -= v * (g * np.sum(v * y[:, k:], axis=1))[:, None]
            logdet += 2 * np.log(np.abs(A[:, k, k]))
        out[a:a + 128] = logdet + 2 * np.sum(np.log(e)) + \
            np.sum(y[:, p:] * y[:, p:], axis=1)
    return out


def model(coef, knots, lam, taps, vels):
    return apply_band(taps, raw_template(coef, knots, lam, vels))


def chisq_grid_truth(coef, knots, lam, spec, espec, polys, taps, vels):
    """-2 log L of one (spectrum, template) at every velocity: longdouble [Nv],
    NaN where the range rule puts the velocity outside the knots"""
    vels = np.atleast_1d(np.asarray(vels, dtype=np.float64))
    out = chisq0_longdouble_batch(spec, model(coef, knots, lam, taps, vels), polys,
                                  espec)
    out[~in_range(knots, lam, vels)] = np.nan
    return out


def orthonormal_f64_form(coef, knots, lam, spec, espec, polys, taps, vels):
    """the same model through the float64 emulation of the device's arithmetic"""
    vels = np.atleast_1d(np.asarray(vels, dtype=np.float64))
    mm = model(coef, knots, lam, taps, vels).astype(np.float64)
    out = np.array([chisq0_orthonormal_f64(spec, t, polys, espec) for t in mm])
    out[~in_range(knots, lam, vels)] = np.nan
    return out


# --------------------------------------------------------------------------
# records and bands
# --------------------------------------------------------------------------
def power_form(knots, ys):
    """natural cubic spline through (knots, ys) as the records the kernels read:
    float64 [ntp, 4] = {y, b, c, d} per interval (the last row is never read)"""
    x = np.asarray(knots, dtype=np.float64).astype(LD)
    y = np.asarray(ys, dtype=np.float64).astype(LD)
    n = len(x)
    h = np.diff(x)
    sl = np.diff(y) / h
    z = np.zeros(n, dtype=LD)
    m = n - 2
    cp, dp = np.zeros(m, dtype=LD), np.zeros(m, dtype=LD)
    for i in range(m):      # Thomas sweep on the interior second derivatives
        diag = 2 * (h[i] + h[i + 1])
        rhs = 6 * (sl[i + 1] - sl[i])
        if i == 0:
            den = diag
        else:
            den = diag - h[i] * cp[i - 1]
            rhs = rhs - h[i] * dp[i - 1]
        cp[i] = h[i + 1] / den
        dp[i] = rhs / den
    for i in range(m - 1, -1, -1):
        z[i + 1] = dp[i] - (cp[i] * z[i + 2] if i < m - 1 else 0)
    out = np.zeros((n, 4))
    out[:-1, 0] = y[:-1]
    out[:-1, 1] = sl - h * (2 * z[:-1] + z[1:]) / 6
    out[:-1, 2] = z[:-1] / 2
    out[:-1, 3] = (z[1:] - z[:-1]) / (6 * h)
    return out


def band_taps(npix, nd, seed):
    """row taps [npix, nd] of a band whose every entry inside the matrix -- the
    first and last (nd - 1) / 2 rows included -- is non-trivial, zero where the
    column is outside [0, npix); rows sum to one"""
    rng = np.random.RandomState(seed)
    m = (nd - 1) // 2
    offs = np.arange(-m, m + 1)
    t = rng.uniform(0.3, 1.0, (npix, nd)) * \
        np.exp(-0.5 * (offs[None, :] / (0.4 * m + 0.5))**2)
    col = np.arange(npix)[:, None] + offs[None, :]
    t[(col < 0) | (col >= npix)] = 0.0
    return t / t.sum(axis=1)[:, None]


def pad_taps(taps, nd):
    """the same matrix with zero diagonals added on both sides: [..., npix, nd]"""
    taps = np.asarray(taps)
    w = (nd - taps.shape[-1]) // 2
    assert w >= 0 and taps.shape[-1] + 2 * w == nd
    out = np.zeros(taps.shape[:-1] + (nd, ))
    out[..., w:w + taps.shape[-1]] = taps
    return out


def taps_from_sparse(R, nd):
    """row taps [n, nd] of a scipy.sparse matrix that lies inside nd diagonals"""
    R = R.tocoo()
    m = (nd - 1) // 2
    out = np.zeros((R.shape[0], nd))
    o = R.col - R.row
    assert np.all(np.abs(o[R.data != 0]) <= m)
    keep = np.abs(o) <= m
    np.add.at(out, (R.row[keep], o[keep] + m), R.data[keep])
    return out


def taps_to_sparse(taps):
    import scipy.sparse
    npix, nd = taps.shape
    m = (nd - 1) // 2
    k, d = np.meshgrid(np.arange(npix), np.arange(nd), indexing='ij')
    col = k - m + d
    ok = (col >= 0) & (col < npix)
    assert np.all(taps[~ok] == 0)
    return scipy.sparse.csr_matrix((taps[ok], (k[ok], col[ok])), shape=(npix, npix))


# --------------------------------------------------------------------------
# libraries, templates and synthetic spectra (host, float64)
# --------------------------------------------------------------------------
_libd, _olib, _rec = {}, {}, {}


def lib_dict(key):
    """'gold_b', 'gold_r', or 'gold_b_lin': gold_b's rows on a LINEAR knot grid
    (the construction of test_gpu_parity._linear_grid_config)"""
    if key not in _libd:
        n = key[:6]
        d = dict(np.load(os.path.join(GOLD, 'lib_%s.npz' % n)))
        d.update(np.load(os.path.join(GOLD, 'lib_nocont_%s.npz' % n)))
        if key.endswith('_lin'):
            ll = np.asarray(d['lam'], dtype=np.float64)
            d['lam'] = np.linspace(ll[0], ll[-1], len(ll))
            d['log_step'] = np.array(False)
        _libd[key] = d
    return _libd[key]


def oracle_lib(key):
    from oracle import rvs_oracle as orc
    if key not in _olib:
        _olib[key] = orc.Library(lib_dict(key))
    return _olib[key]


def host_records(key, params):
    """records [Tn, ntp, 4] of the oracle's templates at `params` (a row that is
    not finite in the oracle stays NaN), knots"""
    lib = oracle_lib(key)
    out = []
    for p in np.atleast_2d(params):
        k = (key, tuple(float(_) for _ in p))
        if k not in _rec:
            with np.errstate(all='ignore'):
                bad = not np.isfinite(lib.outside_flag(p))
            if bad:
                _rec[k] = np.full((len(lib.lam), 4), np.nan)
            else:
                assert lib.outside_flag(p) == 0, p
                _rec[k] = power_form(lib.lam, lib.eval(p))
        out.append(_rec[k])
    return np.stack(out), lib.lam


PARAMS = np.array([(6123., 2.5, -0.4, 0.1), (5100., 2.3, -0.9, 0.15),
                   (4800., 3.4, -1.5, 0.3), (6800., 1.6, -0.2, 0.05)])
SNR = 30.0


def synth(coef, knots, lam, taps, vel, seed, snr=SNR):
    """a template through the band at a known velocity, times a smooth continuum,
    plus seeded noise -> spec, espec"""
    t = model(coef, knots, lam, taps, [vel])[0].astype(np.float64)
    x = np.linspace(-1, 1, len(lam))
    m = t * (1 + 0.2 * x + 0.1 * np.cos(3 * x))
    es = np.abs(m) / snr
    rng = np.random.RandomState(seed)
    return m + es * rng.standard_normal(len(lam)), es


def golden_lam(name):
    c = np.load(os.path.join(GOLD, 'cases.npz'))
    return np.asarray(c['c1/%s/lam' % name], dtype=np.float64)


# --------------------------------------------------------------------------
# the inputs of sweeps A-F
# --------------------------------------------------------------------------
A_NPIX = (2, 3, 5, 6, 7, 11, 12, 13, 23, 24, 25, 37)
B_SHAPES = ((1, 17), (63, 9), (64, 8), (65, 7), (255, 1), (256, 2), (257, 3),
            (321, 9))
C_BASES = tuple((n, True) for n in range(1, 17)) + ((7, False), (16, False))


def truth_key(band):
    """'nd11as13' is the 11-diagonal matrix zero-padded to 13: one truth"""
    return band.split('as')[0]


def _arm(libkey, grids, gid, nds, params, spec_templ, spec_vel, seed, one=False):
    """an arm of S = len(spec_templ) spectra.  grids: list of wavelength arrays,
    gid[s] the grid of spectrum s.  nds: {band key: nd, or a list of S nd (the
    batch's band is the widest)}; the spectra are made with the first band."""
    coef, knots = host_records(libkey, params)
    S = len(spec_templ)
    npix = max(len(g) for g in grids)
    bands = {}
    for ib, (bk, nd) in enumerate(nds.items()):
        per = nd if isinstance(nd, (list, tuple)) else [nd] * S
        wide = max(per)
        t = np.zeros((S, npix, wide))
        for s in range(S):
            n = len(grids[gid[s]])
            t[s, :n] = pad_taps(band_taps(n, per[s], seed + 101 * ib +
                                          (0 if one else 7 * s)), wide)
        bands[bk] = t[:1] if one else t
    first = next(iter(bands))
    spec = np.zeros((S, npix))
    espec = np.full((S, npix), np.inf)
    for s in range(S):
        lam = grids[gid[s]]
        n = len(lam)
        tp = bands[first][0 if one else s, :n]
        spec[s, :n], espec[s, :n] = synth(coef[spec_templ[s]], knots, lam, tp,
                                          spec_vel[s], seed + 1000 + s)
    name = libkey[:6]
    return dict(lib=libkey, name=name, grids=grids, gid=list(gid), spec=spec,
                espec=espec, bands=bands)


def _with_padded(arm, src, nd):
    arm['bands']['%sas%d' % (src, nd)] = pad_taps(arm['bands'][src], nd)


def _case(name, arms, npoly, rbf, params, job_spec, job_templ, vels):
    return dict(name=name, arms=arms, npoly=npoly, rbf=rbf,
                params=np.atleast_2d(params),
                job_spec=np.asarray(job_spec, dtype=np.int32),
                job_templ=np.asarray(job_templ, dtype=np.int32),
                vels=np.asarray(vels, dtype=np.float64))


_cases = {}


def cases():
    """{name: case} of sweeps A-F, the same on every machine"""
    if _cases:
        return _cases
    lb, lr = golden_lam('gold_b'), golden_lam('gold_r')
    out = []
    # A: pixel-loop tails
    for npix in A_NPIX:
        a = _arm('gold_b', [lb[100:100 + npix].copy()], [0, 0],
                 dict(nd11=11, nd3=3, nd33=33), PARAMS[:2], [0, 1], [-50., 40.],
                 seed=npix)
        _with_padded(a, 'nd11', 13)
        out.append(_case('A-%d' % npix, [a], min(npix, 3), True, PARAMS[:2],
                         [1, 0], [0, 1], np.linspace(-280., 290., 5)))
    # B: velocity and job tails
    ab = _arm('gold_r', [lr], [0, 0, 0], dict(nd11=11, nd9=9), PARAMS, [0, 2, 3],
              [-120., 15., 210.], seed=50)
    _with_padded(ab, 'nd11', 13)
    for Nv, J in B_SHAPES:
        j = np.arange(J)
        js, jt = (7 * j + 2) % 3, (5 * j + 3) % 4
        shared = np.linspace(-300., 300., Nv)
        own = np.stack([np.linspace(-300. + 3.7 * k, 300. - 2.1 * k, Nv) for k in j])
        out.append(_case('B-%dx%d-shared' % (Nv, J), [ab], 5, True, PARAMS, js, jt,
                         shared))
        out.append(_case('B-%dx%d-own' % (Nv, J), [ab], 5, True, PARAMS, js, jt, own))
    # C: every P
    ac = _arm('gold_b', [lb], [0, 0], dict(nd11=11), PARAMS[:2], [1, 0],
              [-200., 77.], seed=60)
    _with_padded(ac, 'nd11', 13)
    for npoly, rbf in C_BASES:
        out.append(_case('C-%d-%s' % (npoly, 'rbf' if rbf else 'cheb'), [ac], npoly,
                         rbf, PARAMS[:2], [1, 0], [0, 1],
                         np.linspace(-310., 295., 70)))
    # D: launch forms
    ad = _arm('gold_r', [lr], [0, 0, 0], dict(nd11=11), PARAMS[:3], [2, 0, 1],
              [-30., 110., -260.], seed=70, one=True)
    ad['bands']['nd11rep'] = np.repeat(ad['bands']['nd11'], 3, axis=0)
    _with_padded(ad, 'nd11', 13)
    ad['bands']['nd11repas13'] = np.repeat(ad['bands']['nd11as13'], 3, axis=0)
    out.append(_case('D-shared-matrix', [ad], 10, True, PARAMS[:3], [2, 0, 1, 1, 0],
                     [0, 1, 2, 0, 2], np.linspace(-310., 295., 70)))
    d2 = [_arm(k, [l], [0, 0], dict(nd11=11), PARAMS[:2], [0, 1], [-75., 130.],
               seed=80 + i) for i, (k, l) in enumerate((('gold_b', lb),
                                                        ('gold_r', lr)))]
    for a in d2:
        _with_padded(a, 'nd11', 13)
    out.append(_case('D-two-arms', d2, 10, True, PARAMS[:2], [1, 0, 0], [0, 1, 0],
                     np.linspace(-310., 295., 70)))
    pn = np.array([PARAMS[0], (-100., 2., -1., 0.2), PARAMS[1]])
    an = _arm('gold_r', [lr], [0, 0], dict(nd11=11), pn, [0, 2], [-75., 130.],
              seed=90)
    _with_padded(an, 'nd11', 13)
    out.append(_case('D-nan-template', [an], 10, True, pn, [1, 0, 1], [0, 1, 2],
                     np.linspace(-310., 295., 70)))
    # E: linear template grid
    ae = _arm('gold_b_lin', [lb], [0, 0], dict(nd11=11), PARAMS[:2], [0, 1],
              [-160., 45.], seed=100)
    _with_padded(ae, 'nd11', 13)
    out.append(_case('E-linear', [ae], 10, True, PARAMS[:2], [1, 0], [0, 1],
                     np.linspace(-310., 295., 70)))
    # F: grid sets
    grids = [lr[:301].copy(), lr[:280].copy(), lr[12:290].copy(), lr[:296].copy()]
    assert [len(g) for g in grids] == [301, 280, 278, 296]
    af = _arm('gold_r', grids, [0, 1, 2, 3], dict(nd11=11, mixed21=[9, 13, 21, 11]),
              PARAMS[:2], [0, 1, 1, 0], [-90., 20., 150., -210.], seed=110)
    out.append(_case('F-grid-set', [af], 10, True, PARAMS[:2], [2, 0, 3, 1],
                     [0, 1, 1, 0], np.linspace(-310., 295., 70)))
    for c in out:
        _cases[c['name']] = c
    return _cases


def case_bands(case):
    return list(case['arms'][0]['bands'])


def job_vels(case, j):
    v = case['vels']
    return v if v.ndim == 1 else v[j]


_polys = {}


def _basis(lam, npoly, rbf):
    from oracle import rvs_oracle as orc
    k = (lam.tobytes(), npoly, rbf)
    if k not in _polys:
        _polys[k] = orc.get_poly_basis(lam, npoly, rbf=rbf)
    return _polys[k]


def evaluate(case, band, records, fn=chisq_grid_truth, jobs=None):
    """fn summed over the arms for every job of `case` -> [J, Nv].  records[ia]:
    (coef [Tn, ntp, 4], knots) of arm ia.  A job whose template is not finite
    gets NaN.  Jobs that share spectrum, template and velocities are computed once."""
    J = len(case['job_spec'])
    Nv = case['vels'].shape[-1]
    out = np.full((J, Nv), np.nan, dtype=LD)
    seen = {}
    for j in (range(J) if jobs is None else jobs):
        s, t = int(case['job_spec'][j]), int(case['job_templ'][j])
        v = job_vels(case, j)
        key = (s, t, v.tobytes())
        if key not in seen:
            tot = np.zeros(Nv, dtype=LD)
            for ia, arm in enumerate(case['arms']):
                coef, knots = records[ia]
                lam = arm['grids'][arm['gid'][s]]
                n = len(lam)
                tp = arm['bands'][band]
                tp = tp[0 if tp.shape[0] == 1 else s, :n]
                tot = tot + fn(coef[t], knots, lam, arm['spec'][s, :n],
                               arm['espec'][s, :n],
                               _basis(lam, case['npoly'], case['rbf']), tp, v)
            seen[key] = tot
        out[j] = seen[key]
    return out


def case_npix(case, j):
    s = int(case['job_spec'][j])
    return sum(len(a['grids'][a['gid'][s]]) for a in case['arms'])


def rel_err(got, truth, npix):
    """|got - truth| / max(|truth|, npix), elementwise (float64)"""
    truth = np.asarray(truth, dtype=LD)
    d = np.abs(np.asarray(got).astype(LD) - truth)
    return (d / np.maximum(np.abs(truth), npix)).astype(np.float64)


def host_case_records(case):
    return [host_records(a['lib'], case['params']) for a in case['arms']]


def emulation_worst(per_case=False):
    """worst error of orthonormal_f64_form against the truth over sweeps A-F"""
    worst = {}
    for name, c in cases().items():
        rec = host_case_records(c)
        w = 0.0
        for band in {truth_key(b) for b in case_bands(c)}:
            if band not in c['arms'][0]['bands']:
                continue
            tr = evaluate(c, band, rec)
            em = evaluate(c, band, rec, fn=orthonormal_f64_form)
            for j in range(len(tr)):
                if np.all(np.isnan(tr[j])):
                    continue       # (the template that is not finite)
                w = max(w, float(np.max(rel_err(em[j], tr[j], case_npix(c, j)))))
        worst[name] = w
    return worst if per_case else max(worst.values())


# --------------------------------------------------------------------------
# sweep H: weightless stretches under a band (the cases of
# test_chisq_accuracy.test_long_weightless_stretches_take_the_robust_path)
# --------------------------------------------------------------------------
H_LAM = np.arange(4400., 4720.1, 0.8)
H_PARAM = (5100., 2.3, -0.9, 0.15)
H_VELS = 30. + 5 * np.arange(4.)
H_SPECTRA = tuple((snr, frac, infl) for snr in (30., 1000.)
                  for frac, infl in ((0.5, 1e4), (0.5, 1e6), (0.7, 1e4), (0.3, 1e6)))
H_NPOLY = (10, 15)
H_ND = (11, 13)


def h_matrix(nd):
    """construct_resol_mat bands of 11 (constant width, pipe kernel) and 13
    (R = 2500, ring kernel) diagonals on H_LAM -> scipy.sparse"""
    from oracle import rvs_oracle as orc
    if nd == 11:
        return orc.construct_resol_mat(H_LAM, width=0.75).tocsr()
    assert nd == 13
    return orc.construct_resol_mat(H_LAM, resol=2500.).tocsr()


def h_spectra(nd):
    """spec, espec [8, npix] in the order of H_SPECTRA: the template through the
    band at 30 km/s plus noise, the red part of the arm with inflated errors"""
    coef, knots = host_records('gold_b', [H_PARAM])
    taps = taps_from_sparse(h_matrix(nd), nd)
    sp0 = model(coef[0], knots, H_LAM, taps, [30.])[0].astype(np.float64)
    spec, espec = [], []
    for snr, frac, infl in H_SPECTRA:
        rng = np.random.RandomState(1)
        es = sp0 / snr
        spec.append(sp0 + es * rng.standard_normal(len(H_LAM)))
        es = es.copy()
        es[int(len(H_LAM) * (1 - frac)):] *= infl
        espec.append(es)
    return np.stack(spec), np.stack(espec), taps


def h_evaluate(nd, npoly, coef, knots, fn=chisq_grid_truth):
    """[8, 4]: fn for every spectrum of h_spectra(nd) at H_VELS"""
    spec, espec, taps = h_spectra(nd)
    polys = _basis(H_LAM, npoly, True)
    return np.stack([fn(coef, knots, H_LAM, spec[i], espec[i], polys, taps, H_VELS)
                     for i in range(len(spec))])


def h_emulation_errors():
    coef, knots = host_records('gold_b', [H_PARAM])
    out = {}
    for nd in H_ND:
        for npoly in H_NPOLY:
            tr = h_evaluate(nd, npoly, coef[0], knots)
            with np.errstate(all='ignore'):
                em = h_evaluate(nd, npoly, coef[0], knots, fn=orthonormal_f64_form)
            for i, (snr, frac, infl) in enumerate(H_SPECTRA):
                out[(snr, frac, infl, npoly, nd)] = float(
                    np.max(rel_err(em[i], tr[i], len(H_LAM))))
    return out


def h_must_flag():
    return sorted(k for k, v in H_EMULATION.items() if v > H_FLAG_ABOVE)
