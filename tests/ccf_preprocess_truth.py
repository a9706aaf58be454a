"""Stage-by-stage truth of ccf_preprocess_kernel (csrc/ccf.hip; rvs_ccf_preprocess,
rvs_ccf_preprocess_g), numpy and np.longdouble only.

A plain restatement of make_ccf.preprocess_data (make_ccf.py:105-164, 288-414; the
project's float64 restatement is oracle/rvs_oracle.py:676-778), cut into stages so that
each can be checked from the DEVICE's own upstream outputs: the one quantity that holds
an optimiser's stopping point (pfit) does not loosen the stages after it.

Inputs are the arrays the C entry takes.  The tables (Eb, El, Cinv | C, istart,
bin_start, xind, rw) come from the host functions of rvspecfit_amd/ccf_tables.py, which
tests/test_ccf_tables_cpu.py and tests/test_tables_gpu.py pin to the reference and to
the device builder.

Scope: flux and errors are finite, or the errors are +inf.  NaN flux and NaN errors are
out of scope: scipy's medfilt and least_squares leave them unspecified or raise.

Stages, and what each is held to
--------------------------------
masks (exact).  mederr = np.nanmedian(espec), an order statistic or the mean of two.
    medfilt11 is a sort of the eleven zero-padded taps.  mask = badmask | (espec >
    maxerr mederr) | (medfilt11 <= 0); with continuum = 0 it is badmask alone.  The
    mask is read back as the zero pattern of proc_spec / proc_ivar: a masked pixel
    gives c = 0 and iv = 0 exactly, and on a `pixels` FFT grid (one FFT point per
    pixel, rw = 0; the last point rw = 1) proc_spec[n] = c[n] bit for bit and
    proc_ivar[n] = 0 exactly where pixel n or n + 1 is masked.  RVS_ST_ALLMASKED exact.

filled spectrum, medv (through their consequences).  interp_masker's formula has two
    products and a sum that the compiler may contract, so a filled pixel may differ
    from numpy's by an ulp; it carries an error of 1e9 mederr, so nothing downstream
    sees that but a bin median that lands on a filled pixel (below).  medv decides the
    floor of the continuum: where exp(S) and the floor differ by 1e-6 relative or more
    the branch is compared exactly (the two pixel sets cont_given_pfit returns).

binned start (fit = 'gtol').  With errors 1e12 x the flux level the kernel leaves at
    its gtol test and pfit = C (C^-1 p0): the two median paths (a wave's bisection for
    bins of <= 256 pixels, the block-wide selection above) and the empty-bin rule are
    seen undiluted.  p0 = log(max(np.median(bin), 1e-3 med)), log(med) for an empty
    bin.  Bound  |pfit - p0|_inf <= 8 eps cond(C) max|p0|,  cond(C) = |C|_inf
    |C^-1|_inf:  c = fl(C^-1 p0) and p = fl(C c) are fma chains.  A row of C has three
    non-zero entries (3 eps |C||c|); a row of C^-1 has m, but they fall off
    geometrically from the diagonal, so a handful of terms carry the sum (about 4 eps
    |C^-1||p0| where the worst case of an m-term chain is (m + 1) eps); together
    |dp| <= (3 + 4) eps |C||C^-1||p0|, and one more eps for log and for a median that
    lands on a filled pixel (eps max(1, |p0|), inside eps cond max|p0| for max|p0|
    >= 1: the cases keep the flux level away from 1 for that reason).  Measured: the
    emulation and the device both stay below 0.1 of the bound.
    12 pixels under 24 nodes (empty knot intervals, more unknowns than pixels): the
    minimiser is not unique, so the full fit there (fit = None) is held only to
    "the objective does not rise" and to the stages after it; the binned start is
    held through the gtol exit like every other.

the fit (fit = 'newton').  p* = argmin sum_k (sqrt(1 + f_k^2) - 1), f = (exp(clip(S(p),
    +-100)) - s) / e, by Newton's method with the full Hessian in longdouble from the
    device's pfit (on the CPU: from the emulation's end point) until the step is below
    1e-17; more than 50 iterations fail.  Asserted: d = |pfit - p*|_inf (log flux)
    <= the largest distance d_trf, over the family's cases, of the REFERENCE's own
    optimiser from p*: scipy.optimize.least_squares(loss='soft_l1') at its default
    tolerances from the same p0 on the same objective.  No margin on top.  A float64
    emulation of the kernel's schedule (lambda0 1e-3, / 8 on accept, x 4 on reject,
    stop at step < 1e-9 or relative decrease < 1e-12, Gauss-Newton weights as in
    lm_normal) must stay 10 x inside that on every case (CPU test).
    fit = None: the masked stretch is so long that the Hessian's condition is that of
    the masked errors squared (1e18 and more); d means nothing there and only the
    stages before and after the fit are held.

cont given pfit.  c' = C^-1 pfit_dev, S = E c', cont = exp(clip(S)), floored, all in
    longdouble.  The device holds c, writes pfit = fl(C c) and evaluates E c: the two
    differ by the rounding of C c mapped back, |C^-1| (m + 1) eps |C| |c|, plus the
    three-term fma chain (3 eps sum |Eb c|), the exponent's error times 1 (d exp = exp
    dS), exp itself and the product of the floor (4 eps):
        |cont_dev / cont - 1| <= eps (4 |E||c'| + (m + 2) |E| |C^-1| |C| |c'| + 4)
    of the order eps (|S| + cond(C) max|p|), and independent of where the fit stopped.

proc_spec, proc_ivar, sse given cont.  From the device's cont, the mask, the inflated
    errors and xind / rw in longdouble.  c = s / cont (1 rounding), iv = cont cont (1 /
    (e e)) (4); r1 = lw c_i + rw c_{i+1}: <= 4 eps (|lw c_i| + |rw c_{i+1}|), products
    contracted or not; r2 = a b / (lw^2 b + rw^2 a + [a b == 0]): all terms >= 0, 24
    eps relative (4 + 4 numerator and product, 2 + 4 + 1 per denominator term, the
    sum, the division).  (a b) == 0 and xind < 0 give exact zeros.  sse = sum r1^2 r2
    over the device's own r1, r2: (nfft / 512 + 16) eps of the sum, every term >= 0
    (three roundings a term, a serial chain of nfft / 512 terms a thread, a 9-level
    tree).
"""
import functools

import numpy as np

from rvspecfit_amd import ccf_tables as ct

LD = np.longdouble
EPS = 2.0 ** -52
ST_ALLMASKED = 0x40
NEWTON_TOL = 1e-17
NEWTON_MAXIT = 50
BRANCH_MARGIN = 1e-6

# Measured, per family: (largest TRF distance d_trf = the asserted bound, the float64
# emulation's largest d, the device's largest d on an MI355X).  scipy 1.15; nothing is
# asserted against the third column.  The arm at the LDS limit (6247 pixels, 24 nodes)
# belongs to `npix`: TRF 5.4e-9, emulation 3.6e-9, device 3.6e-9.
MEASURED = {
    'npix': (1.5e-05, 1.1e-07, 1.1e-07),
    'nodes': (1.36e-05, 9.22e-08, 9.22e-08),
    'bins': (2.13e-08, 3.92e-10, 3.92e-10),
    'scale': (5.52e-09, 1.57e-11, 1.54e-11),
    'medv': (2.95e-05, 2.02e-07, 2.02e-07),
    'masks': (4.2e-08, 1.26e-10, 1.26e-10),
    'oracle': (1.07e-09, 4.25e-12, 4.25e-12),
    'grids': (1.96e-06, 3.98e-09, 3.98e-09),
    'models': (2.18e-06, 2.3e-08, 2.3e-08),
}
# Device value / a-priori bound, worst over all launches (MI355X): binned start (gtol
# exit) 0.081, cont given pfit 0.104, proc_spec 0.333, proc_ivar 0.095, sse 0.049;
# template rows: cont 0.112, model values 0.055.


# ------------------------------------------------------------------ geometry
def lam_of(x):
    """pixel coordinate -> wavelength (log-uniform, 30 km/s a pixel)"""
    return 4000.0 * np.exp(1e-4 * np.asarray(x, dtype=np.float64))


def _edges_for(sizes, first=0):
    """bin edges (wavelength) that put sizes[j] pixels into bin j, from pixel `first`
    on; an empty bin is a pair of edges between two pixels"""
    x, out = first - 0.5, []
    out.append(x)
    for n in sizes:
        if n == 0:
            # an edge a sixteenth of a pixel on, still in front of the next pixel
            x = x + 1.0 / 16
        else:
            x = np.floor(x + 0.5) + n - 0.5
        out.append(x)
    return lam_of(np.array(out))


def fft_span(L):
    """(logl0, logl1) of the FFT grid of launch L"""
    lam = L['lam']
    l0, l1 = np.log(lam[0]), np.log(lam[-1])
    w = l1 - l0
    g = L['grid']
    if g == 'inside':
        return l0 + 0.1 * w, l1 - 0.15 * w
    if g == 'wider':
        return l0 - 0.2 * w, l1 + 0.3 * w
    assert g == 'disjoint'
    return l1 + 0.5 * w, l1 + 2 * w


def _fft_tables(L):
    lam, nfft, npix = L['lam'], L['nfft'], len(L['lam'])
    g = L['grid']
    if g == 'pixels':
        assert nfft == npix
        xi = np.minimum(np.arange(npix), npix - 2).astype(np.int32)
        rw = np.zeros(npix)
        rw[-1] = 1.0
        return xi, rw
    a, b = fft_span(L)
    return ct.rebin_tables(lam, a, b, nfft)


_tables = {}


def tables(L):
    """the arrays of the C entry for launch L (host functions of ccf_tables only)"""
    if L['name'] in _tables:
        return _tables[L['name']]
    T = {}
    T['xind'], T['rw'] = _fft_tables(L)
    if L['continuum']:
        Eb, El, Cinv, istart = ct.interp_spline_tables(L['nodes'], L['lam'])
        m = len(L['nodes'])
        C = np.linalg.inv(Cinv)
        T.update(Eb=np.ascontiguousarray(Eb), El=El, Cinv=Cinv, C=C,
                 CinvC=np.concatenate([Cinv.ravel(), C.ravel()]),
                 istart=istart[:m - 1].astype(np.int32),
                 bin_start=ct.bin_ranges(L['lam'], L['edges']))
        E = np.zeros((len(L['lam']), m), dtype=LD)
        for q in range(3):
            E[np.arange(len(El)), El + q] = Eb[:, q]
        T['E'] = E
        T['A'] = E @ Cinv.astype(LD)
        T['cond'] = float(np.abs(C).sum(1).max() * np.abs(Cinv).sum(1).max())
    _tables[L['name']] = T
    return T


# ------------------------------------------------------------------ the stages
def medfilt11(s):
    pad = np.concatenate([np.zeros(5), s, np.zeros(5)])
    win = np.stack([pad[q:q + len(s)] for q in range(11)], axis=1)
    return np.sort(win, axis=1)[:, 5]


def stage_masks(L, i):
    s, e = L['spec'][i], L['espec'][i]
    bad = np.zeros(len(s), bool) if L['badmask'] is None else L['badmask'][i] != 0
    mederr = np.nanmedian(e)
    mask = bad.copy()
    if L['continuum']:
        mask |= (e > L['maxerr'] * mederr) | (medfilt11(s) <= 0)
    return mederr, mask


def stage_fill(L, i, mask, mederr, edge='copy'):
    """interp_masker (make_ccf.py:288-327) and the inflated errors.  edge='interp' is
    a deliberately wrong restatement (the CPU test's mutation)"""
    lam, s = L['lam'], L['spec'][i]
    ce = L['espec'][i].copy()
    ce[mask] = 1e9 * mederr
    cs = s.copy()
    good = np.nonzero(~mask)[0]
    if len(good) == 0:
        cs[~np.isfinite(cs)] = 1
        return cs, ce, ST_ALLMASKED
    for k in np.nonzero(mask)[0]:
        j = np.searchsorted(good, k)
        if j == 0 or j == len(good):
            if edge == 'interp' and len(good) > 1:
                a, c = (good[0], good[1]) if j == 0 else (good[-2], good[-1])
            else:
                cs[k] = s[good[0]] if j == 0 else s[good[-1]]
                continue
        else:
            a, c = good[j - 1], good[j]
        l1, l2, l0 = lam[a], lam[c], lam[k]
        cs[k] = (-(l1 - l0) * s[c] + (l2 - l0) * s[a]) / (l2 - l1)
    return cs, ce, 0


def stage_medv(cs):
    medv = np.median(cs)
    med = medv
    if med <= 0:
        med = abs(med)
        if med == 0:
            med = 1.0
    return medv, med


def stage_p0(L, cs, med, rank_shift=0):
    """binned medians (make_ccf.py:141-143).  rank_shift = 1: a wrong restatement"""
    bs = tables(L)['bin_start']
    m = len(L['nodes'])
    p0 = np.zeros(m)
    for j in range(m):
        v = np.sort(cs[bs[j]:bs[j + 1]])
        if len(v) == 0:
            p0[j] = np.log(med)
            continue
        if rank_shift:
            stat = v[min(len(v) // 2 + rank_shift, len(v) - 1)]
        else:
            stat = np.median(v)
        p0[j] = np.log(max(stat, 1e-3 * med))
        if not np.isfinite(p0[j]):
            p0[j] = np.log(med)
    return p0


def upstream(L, i, **kw):
    """everything in front of the fit for spectrum i of launch L"""
    mederr, mask = stage_masks(L, i)
    cs, ce, st = stage_fill(L, i, mask, mederr, edge=kw.get('edge', 'copy'))
    medv, med = stage_medv(cs)
    out = dict(mederr=mederr, mask=mask, cs=cs, ce=ce, status=st, medv=medv, med=med)
    if L['continuum']:
        out['p0'] = stage_p0(L, cs, med, rank_shift=kw.get('rank_shift', 0))
    return out


_up = {}


def truth(L, i):
    key = (L['name'], i)
    if key not in _up:
        _up[key] = upstream_model(L, i) if L.get('model') else upstream(L, i)
    return _up[key]


def p0_bound(L, p0):
    return 8 * EPS * tables(L)['cond'] * float(np.abs(p0).max())


# ------------------------------------------------------------------ the minimiser
def _solve_ld(H, b):
    """Gaussian elimination with partial pivoting in longdouble"""
    n = len(b)
    M = np.concatenate([H.astype(LD), b.astype(LD)[:, None]], axis=1)
    for c in range(n):
        piv = c + int(np.argmax(np.abs(M[c:, c])))
        if piv != c:
            M[[c, piv]] = M[[piv, c]]
        M[c + 1:] -= np.outer(M[c + 1:, c] / M[c, c], M[c])
    x = np.zeros(n, dtype=LD)
    for c in range(n - 1, -1, -1):
        x[c] = (M[c, n] - M[c, c + 1:n] @ x[c + 1:]) / M[c, c]
    return x


def objective(A, s, e, p, drop=None):
    """cost, gradient and full Hessian of sum (sqrt(1 + f^2) - 1) in longdouble.
    drop: a pixel left out of the gradient (a wrong restatement, CPU test)"""
    S = A @ p.astype(LD)
    clipped = np.abs(S) > 100
    mod = np.exp(np.clip(S, -100, 100))
    f = (mod - s) / e
    r = np.sqrt(1 + f * f)
    d = np.where(clipped, 0, mod / e)
    gw = f / r * d
    if drop is not None:
        gw = gw.copy()
        gw[drop] = 0
    w = d * d / (r * r * r) + f / r * d
    # (sqrt(1 + z) - 1 as z / (1 + sqrt(1 + z)): no cancellation under huge errors)
    return (f * f / (1 + r)).sum(), A.T @ gw, (A * w[:, None]).T @ A


def newton(L, i, p_start, drop=None):
    """p*, iterations, |gradient|_inf; raises if it does not converge"""
    t, A = truth(L, i), tables(L)['A']
    s, e = t['cs'].astype(LD), t['ce'].astype(LD)
    p = np.asarray(p_start, dtype=LD).copy()
    for it in range(1, NEWTON_MAXIT + 1):
        _, g, H = objective(A, s, e, p, drop)
        step = _solve_ld(H, -g)
        p = p + step
        if float(np.abs(step).max()) < NEWTON_TOL:
            _, g, _ = objective(A, s, e, p, drop)
            return p, it, float(np.abs(g).max())
    raise AssertionError('Newton did not converge: %s[%d], last step %.3g' %
                         (L['name'], i, float(np.abs(step).max())))


def _resid64(L, i):
    t, A64 = truth(L, i), tables(L)['A'].astype(np.float64)
    s, e = t['cs'], t['ce']
    return lambda p: (np.exp(np.clip(A64 @ p, -100, 100)) - s) / e


_trf = {}


def trf(L, i):
    """the reference's optimiser (make_ccf.py:146-150) on the same objective"""
    import scipy.optimize
    key = (L['name'], i)
    if key not in _trf:
        _trf[key] = scipy.optimize.least_squares(_resid64(L, i), truth(L, i)['p0'],
                                                 loss='soft_l1')['x']
    return _trf[key]


def emulate(L, i, drop=None):
    """float64 emulation of lm_fit's schedule (dense algebra in place of the banded
    one).  Returns pfit = C c.  drop: a pixel left out of the normal equations"""
    T, t = tables(L), truth(L, i)
    E = T['E'].astype(np.float64)
    Cinv, C = T['Cinv'], T['C']
    s, e = t['cs'], t['ce']

    def ev(c):
        S = E @ c
        clipped = np.abs(S) > 100
        mod = np.exp(np.clip(S, -100, 100))
        f = (mod - s) / e
        return 0.5 * np.sum(2 * (np.sqrt(1 + f * f) - 1)), np.where(clipped, 0.0, mod)

    c = Cinv @ t['p0']
    lamd = 1e-3
    cost, wm = ev(c)
    for it in range(60):
        f = (wm - s) / e
        r = np.sqrt(1 + f * f)
        d = wm / e
        h, gg = d * d / (r * r * r), d * f / r
        if drop is not None:
            h, gg = h.copy(), gg.copy()
            h[drop] = gg[drop] = 0
        B, b = E.T @ (h[:, None] * E), E.T @ gg
        if it == 0 and np.abs(Cinv.T @ b).max() < 1e-8:
            break
        accepted = stop = False
        for _ in range(40):
            M = B + lamd * np.diag(np.diag(B))
            try:
                np.linalg.cholesky(M)
                dl = np.linalg.solve(M, -b)
            except np.linalg.LinAlgError:
                dl = np.zeros_like(b)
            cn, wmn = ev(c + dl)
            if cn <= cost:
                accepted = True
                rel = (cost - cn) / max(cost, 1e-300)
                c, wm, lamd = c + dl, wmn, max(lamd / 8, 1e-12)
                if np.abs(dl).max() < 1e-9 or rel < 1e-12:
                    stop = True
                cost = cn
                break
            lamd *= 4
            if lamd > 1e12:
                stop = True
                break
        if stop:
            break
        if not accepted:
            cost, wm = ev(c)
    return C @ c


def family_bound(family):
    """the largest TRF distance from p* over the family's fitted cases"""
    worst = 0.0
    for L in by_family(family):
        if L['fit'] != 'newton':
            continue
        for i in range(L['B']):
            if i in L.get('nofit', ()):
                continue
            x = trf(L, i)
            pstar, _, _ = newton(L, i, x)
            worst = max(worst, float(np.abs(x - pstar).max()))
    return worst


_fb = {}


def bound_of(family):
    if family not in _fb:
        _fb[family] = family_bound(family)
    return _fb[family]


# ------------------------------------------------------------------ after the fit
def raw_cont(L, pfit):
    """exp(clip(E C^-1 pfit)) in longdouble and its relative rounding bound"""
    T = tables(L)
    m = len(L['nodes'])
    c = T['Cinv'].astype(LD) @ np.asarray(pfit, dtype=LD)
    aE = np.abs(T['E'])
    raw = np.exp(np.clip(T['E'] @ c, -100, 100))
    spread = np.abs(T['Cinv']).astype(LD) @ (np.abs(T['C']).astype(LD) @ np.abs(c))
    return raw, EPS * (4 * (aE @ np.abs(c)) + (m + 2) * (aE @ spread) + 4)


def cont_given_pfit(L, i, pfit):
    """(cont, relative bound, floored-by-margin, free-by-margin) in longdouble from
    the device's pfit (continuum = 0: cont 1 or its floor, bound 2 eps)"""
    t = truth(L, i)
    npix = len(L['lam'])
    if L['continuum']:
        raw, bound = raw_cont(L, pfit)
    else:
        raw = np.ones(npix, dtype=LD)
        bound = np.full(npix, 2 * EPS, dtype=LD)
    floor = LD(1e-2 * t['medv']) if t['medv'] > 0 else LD(1)
    cont = np.maximum(raw, floor)
    rel = raw / floor - 1
    return cont, bound, rel < -BRANCH_MARGIN, rel > BRANCH_MARGIN, float(floor)


def proc_given_cont(L, i, cont):
    """proc_spec, proc_ivar and their absolute bounds from the device's cont"""
    t, T = truth(L, i), tables(L)
    mask = t['mask']
    cont = np.asarray(cont, dtype=LD)
    with np.errstate(all='ignore'):
        e = t['ce'].astype(LD)
        c = np.where(mask, 0, L['spec'][i].astype(LD) / cont)
        iv = np.where(mask, 0, cont * cont * (1 / (e * e)))
    xi, rw = T['xind'], T['rw'].astype(LD)
    lw = (1 - T['rw']).astype(LD)        # the float64 difference, as the kernel's
    ok = xi >= 0
    j = np.where(ok, xi, 0)
    t1, t2 = lw * c[j], rw * c[j + 1]
    r1 = np.where(ok, t1 + t2, 0)
    b1 = np.where(ok, 4 * EPS * (np.abs(t1) + np.abs(t2)), 0)
    a, b = iv[j], iv[j + 1]
    zero = (a * b) == 0
    r2 = np.where(ok, a * b / (lw * lw * b + rw * rw * a + zero), 0)
    b2 = 24 * EPS * r2
    return r1, b1, r2, b2


def sse_given_proc(r1, r2):
    r1, r2 = np.asarray(r1, dtype=LD), np.asarray(r2, dtype=LD)
    s = (r1 * r1 * r2).sum()
    return s, (len(r1) / 512 + 16) * EPS * s


def ratio(got, want, bound):
    """|got - want| / bound; 0 where both are equal (a zero bound then passes)"""
    err = np.abs(np.asarray(got, dtype=LD) - want)
    with np.errstate(all='ignore'):
        r = np.where(err == 0, 0, err / bound)
    return float(np.max(r)) if np.size(r) else 0.0


# ------------------------------------------------------------------ the cases
def _flux(npix, seed, snr=30.0, level=100.0, lines=True):
    rng = np.random.default_rng(seed)
    x = np.arange(npix) / max(npix - 1, 1)
    f = 1 + 0.3 * x - 0.25 * x * x + 0.05 * np.sin(7 * x + seed)
    if lines:
        for _ in range(max(1, npix // 100)):
            c, w = rng.uniform(0, 1), rng.uniform(1, 3) / npix
            f *= 1 - rng.uniform(0.1, 0.6) * np.exp(-0.5 * ((x - c) / w) ** 2)
    sig = (1 + 0.2 * rng.uniform(size=npix)) / snr
    return level * (f + sig * rng.standard_normal(npix)), level * sig


def _gtol_err(s):
    """errors that dwarf the flux: the kernel leaves at its gtol test"""
    return np.full(len(s), 1e12 * max(float(np.median(np.abs(s))), 1e-300))


def _mk(name, family, npix, nnode, spectra, fit, continuum=1, nfft=64, grid='wider',
        sizes=None, maxerr=10.0, first=0, node_x=None, splinestep=None, x0=0):
    """one launch: B spectra on one arm.  spectra: (spec, espec, badmask or None).
    Nodes: nnode of them, uniform over the arm, or at the pixel coordinates node_x, or
    the reference's own for `splinestep` (make_ccf.py:123-131; then the oracle's
    preprocess_data applies as a whole)"""
    lam = lam_of(x0 + np.arange(npix))
    nodes = lam_of(x0 + (np.linspace(0, npix - 1, nnode) if node_x is None else
                         np.asarray(node_x, dtype=np.float64)))
    assert len(nodes) == nnode
    if splinestep is not None:
        nodes, edges = ct.continuum_nodes(lam, splinestep)
        assert len(nodes) == nnode
    elif sizes is None:
        h = (npix - 1) / (nnode - 1)
        edges = lam_of(x0 + (np.arange(nnode + 1) - 0.5) * h)
    else:
        assert len(sizes) == nnode and x0 == 0
        edges = _edges_for(sizes, first)
    any_mask = any(b is not None for _, _, b in spectra)
    bad = None
    if any_mask:
        bad = np.stack([np.zeros(npix, np.uint8) if b is None else
                        np.asarray(b, np.uint8) for _, _, b in spectra])
    return dict(name=name, family=family, lam=lam, nodes=nodes, edges=edges,
                continuum=continuum, nfft=nfft, grid=grid, maxerr=maxerr, fit=fit,
                splinestep=splinestep,
                spec=np.stack([np.asarray(s, np.float64) for s, _, _ in spectra]),
                espec=np.stack([np.asarray(e, np.float64) for _, e, _ in spectra]),
                badmask=bad, B=len(spectra))


def _pair(npix, seeds, fit, **kw):
    out = []
    snr = kw.pop('snr', 30.0)
    for j, sd in enumerate(seeds):
        s, e = _flux(npix, sd, snr=snr[j % len(snr)] if isinstance(snr, tuple) else snr,
                     **kw)
        out.append((s, _gtol_err(s) if fit == 'gtol' else e, None))
    return out


def _build():
    Ls = []
    # ---- pixel counts x FFT grids: nodes every ~ 60 pixels, at least 3 ------------
    grids = ['inside', 'wider', 'disjoint', 'pixels']
    nffts = [2, 64, 513, 8192]
    for n, npix in enumerate((12, 13, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025,
                              1537)):
        nnode = min(24, max(3, npix // 60))
        g = grids[n % 4]
        nfft = npix if g == 'pixels' else nffts[n % 4 if npix > 13 else 0]
        Ls.append(_mk('npix-%d' % npix, 'npix', npix, nnode,
                      _pair(npix, (n, 100 + n, 200 + n, 300 + n), 'newton',
                            lines=npix > 64, snr=(30.0, 300.0, 3.0, 100.0)),
                      'newton', nfft=nfft, grid=g))
        Ls.append(_mk('npix-%d-gtol' % npix, 'start', npix, nnode,
                      _pair(npix, (n, ), 'gtol'), 'gtol', nfft=nffts[(n + 1) % 4],
                      grid=grids[(n + 1) % 3]))
    for g, nfft in (('disjoint', 64), ('wider', 8192), ('inside', 513)):
        Ls.append(_mk('fft-%s' % g, 'npix', 700, 6, _pair(700, (7, ), 'newton'),
                      'newton', nfft=nfft, grid=g))
    # ---- node counts and interval sizes --------------------------------------------
    for nnode, h in ((3, 40), (4, 40), (5, 600), (5, 40), (23, 63.5), (24, 64.5),
                     (6, 255.5), (6, 256.5), (24, 1.0)):
        npix = int(round((nnode - 1) * h)) + 1
        Ls.append(_mk('nodes-%d-h%g' % (nnode, h), 'nodes', npix, nnode,
                      _pair(npix, (nnode, 50 + nnode, 150 + nnode), 'newton',
                            lines=h > 30, snr=(100.0, 300.0, 10.0) if h < 2 else
                            (30.0, 300.0, 3.0)),
                      'newton', nfft=64))
    # more nodes than pixels: empty knot intervals, no unique minimiser
    Ls.append(_mk('nodes-24-npix-12', 'start', 12, 24, _pair(12, (3, ), 'gtol'),
                  'gtol', nfft=2))
    Ls.append(_mk('nodes-24-npix-12-fit', 'start', 12, 24,
                  _pair(12, (4, ), 'newton', lines=False), None, nfft=64))
    # an empty knot interval in a well-posed fit: three nodes inside one pixel put two
    # knots between pixels 150 and 151
    Ls.append(_mk('nodes-empty-interval', 'nodes', 300, 9,
                  _pair(300, (8, 9), 'newton'), 'newton', nfft=64,
                  node_x=[0, 60, 120, 150.0, 150.6, 150.8, 200, 260, 299]))
    # ---- bin sizes, through the gtol exit and through a full fit --------------------
    bins = {'wave': [0, 1, 2, 64, 65, 256, 100, 7],
            'block': [257, 600, 0, 1, 2, 130],
            'mixed': [256, 257, 256, 257, 256]}
    for key, sizes in bins.items():
        npix = sum(sizes) + 9                 # nine pixels beyond the last edge
        for fit in ('gtol', 'newton'):
            sp = _pair(npix, {'wave': (11, 12), 'block': (13, 14),
                              'mixed': (15, 16)}[key], fit)
            if key != 'mixed':
                # plateaus and quantised values; a bin far below the 1e-3 med floor
                s, e, _ = sp[1]
                s = np.round(s / 4) * 4
                if fit == 'gtol':
                    s[3:3 + (60 if key == 'wave' else 200)] = 0.02
                sp[1] =(s, _gtol_err(s) if fit == 'gtol' else e, None)
            Ls.append(_mk('bins-%s-%s' % (key, fit), 'start' if fit == 'gtol' else
                          'bins', npix, len(sizes), sp, fit, sizes=sizes, first=2,
                          nfft=64))
    # ---- the reference's own nodes: the oracle's preprocess_data applies as a whole -
    so, eo = _flux(900, 41)
    bo = np.zeros(900, np.uint8)
    bo[[0, 1, 400, 401, 402, 899]] = 1
    so2 = so.copy()
    so2[640:646] = -5.0
    Ls.append(_mk('oracle-arm', 'oracle', 900, 6, [(so, eo, bo), (so2, eo, None)],
                  'newton', nfft=513, grid='wider', splinestep=5000.0))
    # ---- three grids of a grid set: pixel count, node count and band all differ ------
    for k, (npix, nnode, x0) in enumerate(((81, 3, 0), (700, 23, 500),
                                           (300, 5, 2000))):
        Ls.append(_mk('grid-%d' % k, 'grids', npix, nnode,
                      _pair(npix, (60 + k, 70 + k, 80 + k), 'newton'), 'newton',
                      nfft=64, grid=('wider', 'inside', 'wider')[k], x0=x0))
    # ---- flux sign and scale --------------------------------------------------------
    npix = 300
    s, e = _flux(npix, 21)
    sp = [(s * 1e-30, e * 1e-30, None), (s * 1e30, e * 1e30, None)]
    Ls.append(_mk('scale-fit', 'scale', npix, 5, sp, 'newton', nfft=64))
    Ls.append(_mk('scale-gtol', 'start', npix, 5,
                  [(a, _gtol_err(a), None) for a, _, _ in sp], 'gtol', nfft=64))
    # a non-positive median of the filled spectrum needs every pixel masked (a good
    # pixel has a positive filtered value): all negative, and 150 negative, 150
    # positive and one 0 under a full badmask (301 pixels: the median is the 0)
    neg = -s
    zero = np.concatenate([-np.abs(s[:150]) - 1, [0.0], np.abs(s[150:]) + 1])
    Ls.append(_mk('sign-gtol', 'start', npix, 5, [(neg, _gtol_err(neg), None)],
                  'gtol', nfft=64))
    Ls.append(_mk('sign-zero-gtol', 'start', npix + 1, 5,
                  [(zero, np.full(npix + 1, 1e14), np.ones(npix + 1, np.uint8))],
                  'gtol', nfft=64))
    # medv against the fitted continuum: a spectrum whose median is 150 x its
    # faint half, so that 1e-2 medv floors the continuum there by a wide margin
    st = np.where(np.arange(npix) < 140, 1.0, 150.0) * (s / 100)
    Ls.append(_mk('medv-floor', 'medv', npix, 5, [(st, np.abs(st) / 30 + 0.01, None),
                                                  (s, e, None)],
                  'newton', nfft=npix, grid='pixels', maxerr=1e6))
    # ---- masks ------------------------------------------------------------------------
    npix = 1100
    s, e = _flux(npix, 31)

    def mk(idx):
        b = np.zeros(npix, np.uint8)
        b[idx] = 1
        return b
    e_eq = e.copy()
    # (two pixels whose errors were above the median already: the median stays)
    k_eq, k_above = (700 + np.nonzero(e[700:] > np.nanmedian(e))[0][:2]).tolist()
    e_eq[k_eq] = 10.0 * np.nanmedian(e)        # exactly maxerr mederr: not masked
    e_eq[k_above] = np.nextafter(10.0 * np.nanmedian(e), np.inf)   # an ulp above: masked
    e_inf = e.copy()
    e_inf[[0, 17, 600, npix - 1]] = np.inf
    s_neg = s.copy()
    s_neg[3] = -1.0                            # the zero padding makes six of eleven
    s_six, s_five = s.copy(), s.copy()
    s_six[500:511:2] = -1.0                    # six of pixels 500..510
    s_five[500:509:2] = 0.0                    # five: masks nothing
    mild = [(s, e, None), (s, e, mk([0])), (s, e, mk([npix - 1])),
            (s, e, mk(slice(0, None, 2))), (s, e, mk(slice(505, 520))),
            (s, e_eq, None), (s, e_inf, None), (s_neg, e, None), (s_six, e, None),
            (s_five, e, None)]
    Ls.append(_mk('masks-mild', 'masks', npix, 8, mild, 'newton', nfft=npix,
                  grid='pixels'))
    Ls.append(_mk('masks-mild-gtol', 'start', npix, 8,
                  [(a, _gtol_err(a), b) for a, _, b in mild[:5]] +
                  [(a, _gtol_err(a), None) for a in (s_neg, s_six, s_five)],
                  'gtol', nfft=npix, grid='pixels'))
    ends = np.r_[0:200, npix - 200:npix]
    s_infm = s.copy()
    s_infm[[5, 900]] = np.inf
    hard = [(s, e, mk(ends)), (s, e, mk(np.r_[0:400, 401:npix])),
            (s, e, mk(np.r_[1:npix - 1])), (s, e, mk(slice(None))),
            (s_infm, e, mk(slice(None)))]
    Ls.append(_mk('masks-hard', 'masks', npix, 8, hard, None, nfft=npix,
                  grid='pixels'))
    Ls.append(_mk('masks-hard-gtol', 'start', npix, 8,
                  [(a, _gtol_err(s), b) for a, _, b in hard[:3]], 'gtol', nfft=513))
    Ls.append(_mk('masks-null', 'masks', npix, 8, [(s, e, None), (s_six, e, None)],
                  'newton', nfft=513, grid='inside'))
    # ---- continuum = 0: badmask only, cont 1 or floored by medv ----------------------
    big = s * 1e3                              # 1e-2 medv = 1000 > 1: floored
    Ls.append(_mk('nocont', 'nocont', npix, 8,
                  [(s / 100, e / 100, None), (big, e * 1e3, mk(ends)),
                   (-s, e, mk([0])), (s_six, e_inf, mk(slice(None))),
                   (s, e_inf, mk([3]))],
                  None, continuum=0, nfft=npix, grid='pixels'))
    Ls.append(_mk('nocont-null', 'nocont', 65, 3, [(s[:65], e[:65], None)], None,
                  continuum=0, nfft=64))
    return Ls


def max_npix():
    """the largest npix rvs_ccf_preprocess_g admits: 24 npix + 16 ceil(npix / 16)
    bytes of dynamic LDS plus the two static structures within 159 KB.  The
    structures' sizes follow from their declarations in csrc/ccf.hip: LMSharedT<24>
    holds 24 (1 + 3 + 1 + 3 + 3 + 9) + 8 + 4 doubles and 7 ints (padded to 8 bytes),
    SelShared 4 + 64 eight-byte words, 512 + 8 + 6 ints."""
    lm = 8 * (24 * 20 + 8 + 4) + 8 * 4
    sel = 8 * 68 + 4 * (512 + 8 + 6)
    sel = (sel + 7) // 8 * 8
    n = (159 * 1024 - lm - sel) // 24
    while 24 * n + (n + 15) // 16 * 16 + lm + sel > 159 * 1024:
        n -= 1
    return n


@functools.lru_cache(None)
def launches():
    Ls = _build()
    names = [L['name'] for L in Ls]
    assert len(set(names)) == len(names)
    return Ls


def largest_arm():
    """the launch at max_npix() (apart from launches(): it is the slow one)"""
    n = max_npix()
    return _mk('npix-max', 'npix', n, 24, _pair(n, (5, ), 'newton'), 'newton',
               nfft=8192, grid='inside')


def by_family(f):
    return [L for L in launches() + model_launches() if L['family'] == f]


def by_name(n):
    return [L for L in launches() + model_launches() if L['name'] == n][0]


# ------------------------------------------------------------------ template rows
# ccf_model_kernel (rvs_ccf_models_build; make_ccf.py:105-164, 167-221) runs the same
# lm_binned_start / lm_fit on float64 template rows, with up to 48 nodes (above 24
# only this kernel's LM state exists).  Truth: the same minimiser with the model's
# error rule max(1e-5 m, 1e-2 median) (or the caller's errors); cont is written
# unfloored; the row is divided by max(cont, 1e-2 median(cont)) and put on the FFT
# grid by interp1d's formula  y_lo + (y_hi - y_lo) / (x_hi - x_lo) (x - x_lo), 1 where
# ihi is outside the row.  Bound of a model value given the device's cont: y carries
# an ulp, the difference one more, slope, product and sum one each, |x - x_lo| <= x_hi
# - x_lo:  8 eps (|y_hi| + |y_lo|).  The median of cont is an order statistic (or the
# mean of two), so the floor is exact.
ST_NONPOS_MEDIAN = 0x200


def upstream_model(L, i):
    row = L['spec'][i]
    md = np.median(row)
    med, st = md, 0
    if med <= 0:
        med, st = abs(med), ST_NONPOS_MEDIAN
        if med == 0:
            med = 1.0
    ce = L['espec'][i] if L['erows'] else np.maximum(row * 1e-5, 1e-2 * md)
    return dict(cs=row, ce=ce, status=st, medv=md, med=med, p0=stage_p0(L, row, med),
                mask=np.zeros(len(row), bool))


def model_given_cont(L, i, cont):
    """the row on the FFT grid, and its absolute bound, from the device's cont"""
    row, ntp = L['spec'][i], len(L['lam'])
    cont = np.asarray(cont, dtype=np.float64)
    y = row.astype(LD) / np.maximum(cont, 1e-2 * np.median(cont)).astype(LD)
    lnlam, logl, ihi = L['lnlam'], L['logl'], L['ihi']
    ok = (ihi >= 1) & (ihi < ntp)
    hi = np.where(ok, ihi, 1)
    ylo, yhi, xlo = y[hi - 1], y[hi], lnlam[hi - 1]
    slope = (yhi - ylo) / LD(1) / (lnlam[hi] - xlo)
    v = slope * (logl - xlo) + ylo
    return np.where(ok, v, 1), np.where(ok, 8 * EPS * (np.abs(yhi) + np.abs(ylo)), 0)


def _mk_model(name, ntp, nnode, rows, erows, npoints=64, nofit=()):
    lam = lam_of(np.arange(ntp))
    h = (ntp - 1) / (nnode - 1)
    lnlam = np.log(lam)
    w = lnlam[-1] - lnlam[0]
    logl = np.linspace(lnlam[0] - 0.1 * w, lnlam[-1] + 0.1 * w, npoints)
    ihi = np.clip(np.searchsorted(lnlam, logl), 1, ntp - 1).astype(np.int32)
    ihi[(logl < lnlam[0]) | (logl > lnlam[-1])] = -1
    ihi[0], ihi[-1] = ntp, ntp + 7            # outside the row on the far side: 1 too
    return dict(name=name, family='models', model=True, lam=lam, continuum=1,
                nodes=lam_of(np.linspace(0, ntp - 1, nnode)),
                edges=lam_of((np.arange(nnode + 1) - 0.5) * h), nfft=2, grid='wider',
                spec=np.stack([r for r, _ in rows]),
                espec=np.stack([e for _, e in rows]), erows=erows, B=len(rows),
                fit='newton', nofit=tuple(nofit), lnlam=lnlam, logl=logl, ihi=ihi,
                npoints=npoints, badmask=None, maxerr=10.0)


@functools.lru_cache(None)
def model_launches():
    Ls = []
    for k, (ntp, nnode) in enumerate(((12, 3), (513, 25), (1025, 48))):
        rows = []
        for sd in (90 + k, 95 + k):
            s, e = _flux(ntp, sd, snr=1e4, level=1.0, lines=ntp > 64)
            rows.append((s, e * 50))
        Ls.append(_mk_model('model-%d-%d' % (ntp, nnode), ntp, nnode, rows, False))
        # the caller's errors; the last row has a non-positive median (flagged; the
        # objective has no minimum there: exp(S) against negative data)
        rows = []
        for sd in (190 + k, 195 + k):
            s, e = _flux(ntp, sd, snr=300.0, level=1.0, lines=ntp > 64)
            rows.append((s, e))
        rows = rows + [(rows[0][0] - 2.0, rows[0][1])]
        Ls.append(_mk_model('model-%d-%d-erows' % (ntp, nnode), ntp, nnode, rows, True,
                            nofit=(2, )))
    return Ls
