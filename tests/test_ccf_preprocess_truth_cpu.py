"""tests/ccf_preprocess_truth.py pinned without a GPU: its stages against the oracle's
(scipy.signal.medfilt, UnivariateSpline, binned_statistic, interp_masker) and, where
the nodes are the reference's own, against oracle.preprocess_data as a whole; its
minimiser against least_squares run to 1e-15; the float64 emulation of the kernel's
Levenberg-Marquardt schedule 10 x inside every family's bound (the reference's own TRF
distance); three wrong restatements rejected; the status of every case; and the case
families' own shape: the interval, bin and pixel counts the device test relies on.

Measured here (scipy 1.15): p* against least_squares(ftol = xtol = gtol = 1e-15) from
p*: 1.6e-8 at most (TRF with a finite-difference Jacobian stops there; Newton's own
gradient is below 5e-12 on every case, after at most 3 iterations).  Per family,
largest TRF distance / largest emulation d: ccf_preprocess_truth.MEASURED and DESIGN
section 2; test_emulation_margin prints them."""
import numpy as np
import scipy.optimize
import scipy.signal

import ccf_preprocess_truth as pt
from oracle import rvs_oracle as orc

LD = pt.LD
FIT_FAMILIES = ('npix', 'nodes', 'bins', 'scale', 'medv', 'masks', 'oracle', 'grids')


def _cases(pred=lambda L: True):
    return [(L, i) for L in pt.launches() if pred(L) for i in range(L['B'])]


def test_stages_against_the_oracle():
    """masks exact (scipy's medfilt), filled spectrum, inflated errors and p0 to 1e-13
    (interp_masker, continuum_start = binned_statistic), the spline design to 1e-12
    (UnivariateSpline) on every case with a continuum fit"""
    worst = dict(filled=0.0, p0=0.0, model=0.0)
    for L, i in _cases(lambda L: L['continuum']):
        t, lam = pt.truth(L, i), L['lam']
        s, e = L['spec'][i], L['espec'][i]
        bad = np.zeros(len(s), bool) if L['badmask'] is None else L['badmask'][i] != 0
        mederr = np.nanmedian(e)
        assert mederr == t['mederr']
        if np.all(np.isfinite(s)):      # (+inf flux lies under a full badmask)
            want = bad | (e > L['maxerr'] * mederr) | (scipy.signal.medfilt(s, 11) <= 0)
            assert np.array_equal(want, t['mask']), (L['name'], i)
        else:
            assert t['mask'].all()
        filled = orc.interp_masker(lam, s, t['mask'])
        scale = np.abs(filled).max()
        worst['filled'] = max(worst['filled'], np.abs(filled - t['cs']).max() / scale)
        p0 = orc.continuum_start(lam, t['cs'], L['edges'])
        worst['p0'] = max(worst['p0'], np.abs(p0 - t['p0']).max())
        p = t['p0'] + 0.01 * np.cos(np.arange(len(p0)))
        mine = np.exp(np.clip((pt.tables(L)['A'] @ p.astype(LD)), -100, 100))
        theirs = orc.continuum_model(p, L['nodes'], lam)
        worst['model'] = max(worst['model'], float(np.abs(theirs / mine - 1).max()))
    print('truth against oracle stages', worst)
    assert worst['filled'] <= 1e-13 and worst['p0'] <= 1e-13
    assert worst['model'] <= 1e-12 * pt.tables(pt.by_name('nodes-empty-interval'))['cond']


def test_whole_preprocess_against_the_oracle():
    """the reference's own nodes: oracle.preprocess_data end to end.  Masks, filled
    spectrum exact / 1e-13; cont inside the family's TRF distance (the oracle runs TRF
    too, on UnivariateSpline: both lie within d_trf of p*, so within 2 d_trf |A|_inf
    of each other in log cont); proc_spec / proc_ivar to the same plus 1e-12"""
    bound = pt.bound_of('oracle')
    for L in pt.by_family('oracle'):
        a, b = pt.fft_span(L)
        conf = dict(logl0=a, logl1=b, npoints=L['nfft'], continuum=True,
                    splinestep=L['splinestep'])
        T = pt.tables(L)
        rowsum = float(np.abs(T['A']).sum(1).max())
        for i in range(L['B']):
            t = pt.truth(L, i)
            bad = None if L['badmask'] is None else L['badmask'][i] != 0
            r1, r2, info = orc.preprocess_data(L['lam'], L['spec'][i], L['espec'][i],
                                               conf, badmask=bad, maxerr=L['maxerr'],
                                               details=True)
            assert np.array_equal(info['badmask'], t['mask'])
            assert np.abs(info['filled'] - t['cs']).max() <= 1e-13 * np.abs(t['cs']).max()
            assert np.array_equal(info['cespec'], t['ce'])
            assert np.array_equal(info['nodes'], L['nodes'])
            assert np.abs(info['p0'] - t['p0']).max() <= 1e-13
            pstar, _, _ = pt.newton(L, i, pt.emulate(L, i))
            cont, _, _, _, _ = pt.cont_given_pfit(L, i, pstar)
            dlog = float(np.abs(np.log(info['cont'] / cont.astype(np.float64))).max())
            assert dlog <= 2 * bound * rowsum + 1e-12, (dlog, bound, rowsum)
            t1, _, t2, _ = pt.proc_given_cont(L, i, cont)
            tol = 2 * (2 * bound * rowsum + 1e-12)
            assert np.abs(r1 - t1).max() <= tol * np.abs(t1).max()
            assert np.abs(r2 - t2).max() <= tol * np.abs(t2).max()
            assert np.array_equal(r1 == 0, t1 == 0) and np.array_equal(r2 == 0, t2 == 0)


def test_minimiser_against_least_squares_run_to_the_end():
    """p* against least_squares(ftol = xtol = gtol = 1e-15) started from p*: the
    agreement is measured (printed; docstring) and must be inside the family's bound"""
    worst, worst_g = 0.0, 0.0
    for L, i in _cases(lambda L: L['fit'] == 'newton'):
        pstar, it, g = pt.newton(L, i, pt.emulate(L, i))
        assert it <= 5
        worst_g = max(worst_g, g)
        x = scipy.optimize.least_squares(pt._resid64(L, i), pstar.astype(np.float64),
                                         loss='soft_l1', ftol=1e-15, xtol=1e-15,
                                         gtol=1e-15)['x']
        d = float(np.abs(x - pstar).max())
        worst = max(worst, d)
        assert d <= max(pt.bound_of(L['family']), 1e-12), (L['name'], i, d)
    print('p* against tight least_squares: %.3g; Newton gradient %.3g' % (worst, worst_g))
    assert worst_g < 1e-11


def test_emulation_margin():
    """the float64 emulation of lm_fit's schedule is at least 10 x inside the family's
    TRF distance on every fitted case; Newton converges on all of them"""
    rep = {}
    for L, i in _cases(lambda L: L['fit'] == 'newton'):
        pe = pt.emulate(L, i)
        pstar, _, _ = pt.newton(L, i, pe)
        d = float(np.abs(pe - pstar).max())
        b = pt.bound_of(L['family'])
        r = rep.setdefault(L['family'], [b, 0.0])
        r[1] = max(r[1], d)
        assert 10 * d <= b, (L['name'], i, d, b)
    for f, (b, d) in sorted(rep.items()):
        print('ccf-preprocess family %-7s d_trf %.3g emulation %.3g margin %.0f x' %
              (f, b, d, b / max(d, 1e-300)))
    assert set(rep) == set(FIT_FAMILIES)     # (the model rows: test_model_rows)


def test_gtol_exit_of_the_emulation():
    """fit = 'gtol': the emulation leaves at the gradient test with C (C^-1 p0), inside
    8 eps cond(C) max|p0|, and max|p0| >= 1 so that an ulp of a median is inside it"""
    worst = 0.0
    for L, i in _cases(lambda L: L['fit'] == 'gtol'):
        p0 = pt.truth(L, i)['p0']
        assert np.abs(p0).max() >= 1
        r = np.abs(pt.emulate(L, i) - p0).max() / pt.p0_bound(L, p0)
        worst = max(worst, r)
        assert r <= 1, (L['name'], i, r)
    print('gtol exit: emulation / bound %.3g' % worst)


def test_rejects_a_gradient_without_one_pixel():
    """a Levenberg-Marquardt whose normal equations leave out the last pixel of one
    knot interval ends outside the bound"""
    for name in ('nodes-23-h63.5', 'npix-513', 'nodes-6-h256.5'):
        L = pt.by_name(name)
        ist = pt.tables(L)['istart']
        drop = int(ist[len(ist) // 2]) - 1        # last pixel of an interior interval
        pstar, _, _ = pt.newton(L, 0, pt.emulate(L, 0))
        d = float(np.abs(pt.emulate(L, 0, drop=drop) - pstar).max())
        assert d > pt.bound_of(L['family']), (name, d)
        # and the truth's own gradient notices the pixel: Newton on it goes elsewhere
        pwrong, _, _ = pt.newton(L, 0, pstar, drop=drop)
        assert float(np.abs(pwrong - pstar).max()) > pt.bound_of(L['family'])


def test_rejects_a_bin_median_off_by_one_rank():
    for name in ('bins-wave-gtol', 'bins-block-gtol', 'bins-mixed-gtol'):
        L = pt.by_name(name)
        p0 = pt.truth(L, 0)['p0']
        wrong = pt.upstream(L, 0, rank_shift=1)['p0']
        assert np.abs(wrong - p0).max() > pt.p0_bound(L, p0), name


def test_rejects_an_edge_fill_that_interpolates():
    L = pt.by_name('masks-hard-gtol')
    t = pt.truth(L, 0)                              # first and last 200 masked
    wrong = pt.upstream(L, 0, edge='interp')
    assert np.array_equal(wrong['mask'], t['mask'])
    assert np.abs(wrong['p0'] - t['p0']).max() > pt.p0_bound(L, t['p0'])
    L = pt.by_name('masks-mild-gtol')               # first pixel only: bin 0's median
    t, wrong = pt.truth(L, 1), pt.upstream(L, 1, edge='interp')
    assert wrong['cs'][0] != t['cs'][0] and t['cs'][0] == L['spec'][1][1]


def test_status_of_every_case():
    allmasked = {('masks-hard', 3), ('masks-hard', 4), ('nocont', 3), ('sign-gtol', 0),
                 ('sign-zero-gtol', 0)}
    for L, i in _cases():
        want = pt.ST_ALLMASKED if (L['name'], i) in allmasked else 0
        assert pt.truth(L, i)['status'] == want, (L['name'], i)
    assert pt.truth(pt.by_name('sign-gtol'), 0)['medv'] < 0
    assert pt.truth(pt.by_name('sign-zero-gtol'), 0)['medv'] == 0
    assert pt.truth(pt.by_name('nocont'), 2)['medv'] < 0


def test_masks_of_the_mask_family():
    """what each spectrum of masks-mild is there for"""
    L = pt.by_name('masks-mild')
    m = [pt.truth(L, i)['mask'] for i in range(L['B'])]
    n = len(L['lam'])
    assert not m[0].any()
    assert np.nonzero(m[1])[0].tolist() == [0] and np.nonzero(m[2])[0].tolist() == [n - 1]
    assert m[3][::2].all() and not m[3][1::2].any()
    assert np.nonzero(m[4])[0].tolist() == list(range(505, 520))    # across 511 / 512
    e = L['espec'][5]
    at = np.nonzero(e == L['maxerr'] * np.nanmedian(e))[0]
    assert len(at) == 1 and not m[5][at[0]]                 # exactly maxerr mederr
    assert m[5].sum() == 1 and e[m[5]][0] == np.nextafter(e[at[0]], np.inf)
    assert np.nonzero(m[6])[0].tolist() == [0, 17, 600, n - 1]      # +inf errors
    assert np.nonzero(m[7])[0].tolist() == [0]      # pixel 3 <= 0 + five padded zeros
    assert np.nonzero(m[8])[0].tolist() == [505]            # six of eleven at one centre
    assert not m[9].any()                                   # five of eleven: nothing


def test_shapes_the_device_test_relies_on():
    ints, bins, npixs, nnodes = set(), set(), set(), set()
    for L in pt.launches():
        npixs.add(len(L['lam']))
        if not L['continuum']:
            continue
        T = pt.tables(L)
        nnodes.add(len(L['nodes']))
        ints |= set(np.diff(T['istart']).tolist())
        bs = T['bin_start']
        bins |= set(np.diff(bs).tolist())
        assert np.all(np.diff(bs) >= 0) and bs[-1] <= len(L['lam'])
    assert {0, 1, 63, 64, 65, 255, 256, 257, 600} <= ints
    assert {0, 1, 2, 64, 65, 256, 257, 600} <= bins
    assert {12, 13, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 1537} <= npixs
    assert {3, 4, 5, 23, 24} <= nnodes
    for key in ('wave', 'block', 'mixed'):
        L = pt.by_name('bins-%s-gtol' % key)
        d = np.diff(pt.tables(L)['bin_start'])
        assert (d.max() <= 256) == (key == 'wave')
        assert pt.tables(L)['bin_start'][-1] < len(L['lam'])     # pixels past the edge
    assert 6100 < pt.max_npix() < 6300
    # a bin median below the 1e-3 med floor, in both median paths
    for name in ('bins-wave-gtol', 'bins-block-gtol'):
        L = pt.by_name(name)
        t = pt.truth(L, 1)
        assert np.isclose(t['p0'], np.log(1e-3 * t['med'])).any(), name


def test_floor_branch_margins():
    """medv family: 1e-2 medv floors the fitted continuum on the faint half and not on
    the bright one, both by far more than the margin"""
    L = pt.by_name('medv-floor')
    pstar, _, _ = pt.newton(L, 0, pt.emulate(L, 0))
    _, _, floored, free, floor = pt.cont_given_pfit(L, 0, pstar)
    assert floored.sum() > 100 and free.sum() > 100
    assert (floored | free).all() or (~(floored | free)).sum() < 5
    assert floor == 1e-2 * pt.truth(L, 0)['medv']
    Ln = pt.by_name('nocont')
    _, _, floored, free, floor = pt.cont_given_pfit(Ln, 1, None)
    assert floored.all() and floor > 1
    _, _, floored, free, floor = pt.cont_given_pfit(Ln, 2, None)    # medv < 0: max(cont, 1)
    assert floor == 1 and not floored.any()


def test_downstream_bounds_hold_a_float64_evaluation_and_nothing_worse():
    """cont given pfit and proc given cont: a plain float64 numpy evaluation lies
    inside the bounds, a relative error of 1e-12 outside"""
    worst = dict(cont=0.0, r1=0.0, r2=0.0, sse=0.0)
    for L, i in _cases(lambda L: L['fit'] in ('newton', 'gtol') and L['B'] <= 3):
        T, t = pt.tables(L), pt.truth(L, i)
        pfit = pt.emulate(L, i)
        c64 = T['Cinv'] @ pfit
        S = (T['Eb'] * np.stack([c64[T['El'] + q] for q in range(3)], 1)).sum(1)
        raw = np.exp(np.clip(S, -100, 100))
        cont64 = np.maximum(1e-2 * t['medv'], raw) if t['medv'] > 0 else np.maximum(raw, 1)
        cont, b, _, _, _ = pt.cont_given_pfit(L, i, pfit)
        worst['cont'] = max(worst['cont'], pt.ratio(cont64, cont, b * cont))
        assert pt.ratio(cont64 * (1 + 1e-12), cont, b * cont) > 1
        r1, b1, r2, b2 = pt.proc_given_cont(L, i, cont64)
        with np.errstate(all='ignore'):
            c = np.where(t['mask'], 0, L['spec'][i] / cont64)
            iv = np.where(t['mask'], 0, cont64 * cont64 * (1 / (t['ce'] * t['ce'])))
        xi, rw = T['xind'], T['rw']
        ok, j, lw = xi >= 0, np.where(xi >= 0, xi, 0), 1 - rw
        g1 = np.where(ok, lw * c[j] + rw * c[j + 1], 0)
        a, bb = iv[j], iv[j + 1]
        g2 = np.where(ok, a * bb / (lw * lw * bb + rw * rw * a + ((a * bb) == 0)), 0)
        worst['r1'] = max(worst['r1'], pt.ratio(g1, r1, b1))
        worst['r2'] = max(worst['r2'], pt.ratio(g2, r2, b2))
        if np.any(r2 != 0):
            assert pt.ratio(g2 * (1 + 1e-12), r2, b2) > 1
        s, bs = pt.sse_given_proc(g1, g2)
        worst['sse'] = max(worst['sse'], pt.ratio(np.sum(g1 * g1 * g2), s, bs))
    print('float64 evaluation / bound', worst)
    assert max(worst.values()) <= 1


def test_largest_arm():
    """the launch at the LDS limit: Newton converges there too"""
    L = pt.largest_arm()
    assert len(L['lam']) == pt.max_npix()
    pe = pt.emulate(L, 0)
    pstar, it, g = pt.newton(L, 0, pe)
    x = pt.trf(L, 0)
    d, dt = float(np.abs(pe - pstar).max()), float(np.abs(x - pstar).max())
    print('largest arm: npix %d emulation %.3g TRF %.3g' % (len(L['lam']), d, dt))
    assert 10 * d <= max(dt, pt.bound_of('npix'))


def test_model_rows():
    """the template-row family (ccf_model_kernel): the emulation 10 x inside the
    family's TRF distance, the status of the non-positive median rows, ihi outside
    the row on both sides, and the bound of a model value holds a float64 evaluation
    and no 1e-12 error"""
    b = pt.bound_of('models')
    worst = 0.0
    shapes = set()
    for L in pt.model_launches():
        ntp = len(L['lam'])
        shapes.add((ntp, len(L['nodes']), L['erows']))
        assert L['ihi'][0] == ntp and L['ihi'][-1] > ntp and (L['ihi'] == -1).sum() > 2
        for i in range(L['B']):
            t = pt.truth(L, i)
            assert t['status'] == (pt.ST_NONPOS_MEDIAN if i in L['nofit'] else 0)
            pe = pt.emulate(L, i)
            if i not in L['nofit']:
                pstar, _, _ = pt.newton(L, i, pe)
                d = float(np.abs(pe - pstar).max())
                worst = max(worst, d)
                assert 10 * d <= b, (L['name'], i, d, b)
            raw, _ = pt.raw_cont(L, pe)
            cont = raw.astype(np.float64)
            v, bv = pt.model_given_cont(L, i, cont)
            y = L['spec'][i] / np.maximum(cont, 1e-2 * np.median(cont))
            ok = (L['ihi'] >= 1) & (L['ihi'] < ntp)
            hi = np.where(ok, L['ihi'], 1)
            g = (y[hi] - y[hi - 1]) / (L['lnlam'][hi] - L['lnlam'][hi - 1]) * \
                (L['logl'] - L['lnlam'][hi - 1]) + y[hi - 1]
            g = np.where(ok, g, 1.0)
            assert pt.ratio(g, v, bv) <= 1 and np.all(g[~ok] == 1)
            assert pt.ratio(np.where(ok, g * (1 + 1e-12), g), v, bv) > 1
    print('ccf-preprocess family models  d_trf %.3g emulation %.3g margin %.0f x' %
          (b, worst, b / worst))
    assert shapes == {(12, 3, False), (12, 3, True), (513, 25, False), (513, 25, True),
                      (1025, 48, False), (1025, 48, True)}
