"""The velocity-grid chi^2 kernels under a banded resolution matrix
(chisq_grid_resol_pipe_kernel<P, 11>: register window, 11 diagonals;
chisq_grid_resol_kernel<P>: LDS ring, any other odd band up to 33; csrc/chisq.hip)
through engine.build_templates -> engine.chisq_grid(..., resols=...), the path of
find_best including the redo of flagged jobs, against the exact truth of
tests/chisq_grid_resol_truth.py.  The truth takes the spline records the kernels
were given (copied from the device), so only the kernels' own arithmetic is
under test.

Taps are built directly ([S or 1, npix, nd], zero where the column is outside the
spectrum) and handed to engine.make_resol; nd is asserted, so that which kernel
runs is not left to engine.resol_taps (it drops all-zero diagonals).  The same
11-diagonal matrix zero-padded to 13 is how it reaches the ring kernel.

Bound of the well-conditioned sweeps A-G: 10 x chisq_grid_resol_truth
.EMULATION_WORST = 2.28e-11 relative to max(|chi^2|, npix) -- ten times the
distance of the float64 statement of the device's arithmetic from the truth on the
same inputs (test_chisq_grid_resol_cpu.py), the factor covering numpy's summation
order against the lanes' sequential fma over up to 401 pixels.  status == 0 is
asserted in every such case: no value was replaced by the redo.

Sweep H (30-70 % of an arm with errors inflated 1e4 ... 1e6-fold): 5e-8, the
bound of test_chisq_accuracy.test_long_weightless_stretches_take_the_robust_path,
and RVS_ST_ILLCOND on every case whose emulation error is above it.

Measured on an MI355X (worst figure per sweep, printed by the tests), relative to
max(|chi^2|, npix):
  A pixel-loop tails 7.59e-13    B velocity / job tails 1.23e-12
  C every npoly 4.03e-12 (npoly 2, where the emulation has its 2.28e-12; every
    other npoly <= 8e-13)        D launch forms 6.85e-13
  E linear knots 7.83e-13        F grid set 6.26e-13
  G in-range entries of a range-flagged job 7.02e-13
  I register window against LDS ring on the padded band: bit-equal at every shape
  H, the twelve cases that must be flagged (emulation 3.0e-7 ... 4.1e-6):
    before the resolution kernels had the pivot-range test: status 0 and
      nd 11: 8.21e-7, 6.53e-7, 1.07e-6, 4.56e-7, 2.32e-6, 2.40e-6
      nd 13: 7.86e-7, 1.03e-6, 1.02e-6, 6.65e-7, 2.41e-6, 3.73e-6
      (S/N 30 then 1000; npoly 10: (0.5, 1e6); npoly 15: (0.5, 1e6), (0.3, 1e6))
    with it: RVS_ST_ILLCOND on exactly these, errors 1.7e-15 ... 1.4e-13
  H, the twenty cases below 5e-8 in the emulation: not flagged, worst 4.66e-8
    ((S/N 1000, 0.3, 1e6), npoly 10, nd 13: emulation 3.82e-8), same before and after
  H, vanishing template: redone before and after (a pivot turns non-positive there,
    which the resolution kernels always reported), worst 2.2e-14
"""
import numpy as np
import pytest
import torch

import chisq_grid_resol_truth as gt
from conftest import GOLD_CONFIG
from oracle import rvs_oracle as orc

pytestmark = pytest.mark.gpu

BOUND = 10 * gt.EMULATION_WORST
H_BOUND = 5e-8
DEV = 'cuda'
WORST = {}


def _mods():
    from rvspecfit_amd import _lib, engine
    _lib.require_gpu()
    return _lib, engine


_dlibs = {}


def _dlib(key):
    from rvspecfit_amd.library import TemplateLibrary
    if key not in _dlibs:
        _dlibs[key] = TemplateLibrary(key[:6], gt.lib_dict(key), device=DEV)
    return _dlibs[key]


def _t(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


_setups = {}


def _setup(case):
    """batch, libraries, device records of `case`, once"""
    if case['name'] in _setups:
        return _setups[case['name']]
    _lib, engine = _mods()
    arms, libs, coefs, outs, rec = [], {}, [], [], []
    for arm in case['arms']:
        lib = _dlib(arm['lib'])
        if len(arm['grids']) == 1:
            ad = engine.ArmData(arm['name'], arm['grids'][0], arm['spec'],
                                arm['espec'], device=DEV)
        else:
            ad = engine.ArmData(arm['name'], arm['grids'], arm['spec'], arm['espec'],
                                device=DEV,
                                grid_id=np.asarray(arm['gid'], dtype=np.int32))
        arms.append(ad)
        libs[arm['name']] = lib
        with np.errstate(all='ignore'):
            c, o = engine.build_templates(lib, _t(case['params']))
        coefs.append(c)
        outs.append(o)
        rec.append((c.cpu().numpy(), lib.lam))
    su = dict(batch=engine.SpecBatch(arms), libs=libs, coefs=coefs, outs=outs,
              rec=rec, truth={}, got={})
    # ordinary templates lie inside the grid: no penalty in the values
    for o in outs:
        o = o.cpu().numpy()
        assert np.all((o == 0) | ~np.isfinite(o)), o
    _setups[case['name']] = su
    return su


def _resols(case, band, su):
    _lib, engine = _mods()
    out = []
    for arm in case['arms']:
        taps = arm['bands'][band]
        r = engine.make_resol(taps, taps.shape[2], arm['spec'].shape[0], DEV)
        assert r['nd'] == taps.shape[2]
        assert r['stride'] == (0 if taps.shape[0] == 1 else
                               taps.shape[1] * taps.shape[2])
        out.append(r)
    return out


def run(case, band, order=None):
    """engine.chisq_grid on the jobs of `case` (in the order `order`) with the
    band `band` -> chisq [J, Nv], status [J] (numpy)"""
    _lib, engine = _mods()
    su = _setup(case)
    js, jt, v = case['job_spec'], case['job_templ'], case['vels']
    if order is not None:
        js, jt = js[order], jt[order]
        v = v if v.ndim == 1 else v[order]
    chisq, st = engine.chisq_grid(
        su['batch'], su['libs'], su['coefs'], su['outs'], _t(v),
        npoly=case['npoly'], rbf=case['rbf'], job_spec=_t(js, torch.int32),
        job_templ=_t(jt, torch.int32), resols=_resols(case, band, su))
    torch.cuda.synchronize()
    return chisq.cpu().numpy(), st.cpu().numpy()


def device(case, band):
    su = _setup(case)
    if band not in su['got']:
        su['got'][band] = run(case, band)
    return su['got'][band]


def truth(case, band):
    su = _setup(case)
    k = gt.truth_key(band)
    if k not in su['truth']:
        su['truth'][k] = gt.evaluate(case, k, su['rec'])
    return su['truth'][k]


def worst_error(case, band, got, jobs=None):
    tr = truth(case, band)
    w = 0.0
    for j in (range(len(got)) if jobs is None else jobs):
        assert np.all(np.isfinite(got[j])), (case['name'], band, j)
        w = max(w, float(gt.rel_err(got[j], tr[j], gt.case_npix(case, j)).max()))
    return w


def check(case, bands, sweep):
    """every band of `bands`: status 0, every value within BOUND of the truth"""
    worst = {}
    for band in bands:
        got, st = device(case, band)
        assert np.all(st == 0), (case['name'], band, st)
        worst[band] = worst_error(case, band, got)
    print('%s: worst error %s (bound %.3g)' % (
        case['name'], ', '.join('%s %.3g' % kv for kv in worst.items()), BOUND))
    WORST[sweep] = max(WORST.get(sweep, 0.0), max(worst.values()))
    print('sweep %s so far: %.3g' % (sweep, WORST[sweep]))
    assert max(worst.values()) <= BOUND, (case['name'], worst)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# --------------------------------------------------------------------------
# A-F: the inputs of chisq_grid_resol_truth.cases()
# --------------------------------------------------------------------------
@pytest.mark.parametrize('npix', gt.A_NPIX)
def test_pixel_loop_tails(npix):
    """A: arms below, at and above the half band (M = 5 / 16) and in every residue
    class of the 12-fold unrolled window that matters; pipe kernel, ring kernel
    with the padded 11 -> 13, with 3 and with 33 diagonals"""
    check(gt.cases()['A-%d' % npix], ['nd11', 'nd11as13', 'nd3', 'nd33'], 'A')


@pytest.mark.parametrize('grid', ['shared', 'own'])
@pytest.mark.parametrize('Nv,J', gt.B_SHAPES)
def test_velocity_and_job_tails(Nv, J, grid):
    """B: Nv against the 64-lane and 256-lane blocks, J against the deal of jobs
    over eight XCDs; job_spec / job_templ neither identity nor monotone; one
    velocity grid for all jobs or one per job; the truth at every velocity"""
    case = gt.cases()['B-%dx%d-%s' % (Nv, J, grid)]
    assert case['vels'].shape == ((Nv, ) if grid == 'shared' else (J, Nv))
    assert len(set(zip(case['job_spec'], case['job_templ']))) == min(J, 12)
    check(case, ['nd11', 'nd9'], 'B')


@pytest.mark.parametrize('npoly,rbf', gt.C_BASES)
def test_every_npoly(npoly, rbf):
    """C: every instantiation P = 1 ... 16 of both kernels (scalar-row pieces of
    its own each; one wave per SIMD from P = 13), RBF and Chebyshev bases"""
    check(gt.cases()['C-%d-%s' % (npoly, 'rbf' if rbf else 'cheb')],
          ['nd11', 'nd11as13'], 'C')


def test_shared_matrix_is_the_per_spectrum_matrix():
    """D: one matrix for all spectra (taps_stride 0) and the same matrix given
    per spectrum: the same bits"""
    case = gt.cases()['D-shared-matrix']
    check(case, ['nd11', 'nd11as13'], 'D')
    for one, rep in (('nd11', 'nd11rep'), ('nd11as13', 'nd11repas13')):
        assert _same_bits(device(case, one)[0], device(case, rep)[0]), one
        assert np.all(device(case, rep)[1] == 0)


def test_second_arm_accumulates():
    """D: two arms (the second launch adds with beta = 1): the sum of the truths"""
    case = gt.cases()['D-two-arms']
    assert len(case['arms']) == 2
    check(case, ['nd11', 'nd11as13'], 'D')


def test_unusable_template_among_ordinary_ones():
    """D: a template whose `outside` flag is not finite: its job is what the
    oracle's get_chisq gives for it, the neighbours are untouched"""
    case = gt.cases()['D-nan-template']
    su = _setup(case)
    assert not np.isfinite(su['outs'][0].cpu().numpy()[1])
    arm = case['arms'][0]
    lam = arm['grids'][0]
    worst = {}
    for band in ('nd11', 'nd11as13'):
        got, st = device(case, band)
        assert np.all(st == 0), st
        s = int(case['job_spec'][1])
        osd = [orc.SpecData(arm['name'], lam, arm['spec'][s], arm['espec'][s])]
        R = gt.taps_to_sparse(arm['bands'][band][s])
        with np.errstate(all='ignore'):
            want = orc.get_chisq(osd, 0., tuple(case['params'][1]), None,
                                 dict(npoly=case['npoly']), GOLD_CONFIG,
                                 {arm['name']: gt.oracle_lib(arm['lib'])},
                                 resol_params={arm['name']: R})
        assert want == 1000. * 10 * len(lam)
        assert np.all(got[1] == want)
        worst[band] = worst_error(case, band, got, jobs=[0, 2])
        assert worst[band] <= BOUND
        alone, st2 = run(case, band, order=np.array([0, 2]))
        assert np.all(st2 == 0) and _same_bits(alone, got[[0, 2]])
    print('D-nan-template: worst error of the neighbours', worst)
    WORST['D'] = max(WORST.get('D', 0.0), max(worst.values()))


def test_linear_template_grid():
    """E: log_step = 0 (knot index (int)((x - x0) / step)), both kernels"""
    case = gt.cases()['E-linear']
    assert not _dlib('gold_b_lin').log_step
    check(case, ['nd11', 'nd11as13'], 'E')


def test_grid_sets():
    """F: four spectra of one arm on grids of their own (301 / 280 / 278 cut from
    pixel 12 / 296 pixels), all with 11 diagonals (pipe kernel) and with 9 / 13 /
    21 / 11 (the batch's band is 21: ring kernel); each against the truth on its
    own grid and matrix, and alone it gives the bits it gives inside the set"""
    _lib, engine = _mods()
    case = gt.cases()['F-grid-set']
    arm = case['arms'][0]
    assert arm['bands']['nd11'].shape == (4, 301, 11)
    assert arm['bands']['mixed21'].shape == (4, 301, 21)
    check(case, ['nd11', 'mixed21'], 'F')
    su = _setup(case)
    for band in ('nd11', 'mixed21'):
        got = device(case, band)[0]
        for j in range(4):
            s, t = int(case['job_spec'][j]), int(case['job_templ'][j])
            lam = arm['grids'][arm['gid'][s]]
            n = len(lam)
            ad = engine.ArmData(arm['name'], lam, arm['spec'][s:s + 1, :n],
                                arm['espec'][s:s + 1, :n], device=DEV)
            taps = arm['bands'][band][s:s + 1, :n].copy()
            r = engine.make_resol(taps, taps.shape[2], 1, DEV)
            c, st = engine.chisq_grid(
                engine.SpecBatch([ad]), su['libs'], su['coefs'], su['outs'],
                _t(case['vels']), npoly=case['npoly'], rbf=case['rbf'],
                job_spec=_t([0], torch.int32), job_templ=_t([t], torch.int32),
                resols=[r])
            assert int(st[0].item()) == 0
            assert _same_bits(c.cpu().numpy()[0], got[j]), (band, j)


# --------------------------------------------------------------------------
# G: range status
# --------------------------------------------------------------------------
def _vel_of(r):
    """velocity whose Doppler factor is r"""
    return gt.C_KMS * (1 - r * r) / (1 + r * r)


@pytest.mark.parametrize('band', ['nd11', 'nd11as13'])
def test_range_status(band):
    """velocities that push the arm's first (job 1) or last (job 2) pixel two or
    more template pixels off the knots next to velocities well inside:
    RVS_ST_SPLINE_RANGE on exactly the jobs the truth's rule names, those entries
    not finite, the in-range entries of the same job within the bound"""
    _lib, engine = _mods()
    base = gt.cases()['B-64x8-own']
    arm = base['arms'][0]
    lam = arm['grids'][0]
    knots = gt.oracle_lib('gold_r').lam
    lo = _vel_of((knots[0] - 2 * (knots[1] - knots[0])) / lam[0])
    hi = _vel_of((knots[-1] + 2 * (knots[-1] - knots[-2])) / lam[-1])
    v = np.stack([np.linspace(-300. + 5 * j, 300. - 3 * j, 70) for j in range(4)])
    v[1, [3, 40, 69]] = lo, 1.01 * lo, 1.05 * lo
    v[2, [0, 17, 64]] = hi, 1.01 * hi, 1.05 * hi
    case = gt._case('G-range', [arm], 5, True, gt.PARAMS, [2, 0, 1, 2], [3, 0, 1, 2], v)
    named = [not gt.in_range(knots, lam, v[j]).all() for j in range(4)]
    assert named == [False, True, True, False]
    got, st = run(case, band)
    tr = truth(case, band)
    worst = 0.0
    for j in range(4):
        assert bool(st[j] & _lib.ST_SPLINE_RANGE) == named[j], (j, st)
        if not named[j]:
            assert st[j] == 0
        ok = gt.in_range(knots, lam, v[j])
        assert not np.any(np.isfinite(got[j][~ok])), j
        assert np.all(np.isfinite(got[j][ok])), j
        worst = max(worst, float(gt.rel_err(got[j][ok], tr[j][ok], len(lam)).max()))
    print('G-range %s: status %s, worst in-range error %.3g' % (band, st, worst))
    WORST['G'] = max(WORST.get('G', 0.0), worst)
    assert worst <= BOUND


# --------------------------------------------------------------------------
# H: weightless stretches under a band
# --------------------------------------------------------------------------
@pytest.mark.parametrize('npoly', gt.H_NPOLY)
@pytest.mark.parametrize('nd', gt.H_ND)
def test_weightless_stretches_under_a_band(nd, npoly):
    """the masked-stretch cases of test_long_weightless_stretches_take_the_robust_
    path with 11 (pipe kernel) and 13 (ring kernel) diagonals: every value within
    5e-8 of the truth (1e-6 is the contract), RVS_ST_ILLCOND on every case whose
    float64 emulation is above 5e-8 (chisq_grid_resol_truth.H_EMULATION), no
    RVS_ST_NONFINITE"""
    _lib, engine = _mods()
    lib = _dlib('gold_b')
    spec, espec, taps = gt.h_spectra(nd)
    S = len(spec)
    ad = engine.ArmData('gold_b', gt.H_LAM, spec, espec, device=DEV)
    r = engine.make_resol(taps[None], nd, S, DEV)
    assert r['nd'] == nd and r['stride'] == 0
    coef, out = engine.build_templates(lib, _t(np.array([gt.H_PARAM])))
    assert float(out[0].item()) == 0
    chisq, st = engine.chisq_grid(
        engine.SpecBatch([ad]), {'gold_b': lib}, [coef], [out], _t(gt.H_VELS),
        npoly=npoly, job_templ=_t(np.zeros(S), torch.int32), resols=[r])
    chisq, st = chisq.cpu().numpy(), st.cpu().numpy()
    tr = gt.h_evaluate(nd, npoly, coef.cpu().numpy()[0], lib.lam)
    err = [float(gt.rel_err(chisq[i], tr[i], len(gt.H_LAM)).max())
           if np.all(np.isfinite(chisq[i])) else np.inf for i in range(S)]
    for i, key in enumerate(gt.H_SPECTRA):
        k = key + (npoly, nd)
        print('H %s: error %.3g status 0x%x (emulation %.3g%s)' % (
            k, err[i], st[i], gt.H_EMULATION[k],
            ', must flag' if k in gt.h_must_flag() else ''))
    for i, key in enumerate(gt.H_SPECTRA):
        k = key + (npoly, nd)
        assert not st[i] & (_lib.ST_NONFINITE | _lib.ST_CHOL_FALLBACK), k
        assert err[i] < H_BOUND, (k, err[i])
        if k in gt.h_must_flag():
            assert st[i] & _lib.ST_ILLCOND, k
        else:
            assert st[i] in (0, _lib.ST_ILLCOND), k


@pytest.mark.parametrize('nd', gt.H_ND)
def test_vanishing_template_under_a_band(nd):
    """a template that is ~e^-60 of its level over the red half of the arm
    (the second half of that test): flagged, and the oracle's SVD statement with
    the band to 1e-8"""
    from rvspecfit_amd.library import TemplateLibrary
    _lib, engine = _mods()
    dd = dict(gt.lib_dict('gold_b'))
    z = np.array(dd['dats'], dtype=np.float32)
    red = dd['lam'] > 4560
    z[:, red] = -60. + 0.01 * z[:, red]
    dd['dats'] = z
    lib = TemplateLibrary('gold_b', dd, device=DEV)
    olibs = {'gold_b': orc.Library(dd)}
    lam, p = gt.H_LAM, gt.H_PARAM
    R = gt.h_matrix(nd)
    taps = gt.taps_from_sparse(R, nd)
    spl = orc.Spline(dd['lam'], olibs['gold_b'].eval(p))
    rng = np.random.RandomState(2)
    sp = (R @ orc.eval_rv(spl, 30., lam)) * (
        1 + 0.01 * rng.standard_normal(len(lam))) + 0.05
    es = np.full_like(sp, 0.01 * np.median(sp))
    ad = engine.ArmData('gold_b', lam, sp, es, device=DEV)
    r = engine.make_resol(taps[None], nd, 1, DEV)
    assert r['nd'] == nd
    osd = [orc.SpecData('gold_b', lam, sp, es)]
    for npoly in gt.H_NPOLY:
        coef, out = engine.build_templates(lib, _t(np.array([p])))
        chisq, st = engine.chisq_grid(
            engine.SpecBatch([ad]), {'gold_b': lib}, [coef], [out], _t(gt.H_VELS),
            npoly=npoly, resols=[r])
        got, st = chisq.cpu().numpy()[0], int(st[0].item())
        worst = 0.0
        for v, g in zip(gt.H_VELS, got):
            o = orc.get_chisq(osd, v, p, None, options=dict(npoly=npoly),
                              config=GOLD_CONFIG, libs=olibs,
                              resol_params={'gold_b': R})
            worst = max(worst, abs(g - o) / max(abs(o), len(lam)))
        print('vanishing template, nd %d npoly %d: status 0x%x worst %.3g' % (
            nd, npoly, st, worst))
        assert st & (_lib.ST_ILLCOND | _lib.ST_CHOL_FALLBACK), (npoly, st)
        assert worst <= 1e-8, (npoly, worst)


# --------------------------------------------------------------------------
# I, J: the two kernels against each other; determinism
# --------------------------------------------------------------------------
@pytest.mark.parametrize('grid', ['shared', 'own'])
@pytest.mark.parametrize('Nv,J', gt.B_SHAPES)
def test_pipe_kernel_against_ring_kernel(Nv, J, grid):
    """I: the same matrix through the register window (11) and, zero-padded to
    13, through the LDS ring: within 1e-11 max(|chi^2|, 1e3), the project's
    tolerance for two device forms of one sum"""
    case = gt.cases()['B-%dx%d-%s' % (Nv, J, grid)]
    (a, sa), (b, sb) = device(case, 'nd11'), device(case, 'nd11as13')
    assert np.all(sa == 0) and np.all(sb == 0)
    d = float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e3)))
    print('%s: pipe against ring %.3g, bit-equal: %s' % (case['name'], d,
                                                        _same_bits(a, b)))
    assert np.all(np.isfinite(a)) and np.all(np.isfinite(b))
    assert d < 1e-11


@pytest.mark.parametrize('band', ['nd11', 'nd11as13'])
def test_determinism_and_job_order(band):
    """J: two calls give the same bits; 17 jobs in another order (every job
    changes its XCD slot) give the permuted rows bit for bit"""
    base = gt.cases()['B-1x17-own']
    J = 17
    v = np.stack([np.linspace(-300. + 3.7 * k, 300. - 2.1 * k, 70) for k in range(J)])
    case = gt._case('J-order', base['arms'], 5, True, gt.PARAMS, base['job_spec'],
                    base['job_templ'], v)
    a, sa = run(case, band)
    b, sb = run(case, band)
    assert np.all(sa == 0) and _same_bits(a, b) and np.array_equal(sa, sb)
    perm = np.random.RandomState(17).permutation(J)
    assert np.sum((perm % 8) != (np.arange(J) % 8)) >= 12
    c, sc = run(case, band, order=perm)
    assert np.all(sc == 0) and _same_bits(c, a[perm])
    assert worst_error(case, band, a) <= BOUND
