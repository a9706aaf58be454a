"""Pins tests/chisq_grid_resol_truth.py, the exact reference of the velocity-grid
chi^2 under a banded resolution matrix, without a device: the band product against
scipy.sparse, the whole value against the oracle's get_chisq, and the two figures
the device test (test_chisq_grid_resol_gpu.py) takes its bounds from."""
import numpy as np
import pytest

import chisq_grid_resol_truth as gt
from chisq_truth import chisq0_longdouble
from conftest import GOLD_CONFIG, gold_specdata
from oracle import rvs_oracle as orc


@pytest.mark.parametrize('nd', [1, 3, 11, 33])
@pytest.mark.parametrize('npix', [2, 5, 301])
def test_band_product_against_scipy_sparse(nd, npix):
    """bands whose first and last (nd - 1) / 2 rows are non-trivial, arms shorter
    than the half band included"""
    taps = gt.band_taps(npix, nd, seed=1000 * nd + npix)
    m = (nd - 1) // 2
    # every tap that refers to a pixel of the arm is there, the others are zero
    col = np.arange(npix)[:, None] - m + np.arange(nd)[None, :]
    inside = (col >= 0) & (col < npix)
    assert np.all(taps[inside] > 0) and np.all(taps[~inside] == 0)
    R = gt.taps_to_sparse(taps)
    assert np.array_equal(gt.taps_from_sparse(R, nd), taps)
    raw = np.random.RandomState(npix).uniform(0.2, 1.5, (3, npix))
    got = gt.apply_band(taps, raw.astype(gt.LD))
    want = np.stack([R @ r for r in raw])
    # nd products of O(1) numbers, float64 rounding of the sparse product
    assert np.max(np.abs(got.astype(np.float64) - want)) <= nd * 2.3e-16 * np.max(want)
    # zero diagonals added on both sides: the same product, bit for bit
    if nd < 33:
        again = gt.apply_band(gt.pad_taps(taps, nd + 2), raw.astype(gt.LD))
        assert np.array_equal(again, got)


def test_batched_qr_is_chisq0_longdouble():
    c = gt.cases()['C-16-rbf']
    (coef, knots), = gt.host_case_records(c)
    arm = c['arms'][0]
    lam = arm['grids'][0]
    vels = np.array([-310., 12.5, 295.])
    mm = gt.model(coef[0], knots, lam, arm['bands']['nd11'][0], vels)
    for npoly, rbf in ((1, True), (10, True), (16, False)):
        P = orc.get_poly_basis(lam, npoly, rbf=rbf)
        got = gt.chisq0_longdouble_batch(arm['spec'][0], mm, P, arm['espec'][0])
        for g, t in zip(got, mm):
            want = chisq0_longdouble(arm['spec'][0], t, P, arm['espec'][0])
            assert abs(g - want) <= 1e-17 * max(abs(want), len(lam))


@pytest.mark.parametrize('npoly', [5, 10, 15])
def test_truth_against_oracle_get_chisq(cases, gold_libs, npoly):
    """the golden arms with a resolution matrix given both ways
    (`resol_params`, SpecData.resolution), three velocities"""
    sds = gold_specdata(cases, 'c1', orc.SpecData)
    p = tuple(cases['c1/truth'])
    mats = {sd.name: orc.construct_resol_mat(sd.lam, width=w).tocsr()
            for sd, w in zip(sds, (0.75, 1.1))}
    own = [orc.SpecData(sd.name, sd.lam, sd.spec, sd.espec, badmask=sd.badmask,
                        resolution=mats[sd.name]) for sd in sds]
    npix = sum(len(sd.lam) for sd in sds)
    worst = 0.0
    for vel in (-871.3, -212.7, 455.):
        want = orc.get_chisq(sds, vel, p, None, dict(npoly=npoly), GOLD_CONFIG,
                             gold_libs, use_c=True, resol_params=mats)
        assert want == orc.get_chisq(own, vel, p, None, dict(npoly=npoly),
                                     GOLD_CONFIG, gold_libs, use_c=True)
        tot = gt.LD(0)
        for sd in sds:
            coef, knots = gt.host_records(sd.name, [p])
            R = mats[sd.name]
            nd = 2 * int(np.max(np.abs(R.tocoo().col - R.tocoo().row))) + 1
            tot += gt.chisq_grid_truth(
                coef[0], knots, sd.lam, sd.spec, sd.espec,
                orc.get_poly_basis(sd.lam, npoly), gt.taps_from_sparse(R, nd),
                [vel])[0]
        worst = max(worst, float(abs(tot - want)) / max(abs(want), npix))
    print('truth against get_chisq, npoly %d: %.3g' % (npoly, worst))
    assert worst <= 1e-12


def test_range_rule():
    knots = gt.oracle_lib('gold_r').lam
    lam = gt.golden_lam('gold_r')
    c = gt.C_KMS

    def vel_of(r):      # velocity whose Doppler factor is r
        return c * (1 - r * r) / (1 + r * r)
    lo = vel_of((knots[0] - 0.5) / lam[0])       # first pixel below the knots
    hi = vel_of((knots[-1] + 0.5) / lam[-1])     # last pixel behind them
    v = np.array([0., lo, hi, 0.9 * lo, 0.9 * hi])
    assert list(gt.in_range(knots, lam, v)) == [True, False, False, True, True]
    # exactly on the first knot is inside, exactly on the last is not
    assert gt.in_range(knots, knots[:5], [0.])[0]
    assert not gt.in_range(knots, knots[-5:], [0.])[0]
    coef, _ = gt.host_records('gold_r', [gt.PARAMS[0]])
    arm = gt.cases()['B-1x17-shared']['arms'][0]
    out = gt.chisq_grid_truth(coef[0], knots, lam, arm['spec'][0], arm['espec'][0],
                              orc.get_poly_basis(lam, 5), arm['bands']['nd9'][0], v)
    assert list(np.isfinite(out.astype(np.float64))) == [True, False, False, True,
                                                         True]


def test_inputs_are_at_snr_30_and_seeded():
    cs = gt.cases()
    assert len(cs) == len(gt.A_NPIX) + 2 * len(gt.B_SHAPES) + len(gt.C_BASES) + 5
    for c in cs.values():
        for arm in c['arms']:
            fin = np.isfinite(arm['espec'])
            r = np.abs(arm['spec'][fin]) / arm['espec'][fin]
            assert 20 < np.median(r) < 40 or arm['spec'].shape[1] < 12
    # the same arrays from a fresh generator
    keep = dict(gt._cases)
    gt._cases.clear()
    try:
        again = gt.cases()
        for k, c in keep.items():
            for a, b in zip(c['arms'], again[k]['arms']):
                assert np.array_equal(a['spec'], b['spec'])
                assert all(np.array_equal(a['bands'][x], b['bands'][x])
                           for x in a['bands'])
    finally:
        gt._cases.clear()
        gt._cases.update(keep)


def test_emulation_worst_is_reproduced():
    """the number the device bound rests on: the float64 statement of the
    device's arithmetic against the truth over the inputs of sweeps A-F"""
    per = gt.emulation_worst(per_case=True)
    worst = max(per.values())
    print('emulation against truth, worst of %d cases: %.3g (%s)' % (
        len(per), worst, max(per, key=per.get)))
    assert gt.EMULATION_WORST / 2 <= worst <= 2 * gt.EMULATION_WORST
    # above this the inputs, not the kernels, would decide the device test
    assert worst <= 1e-11 and gt.EMULATION_WORST <= 1e-11


def test_ill_conditioned_cases_are_the_recorded_ones():
    """sweep H: the emulation error of every case; those above 5e-8 are the ones
    the device has to flag.  (Errors of a near-singular factorisation move with
    the order of the sums: the list has to be reproduced within a factor 2 of
    the threshold, not digit for digit.)"""
    got = gt.h_emulation_errors()
    assert set(got) == set(gt.H_EMULATION)
    for k in sorted(got):
        print(k, 'recorded %.3g now %.3g' % (gt.H_EMULATION[k], got[k]))
    listed = set(gt.h_must_flag())
    assert len(listed) == 12
    assert listed <= {k for k, v in got.items() if v > gt.H_FLAG_ABOVE / 2}
    assert {k for k, v in got.items() if v > 2 * gt.H_FLAG_ABOVE} <= listed
    # without inflated errors the same arithmetic is at the level of sweeps A-F
    coef, knots = gt.host_records('gold_b', [gt.H_PARAM])
    for nd in gt.H_ND:
        spec, espec, taps = gt.h_spectra(nd)
        sp0 = gt.model(coef[0], knots, gt.H_LAM, taps, [30.])[0].astype(np.float64)
        for i, (snr, _, _) in enumerate(gt.H_SPECTRA[::4]):
            P = orc.get_poly_basis(gt.H_LAM, 10)
            a = (coef[0], knots, gt.H_LAM, spec[4 * i], sp0 / snr, P, taps, gt.H_VELS)
            e = gt.rel_err(gt.orthonormal_f64_form(*a), gt.chisq_grid_truth(*a),
                           len(gt.H_LAM)).max()
            assert e < (1e-11 if snr == 30. else 1e-8), (nd, snr, e)
