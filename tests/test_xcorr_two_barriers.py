"""ccf_xcorr_ws_kernel<12, RATIO> (nfft 8192) after its block went from four barriers per
template to two: pass 1 and the folded pass of a consumer wave stay inside the wave's own
512 points of the image (no block barrier between them), the lane that holds a
64-block's sums stores the block's lags itself (a table built from lag_pos: block, end 0
or 63, real or imaginary part -> lag), and the interpolation of template t runs while the
block already transforms template t + 1.  What a missing barrier or a wrong table entry
would give is checked lag by lag:

 (a) the persistent kernel against the 80-bit truth of tests/xcorr_truth.py and against
     the per-pair kernel (option xc_ws = 0), every (spectrum, template) row,
 (b) every template of a spectrum as exact as its first (a stale lag value or image of
     template t - 1 shows from the second template on),
 (c) two launches on the same inputs: the same bits.

Calls go through test_xcorr_shapes.Arm (host-built operands, prune mask by the header's
rule, guarded work buffer)."""
import numpy as np
import pytest

import xcorr_truth as xt
from test_xcorr_shapes import Arm, TOL, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

NFFT = 8192
_ARMS = {}


def _arm(B, T, seed=0):
    key = (B, T, seed)
    if key not in _ARMS:
        spec, ivar, tmod = xt.operands(np.random.RandomState(NFFT + 31 * T + seed),
                                       NFFT, B, T)
        _ARMS[key] = (Arm(spec, ivar, tmod), spec, ivar, tmod)
    return _ARMS[key]


def _window(nlag, first=None):
    """the centred window of an odd nlag (the product's), an even one about lag 0, or
    nlag lags from `first`"""
    if first is None and nlag % 2 == 0:
        first = NFFT - nlag // 2
    return xt.lag_window(NFFT, nlag, first=first)


def _folded(arm, ind):
    """do all lags sit on position 0 or 63 of a 64-block of the transformed image (the
    form whose schedule changed)?  The other windows take the kernel's unfolded passes,
    which keep a barrier behind each."""
    e = arm.fpos[ind >> 1] & 63
    return bool(np.all((e == 0) | (e == 63)))


def _launch(arm, ind, sub, vgrid, continuum, ws, betas=(0.0, 1.0)):
    """[B, T, nvel] after one call per beta into a NaN-filled, guarded buffer"""
    cbuf, flat = _guarded(arm.B * arm.T * len(vgrid))
    flat.fill_(float('nan'))
    out = flat.view(arm.B, arm.T, len(vgrid))
    with arm._lib.option('xc_ws', ws):
        for beta in betas:
            assert arm.call(ind, sub, vgrid, continuum, beta, out)
            _guards_intact(cbuf, 'chisq')
    return out.cpu().numpy()


def _rows_rel(got, want):
    """|got - want| / max|want| per (b, t) row"""
    err = np.abs(got.astype(np.longdouble) - want).max(axis=2)
    return (err / np.abs(want).max(axis=2)).astype(np.float64)


def _both_forms(arm, spec, ivar, tmod, ind, sub, vgrid, continuum, rows=None, what=''):
    """(a) and (b) for one case; `rows`: the spectra whose truth is formed (all)"""
    from rvspecfit_amd import ccf_tables
    rows = np.arange(arm.B) if rows is None else np.asarray(rows)
    ilo = ccf_tables.interp_tables(sub, vgrid)
    want = 2 * xt.xcorr_truth(spec[rows], ivar[rows], tmod, ind, sub, vgrid, ilo,
                              continuum)
    got_ws = _launch(arm, ind, sub, vgrid, continuum, 1)
    got_pp = _launch(arm, ind, sub, vgrid, continuum, 0)
    assert np.all(np.isfinite(got_ws)), what
    form = 'ws12' if continuum else 'ws12r'
    rel_ws, rel_pp = _rows_rel(got_ws[rows], want), _rows_rel(got_pp[rows], want)
    print('xcorr-2bar %-5s ws %.3e pair %.3e  %s' % (form, rel_ws.max(), rel_pp.max(),
                                                     what))
    assert rel_ws.max() <= TOL[form], (what, rel_ws.max())
    assert rel_pp.max() <= TOL['pair'], (what, rel_pp.max())
    # every spectrum, every template: the two kernels on the same operands
    scale = np.abs(got_pp).max(axis=2, keepdims=True)
    assert np.all(np.abs(got_ws - got_pp) <= (TOL[form] + TOL['pair']) * scale), what
    # (b) a later template is no worse than the tolerance the first one meets
    if arm.T >= 2:
        assert rel_ws[:, 1:].max() <= TOL[form], (what, rel_ws[:, 1:].max())
    return got_ws


@pytest.mark.parametrize('nvel', [1, 63, 400, 512])
@pytest.mark.parametrize('nlag', [2, 23, 106, 107, 401, 512])
@pytest.mark.parametrize('continuum', [1, 0])
def test_lag_and_grid_shapes(continuum, nlag, nvel):
    """odd and even lag counts (up to 256 lags about zero are folded; 401 and 512 take
    the unfolded passes of the same kernel) against grids of 1 ... 512 velocities"""
    arm, spec, ivar, tmod = _arm(3, 5)
    ind, sub = _window(nlag)
    assert _folded(arm, ind) == (nlag <= 256)
    vgrid = xt.velocity_grid(sub, nvel, np.random.RandomState(nlag + nvel))
    _both_forms(arm, spec, ivar, tmod, ind, sub, vgrid, continuum,
                what='nlag %d nvel %d cont %d' % (nlag, nvel, continuum))


# windows of lags (first, nlag) by the place of their values in the transformed image:
# element f of the 4096-point transform lands on position 512 q0 + 64 q1 + 8 q2 + q3
# (f = q0 + 8 q1 + 64 q2 + 512 q3), lag 2 f is its real and 2 f + 1 its imaginary part
WINDOWS = [
    (0, 2),           # 64-block 0, position 0, re and im
    (126, 2),         # 64-block 63, position 0
    (NFFT - 128, 2),  # 64-block 0, position 63
    (NFFT - 2, 2),    # 64-block 63, position 63
    (NFFT - 2, 4),    # ... and across the wrap into 64-block 0
    (1, 23),          # begins on an imaginary part
    (NFFT - 127, 106),  # begins on an imaginary part at position 63, ends on a real one
    (NFFT - 128, 256),  # every 64-block, both ends, both parts: the whole lag table
    (21, 107),
]


@pytest.mark.parametrize('first,nlag', WINDOWS)
@pytest.mark.parametrize('continuum', [1, 0])
def test_lags_on_block_ends(continuum, first, nlag):
    """vgrid = sub: the interpolation returns the lag values themselves, so each entry
    of the lag table is held to the truth on its own"""
    arm, spec, ivar, tmod = _arm(3, 5)
    ind, sub = _window(nlag, first)
    assert _folded(arm, ind)
    pos = arm.fpos[ind >> 1]
    if nlag == 256:
        assert set(pos) == set(64 * np.arange(64)) | set(64 * np.arange(64) + 63)
    _both_forms(arm, spec, ivar, tmod, ind, sub, sub, continuum,
                what='first %d nlag %d cont %d' % (first, nlag, continuum))


@pytest.mark.parametrize('T', [1, 2, 3, 76])
@pytest.mark.parametrize('continuum', [1, 0])
def test_template_walk(continuum, T):
    """300 spectra (more persistent blocks than the chip has CUs) x T templates, 107
    lags onto 400 velocities: truth for the first and last spectra of the batch and one
    either side of 256; every row of the two kernels against each other; beta = 0 then
    1; and the same call twice gives the same bits (T = 1 is the per-pair kernel's)"""
    B = 300
    arm, spec, ivar, tmod = _arm(B, T)
    ind, sub = _window(107)
    vgrid = xt.velocity_grid(sub, 400, np.random.RandomState(T))
    got = _both_forms(arm, spec, ivar, tmod, ind, sub, vgrid, continuum,
                      rows=[0, 255, 256, B - 1], what='T %d cont %d' % (T, continuum))
    again = _launch(arm, ind, sub, vgrid, continuum, 1)
    assert got.tobytes() == again.tobytes()
    # the first call alone (beta = 0 overwrites): half of the accumulated pair, exactly
    once = _launch(arm, ind, sub, vgrid, continuum, 1, betas=(0.0,))
    assert np.array_equal(once + once, got)


@pytest.mark.parametrize('continuum', [1, 0])
def test_same_bits_unfolded_and_folded(continuum):
    """two launches, same bits, on both forms of the last two passes"""
    arm, spec, ivar, tmod = _arm(3, 5)
    for nlag in (256, 401):
        ind, sub = _window(nlag)
        vgrid = xt.velocity_grid(sub, 400, np.random.RandomState(nlag))
        a = _launch(arm, ind, sub, vgrid, continuum, 1)
        b = _launch(arm, ind, sub, vgrid, continuum, 1)
        assert a.tobytes() == b.tobytes(), nlag
