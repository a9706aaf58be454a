"""The 80-bit reference of the cross-correlation stage (tests/xcorr_truth.py) pinned
without a GPU, and the host-side halves of tests/test_xcorr_shapes.py: the lag
positions rvs_ccf_fft_pos hands out and the argument checks of rvs_ccf_xcorr."""
import os
import subprocess

import numpy as np
import pytest
import scipy.interpolate

import xcorr_truth as xt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NFFTS = [64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]


@pytest.fixture(scope='module')
def lib():
    so = os.path.join(REPO, 'rvspecfit_amd', 'librvsgpu.so')
    if not os.path.exists(so):
        subprocess.check_call(['make', '-C',
                               os.path.join(REPO, 'rvspecfit_amd', 'csrc'), '-j8'],
                              stdout=subprocess.DEVNULL)
    from rvspecfit_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize('nfft,B,T', [(64, 3, 4), (512, 2, 3), (4096, 1, 1)])
def test_fft_evaluator_equals_direct_sums(nfft, B, T):
    """the complex256 transforms against sums with no transform in them, at EVERY
    lag: 1e-17 of the largest value (the float64 kernels are held to 1e-12)"""
    spec, ivar, tmod = xt.operands(np.random.RandomState(nfft), nfft, B, T)
    f0, f1 = xt.correlations_fft(spec, ivar, tmod)
    d0, d1 = xt.correlations_direct(spec, ivar, tmod, np.arange(nfft))
    assert f0.dtype == np.longdouble and d0.dtype == np.longdouble
    for f, d in ((f0, d0), (f1, d1)):
        assert float(np.abs(f - d).max()) <= 1e-17 * float(np.abs(d).max())


@pytest.mark.parametrize('continuum', [1, 0])
@pytest.mark.parametrize('nfft', [64, 4096])
def test_truth_reproduces_the_numpy_statement(nfft, continuum):
    """the float64 statement of test_gpu_parity._xcorr_vs_numpy (np.fft, a centred
    window of 15 lags, 41 velocities) to 1e-13, by both evaluators"""
    from rvspecfit_amd import ccf_tables
    spec, ivar, tmod = xt.operands(np.random.RandomState(nfft + continuum), nfft, 3, 5)
    ind, sub = xt.lag_window(nfft, 15)
    vgrid = np.linspace(-65., 65., 41)
    ilo = ccf_tables.interp_tables(sub, vgrid)
    tfft, tfft2 = np.fft.rfft(tmod, axis=1), np.fft.rfft(tmod**2, axis=1)
    S = np.conj(np.fft.rfft(spec * ivar, axis=1))
    V = np.conj(np.fft.rfft(ivar, axis=1))
    want = np.empty((3, 5, 41))
    for b in range(3):
        for t in range(5):
            c0 = np.fft.irfft(tfft[t] * S[b], nfft)[ind]
            c1 = np.fft.irfft(tfft2[t] * V[b], nfft)[ind]
            y = (-2 * c0 + c1) if continuum else (-c0**2 / c1)
            want[b, t] = (y[ilo + 1] - y[ilo]) / (sub[ilo + 1] - sub[ilo]) * \
                (vgrid - sub[ilo]) + y[ilo]
    for direct in (False, True):
        got = xt.xcorr_truth(spec, ivar, tmod, ind, sub, vgrid, ilo, continuum,
                             direct=direct)
        assert got.shape == want.shape and got.dtype == np.longdouble
        assert float(np.abs(got - want).max()) <= 1e-13 * np.abs(want).max()


def test_lag_window_is_lag_tables():
    """the centred windows of the GPU module are the product's (ccf_tables.lag_tables,
    fitter_ccf.py:136-154), lag for lag"""
    from rvspecfit_amd import ccf_tables
    npoints = 4096
    for nlag in (3, 23, 117, 511):
        logl1 = npoints * np.log(1 + 10.0 / 3e5)
        step, ind, sub = ccf_tables.lag_tables(0.0, logl1, npoints,
                                               (nlag // 2 - 0.5) * 10.0)
        i2, s2 = xt.lag_window(npoints, nlag, step)
        assert np.array_equal(ind, i2) and np.array_equal(sub, s2)


def test_interpolation_is_interp1d():
    from rvspecfit_amd import ccf_tables
    rng = np.random.RandomState(5)
    sub = np.cumsum(rng.uniform(0.5, 2.0, 57)) - 30.0   # uneven lag velocities
    y = rng.standard_normal((2, 3, 57))
    vgrid = xt.velocity_grid(sub, 203, rng)
    assert vgrid[0] == sub[0] and vgrid[-1] == sub[-1]
    assert np.isin(vgrid, sub).sum() >= 57 and (~np.isin(vgrid, sub)).sum() >= 100
    want = scipy.interpolate.interp1d(sub, y, kind='linear', axis=2,
                                      assume_sorted=True)(vgrid)
    got = xt.interp_linear(sub, y.astype(np.longdouble), vgrid,
                           ccf_tables.interp_tables(sub, vgrid))
    np.testing.assert_allclose(got.astype(np.float64), want, rtol=0, atol=1e-14)


def test_fft_pos_is_a_bijection(lib):
    """rvs_ccf_fft_pos(nfft, .) (the digit reversal of the plan 8, 8, ..., 4 | 2) maps
    0 .. n2 - 1 onto itself for every transform size rvs_ccf_xcorr accepts: two lags
    never share a slot of the LDS image"""
    for nfft in NFFTS:
        n2 = nfft // 2
        pos = np.array([lib.rvs_ccf_fft_pos(nfft, f) for f in range(n2)])
        assert np.array_equal(np.sort(pos), np.arange(n2)), nfft


def test_xcorr_argument_bounds_without_gpu(lib):
    """rvs_ccf_xcorr's checks come before any launch (ccf_fft.hip, head of the entry
    point): T outside 1 .. 65535 (the per-pair grid's x extent), nlag < 2, nvel < 1,
    nfft outside 64 .. 16384, and lag arrays that do not fit the block's LDS"""
    E_ARG = -1

    def call(nfft=64, B=1, T=1, nlag=5, nvel=5):
        return lib.rvs_ccf_xcorr(None, None, nfft, B, None, None, T, None, 1, None,
                                 None, nlag, None, None, nvel, 0., None, None, None,
                                 None)
    assert call(T=0) == E_ARG
    assert call(T=65536) == E_ARG
    assert call(B=0) == E_ARG
    assert call(nlag=1) == E_ARG
    assert call(nvel=0) == E_ARG
    assert call(nfft=32) == E_ARG
    assert call(nfft=32768) == E_ARG
    # image + twiddles + 2 nlag doubles <= 159 KB: 5568 lags at 8192, 960 at 16384
    assert call(nfft=8192, nlag=5569) == E_ARG
    assert call(nfft=16384, nlag=961) == E_ARG
