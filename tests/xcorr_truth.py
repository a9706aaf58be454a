"""Extended-precision statement of what rvs_ccf_xcorr computes for one arm
(fitter_ccf.py:189-216), used as the truth of tests/test_xcorr_shapes.py and pinned
without a GPU by tests/test_xcorr_truth_cpu.py.  Everything is np.longdouble (x87
80-bit, eps 1.1e-19), so the reference's own rounding is four orders below the
float64 kernels':

  c0[b, t, m] = sum_n tmod[t, (n + m) mod N] (spec ivar)[b, n]
  c1[b, t, m] = sum_n tmod[t, (n + m) mod N]^2 ivar[b, n]

which is the orientation of np.fft.irfft(rfft(tmod) conj(rfft(spec ivar))),
  y = -2 c0 + c1 (continuum normalisation) or -c0^2 / c1 at the lags ind,
and the two-point interpolation of scipy's interp1d(kind='linear') from the lag
velocities `sub` onto `vgrid`, with ilo the bracketing index of each grid point.

Two evaluators of c0, c1: direct sums (no transform anywhere: the truth of the
truth, N^2 per row) and scipy.fft on longdouble arrays (complex256 transforms, for
the large sweeps).  The value is that of ONE call; a test that calls the entry point
with beta = 0 and then beta = 1 on the same inputs compares with twice it."""
import numpy as np
import scipy.fft

LD = np.longdouble


def _operands(spec, ivar, tmod):
    iv = np.asarray(ivar, dtype=LD)
    tm = np.asarray(tmod, dtype=LD)
    return np.asarray(spec, dtype=LD) * iv, iv, tm, tm * tm


def correlations_direct(spec, ivar, tmod, lags):
    """c0, c1 [B, T, len(lags)] by direct sums (np.sum adds pairwise)"""
    sw, iv, tm, tm2 = _operands(spec, ivar, tmod)
    N = sw.shape[1]
    c0 = np.empty((sw.shape[0], tm.shape[0], len(lags)), dtype=LD)
    c1 = np.empty_like(c0)
    for l, m in enumerate(lags):
        idx = (np.arange(N) + int(m)) % N
        c0[:, :, l] = np.sum(tm[None, :, idx] * sw[:, None, :], axis=2)
        c1[:, :, l] = np.sum(tm2[None, :, idx] * iv[:, None, :], axis=2)
    return c0, c1


def correlations_fft(spec, ivar, tmod):
    """c0, c1 [B, T, N] at every lag, through complex256 transforms"""
    sw, iv, tm, tm2 = _operands(spec, ivar, tmod)
    N = sw.shape[1]
    S = np.conj(scipy.fft.rfft(sw, axis=1))
    V = np.conj(scipy.fft.rfft(iv, axis=1))
    F, F2 = scipy.fft.rfft(tm, axis=1), scipy.fft.rfft(tm2, axis=1)
    assert S.dtype == np.clongdouble and F.dtype == np.clongdouble
    c0 = scipy.fft.irfft(F[None, :, :] * S[:, None, :], N, axis=2)
    c1 = scipy.fft.irfft(F2[None, :, :] * V[:, None, :], N, axis=2)
    return c0, c1


def interp_linear(sub, y, vgrid, ilo):
    """interp1d(sub, y, kind='linear', axis=-1, assume_sorted=True)(vgrid), given the
    bracketing indices ilo (ccf_tables.interp_tables)"""
    sub, vgrid = np.asarray(sub, dtype=LD), np.asarray(vgrid, dtype=LD)
    lo = np.asarray(ilo)
    slope = (y[..., lo + 1] - y[..., lo]) / (sub[lo + 1] - sub[lo])
    return slope * (vgrid - sub[lo]) + y[..., lo]


def chisq_at_lags(c0, c1, continuum):
    return (-2 * c0 + c1) if continuum else (-c0 * c0 / c1)


def xcorr_truth(spec, ivar, tmod, ind, sub, vgrid, ilo, continuum, direct=False):
    """[B, T, nvel] longdouble: one call of rvs_ccf_xcorr with beta = 0"""
    ind = np.asarray(ind)
    if direct:
        c0, c1 = correlations_direct(spec, ivar, tmod, ind)
    else:
        c0, c1 = (c[:, :, ind] for c in correlations_fft(spec, ivar, tmod))
    return interp_linear(sub, chisq_at_lags(c0, c1, continuum), vgrid, ilo)


# ---- case builders shared by the CPU pins and the GPU module ------------------

def lag_window(nfft, nlag, step=10.0, first=None):
    """lags and their velocities: `first` None -- the centred window of an odd nlag
    exactly as ccf_tables.lag_tables / fitter_ccf.py:136-154 select and order it; else
    nlag consecutive lags first, first + 1, ... (mod nfft) with ascending velocities
    (any window of the transform; an even nlag; nlag = nfft)"""
    if first is None:
        assert nlag % 2 == 1
        off = nfft // 2
        vels = -((np.arange(nfft) + off) % nfft - off) * step
        sel = np.abs(vels) < (nlag // 2 + 0.5) * step
        assert sel.sum() == nlag
        ind = np.roll(np.nonzero(sel)[0], nlag // 2)[::-1]
        sub = np.ascontiguousarray(vels[ind])
    else:
        ind = (first + np.arange(nlag)) % nfft
        sub = (np.arange(nlag) - (nlag - 1) / 2) * step
    assert np.all(np.diff(sub) > 0) and len(np.unique(ind)) == nlag
    return ind.astype(np.int64), sub


def velocity_grid(sub, nvel, rng):
    """nvel ascending grid points inside [sub[0], sub[-1]]: both ends of sub, lag
    velocities themselves and points strictly inside intervals, the last interval
    included"""
    if nvel == 1:
        return np.array([0.5 * (sub[-2] + sub[-1])])
    if nvel == 2:
        return np.array([sub[0], sub[-1]])
    mid = rng.uniform(sub[0], sub[-1], nvel - 2)
    k = min(len(sub), (nvel - 2) // 3)
    mid[:k] = sub[rng.choice(len(sub), k, replace=False)]
    mid[k] = 0.25 * sub[-2] + 0.75 * sub[-1]
    return np.concatenate(([sub[0]], np.sort(mid), [sub[-1]]))


def prune_mask(n2, pos):
    """the `prune` argument by the rule of include/rvsgpu.h (n2 a power of 8, >= 64),
    else None"""
    l2 = n2.bit_length() - 1
    if l2 % 3 != 0 or l2 < 6:
        return None
    pm = np.zeros(n2 // 64 + n2 // 8, dtype=np.uint8)
    for p in pos:
        pm[n2 // 64 + (int(p) >> 3)] |= 1 << (int(p) & 7)
        pm[int(p) >> 6] |= 1 << ((int(p) >> 3) & 7)
    return pm


def operands(rng, nfft, B, T):
    spec = 1 + 0.2 * rng.standard_normal((B, nfft))
    ivar = rng.uniform(0.5, 2.0, (B, nfft))
    tmod = 1 + 0.3 * rng.standard_normal((T, nfft))
    return spec, ivar, tmod
