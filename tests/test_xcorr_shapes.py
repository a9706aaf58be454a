"""rvs_ccf_xcorr and rvs_ccf_select through the C ABI at the shapes on which their
kernels branch (csrc/ccf_fft.hip, csrc/ccf.hip), against references that share nothing
with them: the 80-bit cross-correlation of tests/xcorr_truth.py (pinned to direct sums
in tests/test_xcorr_truth_cpu.py) and a numpy restatement of fitter_ccf.py:218-236.

Every call of rvs_ccf_xcorr here goes through _run: host-built tfft, tfft2, twid,
lag_pos from rvs_ccf_fft_pos, the prune mask by the header's rule, beta = 0 into a
NaN-filled buffer (the first call overwrites) and then beta = 1 (the next arm
accumulates: twice the reference), `chisq` and `work` inside sentinel-filled margins
that must come back untouched, and every (b, t) row held to TOL[form] x max|reference|
of that row.  `form` names the kernel rvs_ccf_xcorr picks (the conditions at the end of
ccf_fft.hip restated in _form), so a failure names the kernel."""
import numpy as np
import pytest
import torch

import xcorr_truth as xt

pytestmark = pytest.mark.gpu

NFFTS = [64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384]
# asserted |device - truth| / max|truth| per (b, t) row; DESIGN.md section 2 has the
# measured worst case of each form
TOL = {'pair': 1e-14, 'ws12': 1e-14, 'ws12r': 1e-14, 'ws11r': 1e-14, 'ws2': 1e-14}
WORST = {}
GUARD = 512          # doubles of margin on each side of chisq and of work
SENTINEL = -12345.678
DEV = 'cuda'


def _lib_():
    from rvspecfit_amd import _lib
    _lib.require_gpu()
    return _lib, _lib.lib()


def _form(nfft, continuum, nlag, nvel, T, pruned, ws):
    """the kernel behind a call (rvs_ccf_xcorr: `ws_on && (p12 || p11) && nlag <=
    XW_HALF && nvel <= XW_HALF && T >= 2`)"""
    if ws and nlag <= 512 and nvel <= 512 and T >= 2:
        if nfft == 8192 and pruned:
            return 'ws12' if continuum else 'ws12r'
        if nfft == 4096:
            return 'ws2' if continuum else 'ws11r'
    return 'pair'


def _guarded(n, dtype=torch.float64):
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _guards_intact(buf, what):
    g = torch.full((GUARD,), SENTINEL, dtype=buf.dtype, device=DEV)
    assert torch.equal(buf[:GUARD], g), 'write in front of ' + what
    assert torch.equal(buf[-GUARD:], g), 'write behind ' + what


class Arm:
    """the device-side operands of one arm: built once, called many times"""

    def __init__(self, spec, ivar, tmod):
        self._lib, self.L = _lib_()
        self.B, self.nfft = spec.shape
        self.T = tmod.shape[0]
        n2 = self.nfft // 2
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
        self.spec, self.ivar = d(spec), d(ivar)
        self.tfft = d(np.fft.rfft(tmod, axis=1))
        self.tfft2 = d(np.fft.rfft(tmod**2, axis=1))
        self.twid = d(np.exp(2j * np.pi * np.arange(n2) / self.nfft))
        self.fpos = np.array([self.L.rvs_ccf_fft_pos(self.nfft, f) for f in range(n2)])

    def call(self, ind, sub, vgrid, continuum, beta, out, pruned=True, B=None, b0=0):
        """one rvs_ccf_xcorr on spectra b0 .. b0 + B - 1; `out` a [B, T, nvel] view"""
        from rvspecfit_amd import ccf_tables
        _lib, L = self._lib, self.L
        nfft, n2 = self.nfft, self.nfft // 2
        B = self.B if B is None else B
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
        pos = self.fpos[ind >> 1]
        lag_pos = d((2 * pos + (ind & 1)).astype(np.int32))
        pm = xt.prune_mask(n2, pos) if pruned else None
        prune = None if pm is None else d(pm)
        ilo = ccf_tables.interp_tables(sub, vgrid)
        t_sub, t_ilo, t_vg = d(sub), d(ilo), d(vgrid)
        wbuf, work = _guarded(B * 2 * (n2 + 1) * 2)
        rc = L.rvs_ccf_xcorr(_lib.ptr(self.spec[b0:b0 + B]), _lib.ptr(self.ivar[b0:b0 + B]),
                             nfft, B, _lib.ptr(self.tfft), _lib.ptr(self.tfft2), self.T,
                             _lib.ptr(self.twid), continuum, _lib.ptr(lag_pos),
                             _lib.ptr(t_sub), len(sub), _lib.ptr(t_ilo), _lib.ptr(t_vg),
                             len(vgrid), beta, _lib.ptr(prune), _lib.ptr(out),
                             _lib.ptr(work), _lib.stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        _guards_intact(wbuf, 'work')
        return pm is not None


def _check(got, want, form, what):
    """every (b, t) row of `got` against the longdouble `want`"""
    err = np.abs(got.astype(np.longdouble) - want).max(axis=2)
    scale = np.abs(want).max(axis=2)
    assert np.all(np.isfinite(got)), what
    rel = float((err / scale).max())
    WORST[form] = max(WORST.get(form, 0.0), rel)
    print('xcorr-err %-6s %.3e  %s' % (form, rel, what))
    assert rel <= TOL[form], (form, rel, what)


def _run(arm, truth, ind, sub, vgrid, continuum, ws=1, pruned=True, what=''):
    """beta = 0 then beta = 1 through the kernel `ws` / `pruned` select; `truth` =
    (c0, c1) of xt.correlations_fft at every lag.  Returns the device values."""
    from rvspecfit_amd import ccf_tables
    nvel = len(vgrid)
    cbuf, flat = _guarded(arm.B * arm.T * nvel)
    flat.fill_(float('nan'))
    out = flat.view(arm.B, arm.T, nvel)
    with arm._lib.option('xc_ws', ws):
        for beta in (0.0, 1.0):
            has_prune = arm.call(ind, sub, vgrid, continuum, beta, out, pruned)
            _guards_intact(cbuf, 'chisq')
    form = _form(arm.nfft, continuum, len(sub), nvel, arm.T, has_prune, ws)
    y = xt.chisq_at_lags(truth[0][:, :, ind], truth[1][:, :, ind], continuum)
    want = 2 * xt.interp_linear(sub, y, vgrid, ccf_tables.interp_tables(sub, vgrid))
    got = out.cpu().numpy()
    _check(got, want, form, '%s nfft %d cont %d nlag %d nvel %d T %d ws %d prune %d' % (
        what, arm.nfft, continuum, len(sub), nvel, arm.T, ws, has_prune))
    return got


_ARMS = {}


def _arm(nfft, B=3, T=5, seed=0):
    """operands and their all-lag truth, cached: the sweeps below reuse them"""
    key = (nfft, B, T, seed)
    if key not in _ARMS:
        spec, ivar, tmod = xt.operands(np.random.RandomState(nfft + seed), nfft, B, T)
        _ARMS[key] = (Arm(spec, ivar, tmod), xt.correlations_fft(spec, ivar, tmod))
    return _ARMS[key]


# B.1 ------------------------------------------------------------------------------
# ccf_xcorr_ws_kernel carves its LDS as  images | T1 | c0 [nlag, padded to a whole
# double2] | T1c [73 double2] | cA [nlag] (RATIO only).  Until this module came, the
# launcher asked for 16 (2 n2 + n2/8) + 8 nlag + 16 * 73 + (continuum ? 0 : 8 nlag)
# bytes: for an odd nlag without continuum normalisation 8 bytes short of cA[nlag - 1].
# The runtime rounds a request up to its allocation granule, so the shortfall showed
# only where the request ENDED on a granule:
#   nfft 8192: 140432 + 16 nlag, nlag = 23 -> 140800 = 275 * 512 = 110 * 1280
#   nfft 4096:  70800 + 16 nlag, nlag = 55 ->  71680 = 140 * 512 =  56 * 1280
# (and every nlag = 23 mod 32 for a 512-byte granule: 55, 87, 311).  There c0 of the
# last lag came back wrong, i.e. the top of the velocity grid -- which velocity_grid
# always reads (its last point is sub[-1]).  The product's nlag is always odd
# (ccf_tables.lag_tables).  2 and 512 are the ABI's even bounds of the persistent
# kernels (XW_HALF); 513 falls back to ccf_xcorr_kernel AND to its loop read-back
# (`pre` false: nlag > XB_NT).
@pytest.mark.parametrize('nlag', [2, 3, 15, 23, 55, 87, 117, 311, 511, 512, 513])
@pytest.mark.parametrize('nfft', [4096, 8192])
@pytest.mark.parametrize('continuum', [1, 0])
def test_lag_counts(nfft, continuum, nlag):
    arm, truth = _arm(nfft)
    first = None if nlag % 2 else nfft - nlag // 2
    ind, sub = xt.lag_window(nfft, nlag, first=first)
    vgrid = xt.velocity_grid(sub, min(2 * nlag + 1, 401), np.random.RandomState(nlag))
    assert vgrid[-1] == sub[-1] and np.sum(vgrid > sub[-2]) >= 2
    for ws in (1, 0):
        _run(arm, truth, ind, sub, vgrid, continuum, ws, what='lag counts')


# B.2 ------------------------------------------------------------------------------
@pytest.mark.parametrize('nvel', [1, 2, 41, 401, 511, 512, 513, 1001])
@pytest.mark.parametrize('nfft', [4096, 8192])
@pytest.mark.parametrize('continuum', [1, 0])
def test_velocity_grid_sizes(nfft, continuum, nvel):
    """nvel against the block: one interpolation per consumer lane up to XW_HALF = 512
    (persistent kernels) / XB_NT = 512 (per-pair register read-back, `pre`), the
    `tid < nvel` / clamped `min(tid, nvel - 1)` loads at 1 and 2, and beyond 512 the
    per-pair kernel's strided loop -- 1001 is the grid ccf_tables.ccf_vel_grid builds
    when the configuration names no step (vel_step0 = 2, max_vel 1000).  Grid points on
    lag velocities, strictly inside intervals and on both ends of sub."""
    arm, truth = _arm(nfft)
    ind, sub = xt.lag_window(nfft, 117)
    vgrid = xt.velocity_grid(sub, nvel, np.random.RandomState(nvel))
    for ws in (1, 0):
        _run(arm, truth, ind, sub, vgrid, continuum, ws, what='grid sizes')


# B.3 ------------------------------------------------------------------------------
@pytest.mark.parametrize('nfft', NFFTS)
@pytest.mark.parametrize('continuum', [1, 0])
def test_every_output_bin(nfft, continuum):
    """every output of the inverse transform of every plan (8,8 / 8,8,2 / 8,8,4 / 8,8,8
    / ... / 8,8,8,8,2): a window of <= 511 consecutive lags slides across all nfft of
    them, vgrid = sub so that the interpolation returns the lag values.  This is the
    register read-back (`pre`), at 4096 / 8192 also the persistent kernels, and where
    n2 is a power of 8 (128, 1024, 8192) a different prune mask per window: away from
    lag 0 the masks fail the fold's vote (`bad`) and the two masked passes run as
    written.  8192 also without a mask (the unpruned per-pair transform).  Then all
    lags in one call where the lag arrays fit the block's LDS beside the image (159 KB):
    nlag = nfft up to 4096, 5567 lags at 8192, 959 at 16384 -- the loop read-back."""
    arm, truth = _arm(nfft, B=2, T=3)
    w = min(511, nfft)
    for first in range(0, nfft, w):
        ind, sub = xt.lag_window(nfft, w, first=first)
        kinds = [(1, True)]
        if nfft in (4096, 8192):
            kinds.append((0, True))
        if nfft == 8192:
            kinds.append((1, False))
        for ws, pruned in kinds:
            _run(arm, truth, ind, sub, sub, continuum, ws, pruned, what='bins @%d' % first)
    nall = {8192: 5567, 16384: 959}.get(nfft, nfft)
    if nall > w:
        ind, sub = xt.lag_window(nfft, nall, first=nfft - nall // 2)
        _run(arm, truth, ind, sub, sub, continuum, what='all lags')


# B.4 ------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 2, 3, 76, 77])
@pytest.mark.parametrize('nfft', [4096, 8192])
@pytest.mark.parametrize('continuum', [1, 0])
def test_template_counts(nfft, continuum, T):
    """T = 1 takes ccf_xcorr_kernel (`T >= 2` of the persistent forms); 2, 3, 76, 77 the
    even and odd tails of ccf_xcorr_ws2_kernel's pairing (`two`, tq's clamp: an odd T
    forms its last template twice and must not write the copy) and the 2 T image
    iterations of the RATIO forms"""
    arm, truth = _arm(nfft, B=2, T=T, seed=T)
    ind, sub = xt.lag_window(nfft, 23)
    vgrid = xt.velocity_grid(sub, 41, np.random.RandomState(T))
    _run(arm, truth, ind, sub, vgrid, continuum, what='template counts')


@pytest.mark.parametrize('continuum', [1, 0])
def test_template_count_upper_bound(continuum):
    """T = 65535 (the ABI's bound) at nfft 64: 69 MB of template spectra, above the
    16 MB of xc_group, so the blocks take the grouped xc_job order (G = 1985, five
    groups of which the last is mostly padding blocks) at a second size beside
    test_xcorr_large_template_set_job_map's T = 140 at 8192"""
    spec, ivar, tmod = xt.operands(np.random.RandomState(3), 64, 2, 65535)
    arm, truth = Arm(spec, ivar, tmod), xt.correlations_fft(spec, ivar, tmod)
    ind, sub = xt.lag_window(64, 15)
    vgrid = xt.velocity_grid(sub, 21, np.random.RandomState(1))
    _run(arm, truth, ind, sub, vgrid, continuum, what='T bound')


# B.5 ------------------------------------------------------------------------------
def test_batch_above_one_grid():
    """B = 65537 at nfft 64, T = 2 (G == 0): ccf_xcorr_kernel's grid is (T, B) and a
    grid's y extent ends at 65535, so the launch loop at the end of rvs_ccf_xcorr runs
    twice, 65535 + 2 spectra, the second through `work + b0 * 2 * (n2 + 1)` and
    `chisq + b0 * T * nvel`.  Every row against the truth; the last three rows equal the
    same spectra run as a batch of three, bit for bit."""
    from rvspecfit_amd import ccf_tables
    B, T, nfft = 65537, 2, 64
    spec, ivar, tmod = xt.operands(np.random.RandomState(7), nfft, B, T)
    arm = Arm(spec, ivar, tmod)
    ind, sub = xt.lag_window(nfft, 15)
    vgrid = xt.velocity_grid(sub, 21, np.random.RandomState(2))
    ilo = ccf_tables.interp_tables(sub, vgrid)
    for continuum in (1, 0):
        cbuf, flat = _guarded(B * T * len(vgrid))
        flat.fill_(float('nan'))
        out = flat.view(B, T, len(vgrid))
        arm.call(ind, sub, vgrid, continuum, 0.0, out)
        _guards_intact(cbuf, 'chisq')
        got = out.cpu().numpy()
        for b0 in range(0, B, 8192):   # (the truth in slices: 80-bit arrays are large)
            sl = slice(b0, min(b0 + 8192, B))
            want = xt.xcorr_truth(spec[sl], ivar[sl], tmod, ind, sub, vgrid, ilo, continuum)
            _check(got[sl], want, 'pair', 'B 65537 rows %d.. cont %d' % (b0, continuum))
        tail = torch.full((3, T, len(vgrid)), float('nan'), dtype=torch.float64,
                          device=DEV)
        arm.call(ind, sub, vgrid, continuum, 0.0, tail, B=3, b0=B - 3)
        assert np.array_equal(got[B - 3:], tail.cpu().numpy())


# B.6 ------------------------------------------------------------------------------
@pytest.mark.parametrize('continuum', [1, 0])
def test_accumulation_across_kernel_forms(continuum):
    """three arms into ONE chisq buffer, as fitter_ccf sums them: nfft 8192 with beta =
    0 into NaN (persistent ccf_xcorr_ws_kernel<12, .>), 4096 with beta = 1
    (ccf_xcorr_ws2_kernel, or <11, true> without continuum normalisation), 2048 with
    beta = 1 (ccf_xcorr_kernel): `beta * old + value` of each form, the sum of the three
    truths"""
    from rvspecfit_amd import ccf_tables
    B, T = 3, 5
    vgrid = np.linspace(-100., 100., 81)
    cbuf, flat = _guarded(B * T * len(vgrid))
    flat.fill_(float('nan'))
    out = flat.view(B, T, len(vgrid))
    want = 0
    forms = []
    for k, (nfft, step) in enumerate(((8192, 10.0), (4096, 13.0), (2048, 17.0))):
        arm, truth = _arm(nfft, B, T, seed=k)
        ind, sub = xt.lag_window(nfft, 2 * int(100 / step + 1) + 1, step)
        has_prune = arm.call(ind, sub, vgrid, continuum, float(k > 0), out)
        _guards_intact(cbuf, 'chisq')
        forms.append(_form(nfft, continuum, len(sub), len(vgrid), T, has_prune, 1))
        y = xt.chisq_at_lags(truth[0][:, :, ind], truth[1][:, :, ind], continuum)
        want = want + xt.interp_linear(sub, y, vgrid, ccf_tables.interp_tables(sub, vgrid))
    assert forms == ['ws12' if continuum else 'ws12r', 'ws2' if continuum else 'ws11r',
                     'pair']
    err = np.abs(out.cpu().numpy().astype(np.longdouble) - want).max(axis=2)
    rel = float((err / np.abs(want).max(axis=2)).max())
    print('xcorr-err %-6s %.3e  three arms cont %d' % ('sum', rel, continuum))
    assert rel <= max(TOL[f] for f in forms)


# D --------------------------------------------------------------------------------
def _select_ref(allc, vgrid):
    """fitter_ccf.py:218-236 on one spectrum's all_chisqs (total_sse added); the
    RuntimeError as a flag.  The parabola is fitted in x - x[1]: np.polyfit's
    Vandermonde matrix of velocities near +-1000 km/s at a spacing of a few km/s has a
    condition number of 1e9, and the vertex it gives carries 1e-7 km/s of polyfit's own
    rounding; shifted, the same polynomial's vertex is good to 1e-12."""
    best_id = int(np.argmin(allc.min(axis=1)))
    best_ccf = allc[best_id]
    best_pix = int(np.argmin(best_ccf))
    best_vel = vgrid[best_pix]
    failed = not np.isfinite(allc[best_id, best_pix])
    if best_pix not in [0, len(best_ccf) - 1] and \
            np.all(np.isfinite(best_ccf[best_pix - 1:best_pix + 2])):
        x = vgrid[best_pix - 1:best_pix + 2]
        coeffs = np.polyfit(x - x[1], best_ccf[best_pix - 1:best_pix + 2], deg=2)
        if coeffs[0] > 0:
            best_vel = x[1] - coeffs[1] / (2 * coeffs[0])
    return best_id, best_pix, best_vel, best_ccf, failed


def _same_bits(a, b):
    """bit for bit, NaN for NaN (whatever its payload)"""
    n = np.isnan(a)
    return np.array_equal(n, np.isnan(b)) and a[~n].tobytes() == b[~n].tobytes()


def _select_surfaces(rng, B, T, nvel):
    """[B, T, nvel]: random surfaces, the first rows each with one of the cases on
    which ccf_select_kernel's order (nan_less: NaN first, then value, then the index
    t * nvel + v) or its vertex (`bp != 0 && bp != nvel - 1`, `a2 > 0`) decides"""
    c = rng.standard_normal((B, T, nvel))
    t1, t2 = 0, T - 1
    tm = T // 2
    va, vb = nvel // 3, nvel - 1 - nvel // 4
    inf = np.inf
    b = iter(range(B))
    k = next(b); c[k, t1, vb] = -9.0; c[k, t2, va] = -9.0       # tie across templates
    c[next(b), tm, [va, vb]] = -9.0                             # tie inside a row
    k = next(b); c[k, t1, va] = -9.0; c[k, t2, vb] = np.nan     # NaN behind the minimum
    k = next(b); c[k, t2, va] = -9.0; c[k, t1, vb] = np.nan     # NaN before it
    k = next(b); c[k, t2, va] = np.nan; c[k, tm, vb] = np.nan   # NaN in two rows
    k = next(b); c[k, t1, :] = inf                              # a row of +inf
    c[next(b)] = inf                                            # everything +inf
    c[next(b), tm, 0] = -9.0                                    # minimum on velocity 0
    c[next(b), tm, nvel - 1] = -9.0                             # ... on the last one
    # a straight line and a concave row far below the rest: the three points about
    # the minimum can be collinear or concave only with the minimum on an end (a
    # strict interior minimum has d1 < 0 <= d2, a2 > 0), which takes vgrid[bp]
    k = next(b); c[k, tm, :] = -50.0 - np.arange(nvel)
    k = next(b); c[k, tm, :] = -50.0 - (np.arange(nvel) - (nvel - 1) / 2.0)**2
    # ... or with a NaN as the "minimum" inside the row: a2 is NaN, `a2 > 0` fails
    k = next(b); c[k, tm, nvel // 2] = np.nan
    k = next(b); c[k, tm, nvel // 2] = -inf                     # not finite: failed
    return c


@pytest.mark.parametrize('T,nvel,narm', [
    (1, 1, 1), (255, 1, 3), (128, 2, 1), (257, 1, 1), (85, 3, 3), (5, 401, 3),
    (76, 401, 3), (3, 1001, 1), (7, 41, 3)])
def test_select_vs_numpy(T, nvel, narm):
    """rvs_ccf_select (ccf.hip: ccf_select_kernel, one 256-thread block per spectrum)
    against numpy's argmin semantics.  T * nvel = 1, 255, 256, 257 and 76 * 401 put the
    strided scan `e = tid; e < T * nvel; e += 256` below, on and beyond one trip with
    idle lanes holding (+inf, 2^62); nvel 1 and 2 have no interior point; best_ccf is
    `row + tot` with tot summed over narm in arm order; B = 300 blocks; an unevenly
    spaced vgrid; a status word that already holds another bit."""
    _lib, L = _lib_()
    rng = np.random.RandomState(T * nvel + narm)
    B = 300
    chisq = _select_surfaces(rng, B, T, nvel)
    sse = rng.uniform(1e3, 2e4, (narm, B))
    vgrid = np.cumsum(rng.uniform(1.0, 9.0, nvel)) - 2.5 * nvel - 1000.0
    d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    t_c, t_s, t_v = d(chisq), d(sse), d(vgrid)
    rbuf, res = _guarded(B * 4)
    bbuf, best = _guarded(B * nvel)
    st0 = np.where(np.arange(B) % 2, _lib.ST_ALLMASKED, 0).astype(np.int32)
    status = d(st0)
    rc = L.rvs_ccf_select(_lib.ptr(t_c), _lib.ptr(t_s), narm, B, T, _lib.ptr(t_v), nvel,
                          _lib.ptr(res), _lib.ptr(best), _lib.ptr(status), _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    _guards_intact(rbuf, 'res')
    _guards_intact(bbuf, 'best_ccf')
    res = res.cpu().numpy().reshape(B, 4)
    best = best.cpu().numpy().reshape(B, nvel)
    status = status.cpu().numpy()
    nfail = 0
    for b in range(B):
        tot = 0.0
        for a in range(narm):
            tot += sse[a, b]
        bid, bpix, bvel, bccf, failed = _select_ref(chisq[b] + tot, vgrid)
        assert res[b, 0] == bid, (b, res[b], bid)
        assert res[b, 2] == bpix, (b, res[b], bpix)
        assert _same_bits(best[b], bccf), b
        assert _same_bits(res[b, 3:4], bccf[bpix:bpix + 1]), b
        assert status[b] == (st0[b] | (_lib.ST_CCF_FAILED if failed else 0)), b
        if not failed:
            assert abs(res[b, 1] - bvel) <= 1e-9, (b, res[b, 1], bvel)
        elif np.isnan(bccf[bpix]) or bpix in (0, nvel - 1):
            assert res[b, 1] == vgrid[bpix], b
        nfail += failed
    assert nfail >= (3 if T * nvel > 1 else 1)
