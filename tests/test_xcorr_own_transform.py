"""ccf_xcorr_ws_kernel<12, RATIO> (nfft 8192) now transforms its own spectrum: the block
packs the rows proc_spec * proc_ivar and proc_ivar into its two LDS images, runs the four
forward radix-8 passes on both, unfolds S*, V* of every producer lane's bin pairs from LDS
and parks the DC / Nyquist bins in LDS, where ccf_rfft_kernel<false> used to write all of
that to `work` in a launch of its own.  Checked here, through the C ABI:

 * every (spectrum, template) row against the per-pair kernel (option xc_ws = 0, which
   still goes through ccf_rfft_kernel) and against numpy's rfft / irfft
   (fitter_ccf.py:126-161, 189-216), at the tolerance the project uses for the same
   formulas compiled twice: rtol 1e-12, atol 1e-12 max|reference|;
 * T = 1 (rvs_ccf_xcorr keeps the per-pair kernel for a single template), 2 and 3 (the
   persistent block's walk of even and odd length behind its prologue);
 * nlag 23 and 24 (an odd count pads c0 to a whole double2 in front of the arrays that
   now precede the parked bins), 41 velocities, both CCF modes, beta = 0 then beta = 1
   into the same output;
 * a seeded spectrum, one whose proc_spec row is zero (S* = 0 in every bin) and one with
   a constant proc_ivar (V* has its DC bin only: the value parked in LDS carries the
   whole second correlation);
 * `work` is not touched where the block makes its own transform.

The last arm of a chunk goes through rvs_ccf_xcorr_select: the same kernel with an
epilogue in which the spectrum's block does what ccf_select_kernel does (running minimum
over the templates it stores, block-wide reduction, read-back of the winning row, first
minimum of that row, parabola, status bit).  Its res, best_ccf and status are held BIT
FOR BIT to rvs_ccf_select run on the accumulator the same call left behind: the shapes
above with three arms accumulated, two identical templates (the first wins), the minimum
on the first and on the last velocity (no parabola), NaN rows (the earliest wins; the
parabola's a2 is not positive), every row +inf (RVS_ST_CCF_FAILED), and the shapes the
entry refuses before any launch (T = 1, nfft 4096, option xc_ws = 0)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NFFT = 8192
N2 = NFFT // 2
B = 3
TMAX = 3
NVEL = 41
STEP = 10.0
SENTINEL = -12345.678
_CACHE = {}


def _operands():
    """rows as test_gpu_parity._xcorr_vs_numpy seeds them; spectrum 1 has a zero
    proc_spec row, spectrum 2 a constant proc_ivar"""
    if 'op' not in _CACHE:
        rng = np.random.RandomState(NFFT + 1)
        spec = 1 + 0.2 * rng.standard_normal((B, NFFT))
        ivar = rng.uniform(0.5, 2.0, (B, NFFT))
        tmod = 1 + 0.3 * rng.standard_normal((TMAX, NFFT))
        spec[1] = 0.0
        ivar[2] = 1.25
        _CACHE['op'] = (spec, ivar, tmod, np.fft.rfft(tmod, axis=1),
                        np.fft.rfft(tmod**2, axis=1))
    return _CACHE['op']


def _window(nlag):
    """nlag lags about zero, in order of increasing velocity (an even count has one lag
    more on the negative-index side), and the 41-point grid inside them"""
    first = NFFT - nlag // 2
    ind = ((first + np.arange(nlag)) % NFFT)[::-1].copy()
    off = NFFT // 2
    sub = np.ascontiguousarray(-((ind + off) % NFFT - off) * STEP)
    assert np.all(np.diff(sub) > 0)
    maxvel = min(-sub[0], sub[-1]) - 0.5 * STEP
    return ind, sub, np.linspace(-maxvel, maxvel, NVEL)


def _reference(T, nlag, continuum):
    """numpy: irfft of the products at the lags, interpolated; [B, T, NVEL]"""
    from rvspecfit_amd import ccf_tables
    key = ('ref', nlag, continuum)
    if key not in _CACHE:
        spec, ivar, _, tfft, tfft2 = _operands()
        ind, sub, vgrid = _window(nlag)
        lo = ccf_tables.interp_tables(sub, vgrid)
        S = np.conj(np.fft.rfft(spec * ivar, axis=1))
        V = np.conj(np.fft.rfft(ivar, axis=1))
        ref = np.empty((B, TMAX, NVEL))
        for b in range(B):
            for t in range(TMAX):
                c0 = np.fft.irfft(tfft[t] * S[b], NFFT)[ind]
                c1 = np.fft.irfft(tfft2[t] * V[b], NFFT)[ind]
                y = (-2 * c0 + c1) if continuum else (-c0**2 / c1)
                ref[b, t] = (y[lo + 1] - y[lo]) / (sub[lo + 1] - sub[lo]) * \
                    (vgrid - sub[lo]) + y[lo]
        ref.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key][:, :T]


def _tensors(nlag):
    """the device-side arguments of a call that do not depend on T, beta or the mode"""
    from rvspecfit_amd import _lib, ccf_tables
    key = ('dev', nlag)
    if key not in _CACHE:
        _lib.require_gpu()
        L = _lib.lib()
        spec, ivar, _, tfft, tfft2 = _operands()
        ind, sub, vgrid = _window(nlag)
        d = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to('cuda')
        pos = np.array([L.rvs_ccf_fft_pos(NFFT, int(n) >> 1) for n in ind])
        e = pos & 63
        assert np.all((e == 0) | (e == 63))    # the folded form of the last two passes
        pm = np.zeros(N2 // 64 + N2 // 8, dtype=np.uint8)
        for p in pos:
            pm[N2 // 64 + (int(p) >> 3)] |= 1 << (int(p) & 7)
            pm[int(p) >> 6] |= 1 << ((int(p) >> 3) & 7)
        _CACHE[key] = dict(
            spec=d(spec), ivar=d(ivar), tfft=d(tfft), tfft2=d(tfft2),
            tw=d(np.exp(2j * np.pi * np.arange(N2) / NFFT)),
            lp=d((2 * pos + (ind & 1)).astype(np.int32)), lv=d(sub), vg=d(vgrid),
            pm=d(pm), ilo=d(ccf_tables.interp_tables(sub, vgrid)))
    return _CACHE[key]


def _args(t, T, nlag, continuum, beta, out, work, nfft=NFFT, tfft=None, tfft2=None):
    """the argument list rvs_ccf_xcorr and rvs_ccf_xcorr_select share (T templates:
    the first T rows of the set, or the rows given)"""
    from rvspecfit_amd import _lib
    tfft = t['tfft'][:T] if tfft is None else tfft
    tfft2 = t['tfft2'][:T] if tfft2 is None else tfft2
    return (_lib.ptr(t['spec']), _lib.ptr(t['ivar']), nfft, B, _lib.ptr(tfft),
            _lib.ptr(tfft2), T, _lib.ptr(t['tw']), continuum, _lib.ptr(t['lp']),
            _lib.ptr(t['lv']), nlag, _lib.ptr(t['ilo']), _lib.ptr(t['vg']), NVEL, beta,
            _lib.ptr(t['pm']), _lib.ptr(out), _lib.ptr(work))


def _device(T, nlag, continuum, ws):
    """beta = 0 into a NaN-filled output, then beta = 1: twice the reference.  Returns
    the output and whether `work` came back untouched."""
    from rvspecfit_amd import _lib
    t = _tensors(nlag)
    L = _lib.lib()
    out = torch.full((B, T, NVEL), float('nan'), dtype=torch.float64, device='cuda')
    work = torch.full((B, 2, N2 + 1, 2), SENTINEL, dtype=torch.float64, device='cuda')
    with _lib.option('xc_ws', ws):
        for beta in (0.0, 1.0):
            rc = L.rvs_ccf_xcorr(*_args(t, T, nlag, continuum, beta, out, work),
                                 _lib.stream())
            assert rc == 0, rc
    torch.cuda.synchronize()
    return out.cpu().numpy(), bool((work == SENTINEL).all())


@pytest.mark.parametrize('continuum', [1, 0])
@pytest.mark.parametrize('nlag', [23, 24])
@pytest.mark.parametrize('T', [1, 2, 3])
def test_own_transform_equals_per_pair_and_numpy(T, nlag, continuum):
    want = 2 * _reference(T, nlag, continuum)
    got_ws, work_clean = _device(T, nlag, continuum, 1)
    got_pp, pp_clean = _device(T, nlag, continuum, 0)
    assert np.all(np.isfinite(got_ws))
    # the persistent block takes T >= 2 and leaves `work` alone; the per-pair kernel
    # and its ccf_rfft_kernel fill it
    assert work_clean == (T >= 2) and not pp_clean
    for name, ref in (('per-pair', got_pp), ('numpy', want)):
        scale = np.abs(ref).max()
        print('own-transform T %d nlag %d cont %d vs %-8s max|diff| / max|ref| %.3e' % (
            T, nlag, continuum, name, np.abs(got_ws - ref).max() / scale))
    for ref in (got_pp, want):
        np.testing.assert_allclose(got_ws, ref, rtol=1e-12,
                                   atol=1e-12 * np.abs(ref).max())
    # each spectrum on its own scale as well: the zero row and the constant-ivar row
    # are not to hide behind the seeded one
    for b in range(B):
        np.testing.assert_allclose(got_ws[b], got_pp[b], rtol=1e-12,
                                   atol=1e-12 * np.abs(got_pp[b]).max())


# ---- the last arm's block selects (rvs_ccf_xcorr_select) ---------------------------
NARM = 3


def _bits(x):
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else x.dtype)


def _select_both(T, nlag, continuum, old, tfft=None, tfft2=None):
    """the third arm through rvs_ccf_xcorr_select on top of `old` [B, T, NVEL] (what two
    arms left: the beta = 1 input), then rvs_ccf_select on the accumulator that call
    left.  Asserts the three outputs equal bit for bit; returns res, best_ccf, status
    and the accumulator as numpy arrays."""
    from rvspecfit_amd import _lib
    t = _tensors(nlag)
    L = _lib.lib()
    rng = np.random.RandomState(7 * T + nlag + continuum)
    sse = torch.as_tensor(rng.uniform(10.0, 20.0, (NARM, B))).to('cuda')
    out = torch.as_tensor(np.ascontiguousarray(old)).to('cuda')
    mk = lambda: (torch.full((B, 4), SENTINEL, dtype=torch.float64, device='cuda'),
                  torch.full((B, NVEL), SENTINEL, dtype=torch.float64, device='cuda'),
                  torch.zeros(B, dtype=torch.int32, device='cuda'))
    res, best, status = mk()
    rc = L.rvs_ccf_xcorr_select(
        *_args(t, T, nlag, continuum, 1.0, out, None, tfft=tfft, tfft2=tfft2),
        _lib.ptr(sse), NARM, _lib.ptr(res), _lib.ptr(best), _lib.ptr(status),
        _lib.stream())
    assert rc == 0, rc
    res2, best2, status2 = mk()
    rc = L.rvs_ccf_select(_lib.ptr(out), _lib.ptr(sse), NARM, B, T, _lib.ptr(t['vg']),
                          NVEL, _lib.ptr(res2), _lib.ptr(best2), _lib.ptr(status2),
                          _lib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert torch.equal(_bits(res), _bits(res2)), (res.cpu(), res2.cpu())
    assert torch.equal(_bits(best), _bits(best2))
    assert torch.equal(status, status2)
    return res.cpu().numpy(), best.cpu().numpy(), status.cpu().numpy(), out.cpu().numpy()


def _two_arms(T, nlag, continuum):
    """what two arms leave in the accumulator (beta = 0, then beta = 1)"""
    got, _ = _device(T, nlag, continuum, 1)
    return got


@pytest.mark.parametrize('continuum', [1, 0])
@pytest.mark.parametrize('nlag', [23, 24])
@pytest.mark.parametrize('T', [2, 3])
def test_select_in_the_last_arm_equals_rvs_ccf_select(T, nlag, continuum):
    """three arms accumulated, the third through the new entry: res, best_ccf and status
    bit for bit what rvs_ccf_select gives on the accumulator, which holds the three
    arms (three times one arm's values to the tolerance of the transform test)"""
    old = _two_arms(T, nlag, continuum)
    res, best, status, acc = _select_both(T, nlag, continuum, old)
    want = 3 * _reference(T, nlag, continuum)
    np.testing.assert_allclose(acc, want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    assert np.all(status == 0)
    assert np.all((res[:, 0] >= 0) & (res[:, 0] < T))


def test_select_unsupported_shapes_return_before_any_launch():
    """T = 1, nfft 4096 and option xc_ws = 0 do not take the persistent kernel of nfft
    8192: RVS_E_ARG, nothing written, the caller makes the two calls"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    t = _tensors(23)
    sse = torch.zeros((NARM, B), dtype=torch.float64, device='cuda')
    out = torch.full((B, TMAX, NVEL), SENTINEL, dtype=torch.float64, device='cuda')
    res = torch.full((B, 4), SENTINEL, dtype=torch.float64, device='cuda')
    best = torch.full((B, NVEL), SENTINEL, dtype=torch.float64, device='cuda')
    tail = (_lib.ptr(sse), NARM, _lib.ptr(res), _lib.ptr(best), None, _lib.stream())
    assert L.rvs_ccf_xcorr_select(*_args(t, 1, 23, 1, 0.0, out, None), *tail) == -1
    assert L.rvs_ccf_xcorr_select(*_args(t, 2, 23, 1, 0.0, out, None, nfft=4096),
                                  *tail) == -1
    with _lib.option('xc_ws', 0):
        assert L.rvs_ccf_xcorr_select(*_args(t, 2, 23, 1, 0.0, out, None), *tail) == -1
    torch.cuda.synchronize()
    for x in (out, res, best):
        assert bool((x == SENTINEL).all())
    assert L.rvs_ccf_xcorr_work_size(NFFT, B, 2, 23, NVEL, 1) == 0
    assert L.rvs_ccf_xcorr_work_size(NFFT, B, 1, 23, NVEL, 1) == B * 2 * (N2 + 1) * 2
    assert L.rvs_ccf_xcorr_work_size(4096, B, 2, 23, NVEL, 1) == B * 2 * 2049 * 2


@pytest.mark.parametrize('continuum', [1, 0])
def test_select_identical_templates_first_wins(continuum):
    """two identical templates give identical rows: the tie goes to template 0"""
    t = _tensors(23)
    f = t['tfft'][:1].repeat(2, 1).contiguous()
    f2 = t['tfft2'][:1].repeat(2, 1).contiguous()
    old = np.zeros((B, 2, NVEL))
    res, _, _, acc = _select_both(2, 23, continuum, old, tfft=f, tfft2=f2)
    assert np.array_equal(acc[:, 0], acc[:, 1])
    assert np.all(res[:, 0] == 0)


@pytest.mark.parametrize('continuum', [1, 0])
def test_select_edge_minima_nan_and_inf(continuum):
    """what the accumulated arms hold decides the branch; it is planted through the
    beta = 1 input.  Spectrum 0: the minimum on velocity 0 of template 1; spectrum 1: on
    velocity NVEL - 1 of template 2 (no parabola at either end); spectrum 2: a NaN in
    rows 2 and 1 at interior velocities (the earliest NaN row wins, its first NaN is the
    'minimum', and the parabola's a2 is NaN -- not > 0 -- so best_vel stays on the grid
    point: the branch a concave triple would take, which a first minimum on an ascending
    grid cannot produce with finite values, since there d1 < 0 <= d2)."""
    T = 3
    old = np.zeros((B, T, NVEL))
    old[0, 1, 0] = -1e12
    old[1, 2, NVEL - 1] = -1e12
    old[2, 2, 5] = np.nan
    old[2, 1, 17] = np.nan
    old[2, 1, 30] = np.nan
    res, best, status, acc = _select_both(T, 23, continuum, old)
    vg = _window(23)[2]
    assert res[0, 0] == 1 and res[0, 2] == 0 and res[0, 1] == vg[0]
    assert res[1, 0] == 2 and res[1, 2] == NVEL - 1 and res[1, 1] == vg[-1]
    assert res[2, 0] == 1 and res[2, 2] == 17 and res[2, 1] == vg[17]
    assert np.isnan(res[2, 3]) and status[2] != 0 and status[0] == 0 and status[1] == 0
    # every row +inf: best_id 0, velocity 0, the failure bit for every spectrum
    res, best, status, acc = _select_both(T, 23, continuum,
                                          np.full((B, T, NVEL), np.inf))
    assert np.all(np.isinf(acc)) and np.all(res[:, 0] == 0) and np.all(res[:, 2] == 0)
    assert np.all(status != 0)
