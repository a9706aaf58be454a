"""ccf_preprocess_kernel (csrc/ccf.hip) through rvs_ccf_preprocess and
rvs_ccf_preprocess_g against the stage-by-stage truth of tests/ccf_preprocess_truth.py,
which tests/test_ccf_preprocess_truth_cpu.py pins without a GPU.  One launch per entry
of ccf_preprocess_truth.launches(), several spectra per launch; every spectrum of every
launch is held to the truth of that spectrum alone, stage by stage, each stage from the
device's own upstream output:

  status                 exactly (RVS_ST_ALLMASKED)
  pfit, fit = 'gtol'     |pfit - p0| <= 8 eps cond(C) max|p0|   (binned start alone)
  pfit, fit = 'newton'   d = |pfit - p*| <= the family's largest TRF distance
  pfit, any fit          the objective at pfit is not above the objective at p0
  cont                   from the device's pfit, inside the rounding bound; floored or
                         free exactly where the margin decides
  proc_spec, proc_ivar   from the device's cont, inside the rounding bounds; zeros exact
  sse                    from the device's proc_spec, proc_ivar

proc_spec, proc_ivar, sse, cont, pfit and status lie inside sentinel-filled margins
that must come back untouched.  What a family adds to that is in its test."""
import numpy as np
import pytest
import torch

import ccf_preprocess_truth as pt

pytestmark = pytest.mark.gpu

DEV = 'cuda'
GUARD = 64
SENT = -12345.678
SENT_I = 0x10000
E_ARG = -1
WORST = {}
WORST_D = {}
LD = pt.LD


def _lib_():
    from rvspecfit_amd import _lib
    _lib.require_gpu()
    return _lib, _lib.lib()


def _guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD, ), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def _intact(buf, fill, what):
    g = torch.full((GUARD, ), fill, dtype=buf.dtype, device=DEV)
    assert torch.equal(buf[:GUARD], g), 'write in front of ' + what
    assert torch.equal(buf[-GUARD:], g), 'write behind ' + what


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


_device_tables = {}


def _tables(L):
    if L['name'] not in _device_tables:
        T = pt.tables(L)
        d = dict(lam=_dev(L['lam']), xind=_dev(T['xind']), rw=_dev(T['rw']))
        for k, src in (('Eb', 'Eb'), ('El', 'El'), ('Cinv', 'CinvC'),
                       ('istart', 'istart'), ('bin_start', 'bin_start')):
            d[k] = _dev(T[src]) if L['continuum'] else None
        _device_tables[L['name']] = d
    return _device_tables[L['name']]


def call(lib, _lib, tabs, spec, espec, bad, npix, B, continuum, nnode, nfft, maxerr,
         want=('cont', 'pfit', 'status'), status0=0, grid=None, expect=0):
    """one rvs_ccf_preprocess (or _g with grid = (grid_id, npix_g, nnode_g)) into
    guarded buffers -> dict of numpy outputs (None for an output not asked for)"""
    bufs, out = {}, {}
    for k, n, dt, fill in (('proc_spec', B * nfft, torch.float64, SENT),
                           ('proc_ivar', B * nfft, torch.float64, SENT),
                           ('sse', B, torch.float64, SENT),
                           ('cont', B * npix, torch.float64, SENT),
                           ('pfit', B * nnode, torch.float64, SENT),
                           ('status', B, torch.int32, SENT_I)):
        bufs[k], out[k] = _guarded(max(n, 1), dt, fill)
    out['status'].fill_(status0)
    p = _lib.ptr
    args = [p(tabs['lam']), p(spec), p(espec), p(bad), npix, B, continuum,
            p(tabs['Eb']), p(tabs['El']), p(tabs['Cinv']), p(tabs['istart']), nnode,
            p(tabs['bin_start']), p(tabs['xind']), p(tabs['rw']), nfft, float(maxerr),
            p(out['proc_spec']), p(out['proc_ivar']), p(out['sse'])] + \
        [p(out[k]) if k in want else None for k in ('cont', 'pfit', 'status')]
    if grid is None:
        rc = lib.rvs_ccf_preprocess(*args, _lib.stream())
    else:
        rc = lib.rvs_ccf_preprocess_g(*args, *[p(g) for g in grid], _lib.stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    for k, fill in (('proc_spec', SENT), ('proc_ivar', SENT), ('sse', SENT),
                    ('cont', SENT), ('pfit', SENT), ('status', SENT_I)):
        _intact(bufs[k], fill, k)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if rc != 0:                      # refused before any launch: nothing written
        for k in ('proc_spec', 'proc_ivar', 'sse', 'cont', 'pfit'):
            assert np.all(res[k] == SENT), k
        assert np.all(res['status'] == status0)
        return res
    for k in ('cont', 'pfit'):
        if k not in want or (k == 'pfit' and not continuum):
            assert np.all(res[k] == SENT), k + ' written'
            res[k] = None
    if 'status' not in want:
        assert np.all(res['status'] == status0)
        res['status'] = None
    res['proc_spec'] = res['proc_spec'].reshape(B, nfft)
    res['proc_ivar'] = res['proc_ivar'].reshape(B, nfft)
    if res['cont'] is not None:
        res['cont'] = res['cont'].reshape(B, npix)
    if res['pfit'] is not None:
        res['pfit'] = res['pfit'].reshape(B, nnode)
    return res


def run(L, rows=None, **kw):
    """launch L, or its spectra `rows` alone"""
    _lib, lib = _lib_()
    rows = list(range(L['B'])) if rows is None else list(rows)
    bad = None if L['badmask'] is None else _dev(L['badmask'][rows])
    return call(lib, _lib, _tables(L), _dev(L['spec'][rows]), _dev(L['espec'][rows]),
                bad, len(L['lam']), len(rows), L['continuum'], len(L['nodes']),
                L['nfft'], L['maxerr'], **kw)


_results = {}


def result(L):
    """the full launch, once per session"""
    if L['name'] not in _results:
        _results[L['name']] = run(L)
    return _results[L['name']]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _same_result(a, b, rows_a=slice(None), rows_b=slice(None)):
    for k in a:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, k
        else:
            assert _same_bits(a[k][rows_a], b[k][rows_b]), k


def _hold(key, got, want, bound, what):
    r = pt.ratio(got, want, bound)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert r <= 1, what + (key, r)


def check_spectrum(L, i, out, row=None, bound=None):
    """spectrum i of launch L (row `row` of the outputs) against its own truth"""
    row = i if row is None else row
    t, what = pt.truth(L, i), (L['name'], i)
    npix = len(L['lam'])
    assert out['status'][row] == t['status'], what + (out['status'][row], )
    pfit = None
    if L['continuum']:
        pfit = out['pfit'][row]
        assert np.all(np.isfinite(pfit)), what
        T = pt.tables(L)
        s, e = t['cs'].astype(LD), t['ce'].astype(LD)
        f_fit = pt.objective(T['A'], s, e, pfit)[0]
        f_0 = pt.objective(T['A'], s, e, t['p0'])[0]
        # (the kernel's own sqrt(1 + z) - 1 carries 2 eps a pixel, which is all there
        # is to the cost of a masked pixel: that much it may accept upwards)
        assert f_fit <= f_0 * (1 + 1e-12) + 4 * npix * pt.EPS, \
            what + (float(f_fit), float(f_0))
        if L['fit'] == 'gtol':
            _hold('p0', pfit, t['p0'], pt.p0_bound(L, t['p0']), what)
        elif L['fit'] == 'newton':
            pstar, _, _ = pt.newton(L, i, pfit)
            d = float(np.abs(pfit - pstar).max())
            WORST_D[L['family']] = max(WORST_D.get(L['family'], 0.0), d)
            b = pt.bound_of(L['family']) if bound is None else bound
            print('ccf-preprocess d %-22s %d %.3g (bound %.3g)' % (L['name'], i, d, b))
            assert d <= b, what + (d, b)
    cont, cb, floored, free, floor = pt.cont_given_pfit(L, i, pfit)
    got = out['cont'][row]
    _hold('cont', got, cont, cb * cont, what)
    assert np.all(np.abs(got[floored] - floor) <= 2 * pt.EPS * floor), what
    assert np.all(got[free] > floor * (1 + pt.BRANCH_MARGIN / 2)), what
    r1, b1, r2, b2 = pt.proc_given_cont(L, i, got)
    _hold('proc_spec', out['proc_spec'][row], r1, b1, what)
    _hold('proc_ivar', out['proc_ivar'][row], r2, b2, what)
    sse, sb = pt.sse_given_proc(out['proc_spec'][row], out['proc_ivar'][row])
    _hold('sse', out['sse'][row], sse, sb, what)
    if L['grid'] == 'pixels':
        # the mask itself, pixel by pixel
        sp = L['spec'][i]
        with np.errstate(all='ignore'):
            c = np.where(t['mask'], 0.0, sp / got)
        assert _same_bits(out['proc_spec'][row][:npix - 1], c[:npix - 1]), what
        nz = sp[:npix - 1] != 0
        assert np.array_equal((out['proc_spec'][row][:npix - 1] == 0)[nz],
                              t['mask'][:npix - 1][nz]), what
        both = t['mask'][:-1] | t['mask'][1:]
        fin = np.isfinite(t['ce'][:-1]) & np.isfinite(t['ce'][1:])
        assert np.array_equal((out['proc_ivar'][row][:npix - 1] == 0)[fin], both[fin]), what
    elif L['grid'] == 'disjoint':
        assert not out['proc_spec'][row].any() and not out['proc_ivar'][row].any()
        assert out['sse'][row] == 0


def check_launch(L):
    out = result(L)
    for i in range(L['B']):
        check_spectrum(L, i, out)
    return out


def _report(family):
    print('ccf-preprocess device/bound %-7s %s | d %s' % (
        family, ' '.join('%s %.3g' % kv for kv in sorted(WORST.items())),
        ' '.join('%s %.3g' % kv for kv in sorted(WORST_D.items()))))


def test_pixel_counts_and_fft_grids():
    """npix 12 ... 1537 (below the block, 513 and 1025: the second load path of
    lm_eval), nfft 2, 64, 513, 8192, the FFT grid inside the arm, wider on both sides,
    disjoint (all zero, sse 0) and on the pixels themselves"""
    for L in pt.by_family('npix'):
        check_launch(L)
    _report('npix')


def test_largest_arm():
    """the largest npix the LDS rule of rvs_ccf_preprocess_g admits
    (ccf_preprocess_truth.max_npix: 24 npix + 16 ceil(npix / 16) bytes and the two
    static structures within 159 KB), and one pixel more refused"""
    _lib, lib = _lib_()
    L = pt.largest_arm()
    out = run(L)
    dt = float(np.abs(pt.trf(L, 0) - pt.newton(L, 0, pt.trf(L, 0))[0]).max())
    check_spectrum(L, 0, out, bound=max(pt.bound_of('npix'), dt))
    n = len(L['lam']) + 1
    tabs = dict(_tables(L))
    z = torch.zeros(3 * n, dtype=torch.float64, device=DEV)
    tabs['lam'] = z
    call(lib, _lib, tabs, z, z, None, n, 1, 1, len(L['nodes']), L['nfft'], 10.0,
         expect=E_ARG)
    _report('largest')


def test_binned_start_through_the_gtol_exit():
    """errors 1e12 x the flux: pfit = C C^-1 p0.  Bins of 0, 1, 2, 64, 65, 256 pixels
    (a wave's bisection), 257 and 600 (the block's selection), 256 and 257 mixed,
    pixels beyond the last edge, plateaus, quantised values, a bin median below the
    floor, negative and zero overall medians, flux scaled by 1e-30 and 1e30, every
    pixel count, 24 nodes on 12 pixels, the masks"""
    for L in pt.by_family('start'):
        check_launch(L)
    _report('start')


def test_node_counts_and_interval_sizes():
    """3, 4, 5, 23, 24 nodes; knot intervals of 0, 1, 63, 64, 65, 255, 256, 257, 600
    pixels (lm_normal's 4 x 64 trip and its tail)"""
    for L in pt.by_family('nodes'):
        check_launch(L)
    _report('nodes')


def test_bin_sizes_through_a_full_fit():
    for L in pt.by_family('bins'):
        check_launch(L)
    _report('bins')


def test_flux_scale_and_medv():
    """flux and errors scaled together by 1e-30 and 1e30; 1e-2 medv above the fitted
    continuum on half of the arm"""
    for f in ('scale', 'medv'):
        for L in pt.by_family(f):
            check_launch(L)
    a, b = result(pt.by_name('scale-fit'))['proc_spec']
    assert np.array_equal(a == 0, b == 0) and np.any(b != 0)
    assert np.abs(a[b != 0] / b[b != 0] - 1).max() < 1e-9   # no scale once normalised
    _report('scale')


def test_masks():
    """no mask, first / last pixel, alternating pixels, a run across pixel 511 / 512,
    espec exactly maxerr mederr (not masked) and an ulp above, +inf errors,
    non-positive flux on pixel 3, six and five of eleven; then the first and last 200,
    all but one, all but the ends, all (with and without +inf flux under the mask);
    badmask NULL.  The mask is read back pixel by pixel (check_spectrum)."""
    for L in pt.by_family('masks'):
        check_launch(L)
    assert pt.by_name('masks-null')['badmask'] is None
    _report('masks')


def test_reference_nodes():
    for L in pt.by_family('oracle'):
        check_launch(L)
    _report('oracle')


def test_without_continuum():
    """continuum = 0: badmask only, cont 1 or floored by medv, every table pointer of
    the fit NULL, pfit untouched; nnode 2 and 25 accepted"""
    for L in pt.by_family('nocont'):
        check_launch(L)
        for nnode in (2, 25):
            _lib, lib = _lib_()
            bad = None if L['badmask'] is None else _dev(L['badmask'])
            out = call(lib, _lib, _tables(L), _dev(L['spec']), _dev(L['espec']), bad,
                       len(L['lam']), L['B'], 0, nnode, L['nfft'], L['maxerr'])
            for k in ('proc_spec', 'proc_ivar', 'sse', 'cont', 'status'):
                assert _same_bits(out[k], result(L)[k]), k
    _report('nocont')


def test_launch_forms():
    """B = 1, 2 and 600 (more blocks than are resident): every row equals the same
    spectrum launched alone, bit for bit, and two launches are bit-identical"""
    for L in pt.launches():
        if len(L['lam']) > 1600 or L['B'] > 5:
            continue
        out = result(L)
        _same_result(run(L), out)
        for i in range(L['B']):
            _same_result(run(L, rows=[i]), out, slice(None), slice(i, i + 1))
    L = pt.by_name('masks-mild')
    rows = [i % L['B'] for i in range(600)]
    big = run(L, rows=rows)
    _same_result(big, run(L, rows=rows))
    out = result(L)
    for k in big:
        assert _same_bits(big[k], out[k][rows]), k
    two = run(L, rows=[4, 1])
    for k in two:
        assert _same_bits(two[k], out[k][[4, 1]]), k


def test_grid_sets():
    """rvs_ccf_preprocess_g: three grids with different npix_g, nnode_g and bands, nine
    spectra with a scrambled grid_id; each equals the same spectrum on its own grid
    through rvs_ccf_preprocess bit for bit; the tails of cont rows past npix_g and of
    pfit rows past nnode_g still hold the sentinel"""
    _lib, lib = _lib_()
    Ls = pt.by_family('grids')
    for L in Ls:
        check_launch(L)
    G, nfft = len(Ls), Ls[0]['nfft']
    npg = np.array([len(L['lam']) for L in Ls], np.int32)
    nng = np.array([len(L['nodes']) for L in Ls], np.int32)
    NP, NN = int(npg.max()), int(nng.max())
    lam, xind, rw = np.zeros((G, NP)), np.zeros((G, nfft), np.int32), np.zeros((G, nfft))
    Eb, El = np.zeros((G, 3 * NP)), np.zeros((G, NP), np.int32)
    Cinv = np.zeros((G, 2 * NN * NN))
    ist, bst = np.zeros((G, NN), np.int32), np.zeros((G, NN + 1), np.int32)
    for g, L in enumerate(Ls):
        T, n, m = pt.tables(L), npg[g], nng[g]
        lam[g, :n], xind[g], rw[g] = L['lam'], T['xind'], T['rw']
        Eb[g, :3 * n], El[g, :n] = T['Eb'].ravel(), T['El']
        Cinv[g, :2 * m * m] = T['CinvC']
        ist[g, :m - 1], bst[g, :m + 1] = T['istart'], T['bin_start']
    gid = np.array([2, 0, 1, 1, 2, 0, 0, 1, 2], np.int32)
    which = np.array([0, 0, 0, 1, 1, 1, 2, 2, 2])          # spectrum inside its grid
    B = len(gid)
    spec, espec = np.full((B, NP), np.nan), np.full((B, NP), np.nan)
    for b in range(B):
        L = Ls[gid[b]]
        spec[b, :npg[gid[b]]], espec[b, :npg[gid[b]]] = L['spec'][which[b]], \
            L['espec'][which[b]]
    tabs = dict(lam=_dev(lam), xind=_dev(xind), rw=_dev(rw), Eb=_dev(Eb), El=_dev(El),
                Cinv=_dev(Cinv), istart=_dev(ist), bin_start=_dev(bst))
    grid = (_dev(gid), _dev(npg), _dev(nng))
    out = call(lib, _lib, tabs, _dev(spec), _dev(espec), None, NP, B, 1, NN, nfft,
               10.0, grid=grid)
    for b in range(B):
        own, i, n, m = result(Ls[gid[b]]), which[b], npg[gid[b]], nng[gid[b]]
        for k in ('proc_spec', 'proc_ivar', 'sse', 'status'):
            assert _same_bits(out[k][b], own[k][i]), (k, b)
        assert _same_bits(out['cont'][b, :n], own['cont'][i])
        assert _same_bits(out['pfit'][b, :m], own['pfit'][i])
        assert np.all(out['cont'][b, n:] == SENT) and np.all(out['pfit'][b, m:] == SENT)
    # grid_id without npix_g (and, with the continuum fit, without nnode_g)
    for bad_grid in ((grid[0], None, grid[2]), (grid[0], grid[1], None)):
        call(lib, _lib, tabs, _dev(spec), _dev(espec), None, NP, B, 1, NN, nfft, 10.0,
             grid=bad_grid, expect=E_ARG)
    _report('grids')


def test_arguments():
    """RVS_E_ARG before any launch, outputs untouched: npix = 11, nnode = 2 or 25 with
    the continuum fit, B = 0, nfft = 1 (the largest npix plus one: test_largest_arm;
    grid_id without npix_g: test_grid_sets).  cont, pfit and status each NULL: the
    other outputs keep their bits.  status is OR-ed into."""
    _lib, lib = _lib_()
    L = pt.by_name('masks-hard')
    tabs, n, m = _tables(L), len(L['lam']), len(L['nodes'])
    spec, espec, bad = _dev(L['spec']), _dev(L['espec']), _dev(L['badmask'])
    for npix, B, nnode, nfft in ((11, L['B'], m, L['nfft']), (n, L['B'], 2, L['nfft']),
                                 (n, L['B'], 25, L['nfft']), (n, 0, m, L['nfft']),
                                 (n, -1, m, L['nfft']), (n, L['B'], m, 1)):
        call(lib, _lib, tabs, spec, espec, bad, npix, B, 1, nnode, nfft, 10.0,
             status0=1, expect=E_ARG)
    full = result(L)
    for drop in ('cont', 'pfit', 'status'):
        want = tuple(k for k in ('cont', 'pfit', 'status') if k != drop)
        out = run(L, want=want)
        assert out[drop] is None
        for k in out:
            if k != drop:
                assert _same_bits(out[k], full[k]), (drop, k)
    out = run(L, status0=0x1)
    assert np.array_equal(out['status'], full['status'] | 0x1)
    assert set(out['status'].tolist()) == {0x1, 0x1 | pt.ST_ALLMASKED}


def _run_model(L, nnode=None, expect=0):
    _lib, lib = _lib_()
    T = pt.tables(L)
    ntp, M, m, npts = len(L['lam']), L['B'], len(L['nodes']), L['npoints']
    bufs, out = {}, {}
    for k, n, dt, fill in (('model', M * npts, torch.float64, SENT),
                           ('cont', M * ntp, torch.float64, SENT),
                           ('pfit', M * m, torch.float64, SENT),
                           ('status', M, torch.int32, SENT_I)):
        bufs[k], out[k] = _guarded(n, dt, fill)
    out['status'].zero_()
    p = _lib.ptr
    keep = [_dev(a) for a in (L['spec'], L['espec'] if L['erows'] else None, T['Eb'],
                              T['El'], T['CinvC'], T['istart'], T['bin_start'],
                              L['lnlam'], L['logl'], L['ihi'])]
    rows, erows, Eb, El, Cinv, ist, bst, lnlam, logl, ihi = keep
    rc = lib.rvs_ccf_models_build(
        p(rows), None, p(erows), ntp, M, 1, p(Eb), p(El), p(Cinv), p(ist),
        m if nnode is None else nnode, p(bst), p(lnlam), p(logl), p(ihi), npts, None,
        p(out['model']), None, None, p(out['cont']), p(out['pfit']), p(out['status']),
        _lib.stream())
    assert rc == expect, rc
    torch.cuda.synchronize()
    for k, fill in (('model', SENT), ('cont', SENT), ('pfit', SENT), ('status', SENT_I)):
        _intact(bufs[k], fill, k)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if rc != 0:
        assert all(np.all(res[k] == SENT) for k in ('model', 'cont', 'pfit'))
        return res
    return dict(model=res['model'].reshape(M, npts), cont=res['cont'].reshape(M, ntp),
                pfit=res['pfit'].reshape(M, m), status=res['status'])


def test_model_rows():
    """rvs_ccf_models_build on float64 rows (fft = fft2 = NULL): ntp 12, 513, 1025 with
    3, 25, 48 nodes (above 24 only ccf_model_kernel's LM state exists), with and
    without erows, a row with a non-positive median (RVS_ST_NONPOS_MEDIAN), ihi outside
    the row on either side (1); 49 nodes refused.  d against the same minimiser under
    the model's error rule, cont (unfloored) from the device's pfit, the model values
    from the device's cont."""
    for L in pt.model_launches():
        out = _run_model(L)
        ntp = len(L['lam'])
        for i in range(L['B']):
            t, what = pt.truth(L, i), (L['name'], i)
            assert out['status'][i] == t['status'], what
            pfit = out['pfit'][i]
            if i not in L['nofit']:
                pstar, _, _ = pt.newton(L, i, pfit)
                d = float(np.abs(pfit - pstar).max())
                WORST_D['models'] = max(WORST_D.get('models', 0.0), d)
                assert d <= pt.bound_of('models'), what + (d, )
            raw, b = pt.raw_cont(L, pfit)
            _hold('model cont', out['cont'][i], raw, b * raw, what)
            v, bv = pt.model_given_cont(L, i, out['cont'][i])
            _hold('model', out['model'][i], v, bv, what)
            outside = (L['ihi'] < 1) | (L['ihi'] >= ntp)
            assert outside.sum() > 4 and np.all(out['model'][i][outside] == 1), what
        two = _run_model(L)
        for k in out:
            assert _same_bits(out[k], two[k]), (L['name'], k)
    _run_model(pt.by_name('model-1025-48'), nnode=49, expect=E_ARG)
    _report('models')
