"""Pair columns of the velocity-grid kernels (csrc/chisq.hip, cg_pair_cols): on one
wavelength grid and npoly <= 13 the last K columns of the packed normal matrix take
their products P_i P_j from the pixel's 128-byte row instead of multiplying P_j w
first.  Held here:

  1. chi^2 against the extended-precision truth (tests/chisq_truth.py) on the
     resampled template, at the figure tests/test_chisq_accuracy.py holds every
     float64 evaluation to: 1e-9 of max(|chi^2|, npix);
  2. a velocity gives the same bits and the same status word wherever it is
     computed: full wave, ragged wave, packed wave, node table;
  3. a grid set (G = 2, here two identical grids) keeps the rows of npoly doubles
     and the K = 0 arithmetic: where one grid has no pair columns either its
     values are those of the one-grid call bit for bit; where it has, they are the
     truth's to the same 1e-9, do not depend on which of the two grids a spectrum
     sits on, and are NOT the one-grid bits;
  4. the library-owned row buffer: calls of different npix and npoly in a row on
     one stream give what each gives alone.

npoly 1, 2, 3, 5, 6, 10, 11, 13, 14, 16 are K = 5, 4, 4, 4, 4, 3, 2, 2, 0, 0 by the
rule (both sides of every change of K, and the two-pass kernels, which are
untouched); the library applies the rule at the npoly where it measured faster
and says which through rvs_chisq_grid_pair_cols (0 = the plain rows).  5, 64,
80 and 129 velocities are packed lanes only, one full wave, a full wave + 16
packed, two full waves + one packed."""
import contextlib

import numpy as np
import pytest
import torch

from chisq_truth import chisq0_longdouble
from conftest import GOLD_CONFIG, gold_lib_dict
from oracle import rvs_oracle as orc

pytestmark = pytest.mark.gpu

NPOLY = [1, 2, 3, 5, 6, 10, 11, 13, 14, 16]
NV = [5, 64, 80, 129]
VELS = np.linspace(-290.0, 300.0, 129) + 0.37
PARAMS = [(5100., 2.3, -0.9, 0.15), (5600., 3.9, -0.4, 0.05)]
TOL = 1e-9          # tests/test_chisq_accuracy.py, relative to max(|chi^2|, npix)
S = 4               # spectra; jobs = S x the two templates = 8


@contextlib.contextmanager
def _knobs(tab, pack):
    from rvspecfit_amd import engine
    keep = engine.CG_TAB_MIN_JOBS, engine.CG_PACK_MIN_JOBS
    engine.CG_TAB_MIN_JOBS, engine.CG_PACK_MIN_JOBS = tab, pack
    try:
        yield
    finally:
        engine.CG_TAB_MIN_JOBS, engine.CG_PACK_MIN_JOBS = keep


class _Arm:
    """S spectra of `npix` pixels on one grid (and the same spectra as a grid set
    of two identical grids), two templates, the oracle's spline of each template
    as the device built it"""

    def __init__(self, npix, linear=False, illcond=False):
        from rvspecfit_amd import _lib, engine, spec_inter
        from rvspecfit_amd.library import TemplateLibrary
        _lib.require_gpu()
        self.dev = torch.device('cuda')
        d = gold_lib_dict('gold_b')
        scheme = 'pair-columns://log'
        if linear:
            lam_log = np.asarray(d['lam'], dtype=np.float64)
            d['lam'] = np.linspace(lam_log[0], lam_log[-1], len(lam_log))
            d['log_step'] = np.array(False)
            scheme = 'pair-columns://lin'
        spec_inter.register_library(TemplateLibrary('gold_b', d), scheme)
        cfg = dict(GOLD_CONFIG, template_lib=scheme)
        self.npix = npix
        self.lam = 4400.0 + 0.8 * np.arange(npix)
        self.libs = spec_inter.get_libs(['gold_b'], cfg)
        lib = self.libs['gold_b']
        assert bool(lib.log_step) == (not linear)
        flat = torch.as_tensor(np.array(PARAMS)).to(self.dev).contiguous()
        coef, outside, templ = engine.build_templates(lib, flat, None,
                                                      return_templ=True)
        self.coefs, self.outs = [coef], [outside]
        assert float(outside.abs().max().item()) == 0.0
        knots = lib.knots.cpu().numpy()
        self.spl = [orc.Spline(knots, t, log_step=not linear)
                    for t in templ.cpu().numpy()]
        rng = np.random.RandomState(7 + npix)
        x = np.linspace(-1, 1, npix) if npix > 1 else np.zeros(1)
        self.spec = np.empty((S, npix))
        self.espec = np.empty((S, npix))
        for s in range(S):
            m = orc.eval_rv(self.spl[s % 2], 30.0 + 11 * s, self.lam) * \
                (1 + 0.2 * x + 0.1 * s * x * x)
            self.espec[s] = np.abs(m) / 100.0
            self.spec[s] = m + self.espec[s] * rng.standard_normal(npix)
        if illcond:   # spectrum 1: half its pixels at 1e6-fold errors
            self.espec[1, npix // 2:] *= 1e6
        self.batch = engine.SpecBatch([engine.ArmData(
            'gold_b', self.lam, self.spec, self.espec, device=self.dev)])
        self.batch2 = {
            gid: engine.SpecBatch([engine.ArmData(
                'gold_b', [self.lam, self.lam.copy()], self.spec, self.espec,
                device=self.dev, grid_id=np.array(gid, dtype=np.int32))])
            for gid in ((0, 1, 0, 1), (1, 0, 1, 0))}
        self._truth = {}

    def jobs(self, J=2 * S):
        js = torch.as_tensor([j % S for j in range(J)], dtype=torch.int32)
        jt = torch.as_tensor([(j // S) % 2 for j in range(J)], dtype=torch.int32)
        return js.to(self.dev), jt.to(self.dev)

    def grid(self, vels, npoly, tab=-1, pack=1, batch=None, J=2 * S,
             defer_redo=False, knobs=True):
        """chi^2 [J, Nv], status [J]; tab: engine.CG_TAB_MIN_JOBS, pack:
        engine.CG_PACK_MIN_JOBS (1 = the left-over velocities packed, -1 = a
        ragged wave); knobs = False: as the engine's globals stand (they are set
        from one thread at a time)"""
        from rvspecfit_amd import engine
        js, jt = self.jobs(J)
        with (_knobs(tab, pack) if knobs else contextlib.nullcontext()):
            r = engine.chisq_grid(
                batch or self.batch, self.libs, self.coefs, self.outs,
                torch.as_tensor(np.ascontiguousarray(vels)).to(self.dev),
                npoly=npoly, job_spec=js, job_templ=jt, defer_redo=defer_redo)
            took = engine.cg_tab_took()
        if defer_redo:
            return r
        if tab > 0 and len(vels) >= 64:
            assert took == 1
        else:
            assert took == 0
        return r[0].cpu().numpy(), r[1].cpu().numpy()

    def truth(self, npoly, j, iv):
        key = (npoly, j, iv)
        if key not in self._truth:
            s, t = j % S, (j // S) % 2
            polys = orc.get_poly_basis(self.lam, npoly)
            self._truth[key] = float(chisq0_longdouble(
                self.spec[s], orc.eval_rv(self.spl[t], VELS[iv], self.lam),
                polys, self.espec[s]))
        return self._truth[key]

    def check_truth(self, chisq, npoly, ivs, jobs=range(2 * S), what=''):
        worst = 0.0
        for j in jobs:
            for iv in ivs:
                ld = self.truth(npoly, j, iv)
                worst = max(worst, abs(chisq[j, iv] - ld) /
                            max(abs(ld), self.npix))
        print('%s npix %d npoly %d: max |chi^2 - truth| / max(|chi^2|, npix) '
              '= %.3g' % (what, self.npix, npoly, worst))
        assert worst < TOL, (what, self.npix, npoly, worst)


_arms = {}


def _arm(npix, **kw):
    key = (npix, ) + tuple(sorted(kw.items()))
    if key not in _arms:
        _arms[key] = _Arm(npix, **kw)
    return _arms[key]


def _placements(arm, npoly, truth_iv):
    """every velocity of VELS computed as a lane of a ragged launch of 129 (the
    value held to the truth), then in every other place: prefixes of 5, 64, 80
    and 129 velocities with the left-over ones packed, the same reversed (what
    was in a full wave is now packed and the other way round), and the full
    waves on the node table"""
    ref, sref = arm.grid(VELS, npoly, pack=-1)
    arm.check_truth(ref, npoly, truth_iv, what='one grid')
    for nv in NV:
        got, st = arm.grid(VELS[:nv], npoly, pack=1)
        np.testing.assert_array_equal(got, ref[:, :nv])
        rev, srev = arm.grid(VELS[:nv][::-1], npoly, pack=1)
        np.testing.assert_array_equal(rev[:, ::-1], ref[:, :nv])
        np.testing.assert_array_equal(st, srev)
        if nv == len(VELS):
            np.testing.assert_array_equal(st, sref)
        if nv >= 64:
            tab, stab = arm.grid(VELS[:nv], npoly, tab=1, pack=1)
            np.testing.assert_array_equal(tab, ref[:, :nv])
            np.testing.assert_array_equal(stab, st)
    return ref, sref


@pytest.mark.parametrize('npoly', NPOLY)
@pytest.mark.parametrize('npix', [37, 130])
def test_truth_and_placements(npix, npoly):
    """assertions 1 and 2, logarithmic knots; 37 pixels: one trip behind the
    two-pixel and the four-pixel unrolled loops, 130: none and two"""
    arm = _arm(npix)
    ref, st = _placements(arm, npoly, (0, 4, 63, 64, 79, 128))
    assert not st.any(), st


@pytest.mark.parametrize('npix,npoly', [(3, 1), (3, 2), (3, 3)])
def test_shortest_arms(npix, npoly):
    """arms shorter than the rows requested ahead (npix = npoly: the fit is exact,
    chi^2 is the log-determinant terms alone)"""
    arm = _arm(npix)
    _placements(arm, npoly, (0, 64, 128))


def test_one_pixel():
    """npix = 1, npoly = 1: every row request of the loop is clamped to row 0.
    The engine's basis builder takes arms from two pixels up, so this is the raw
    call, on the raw basis (one number), full, ragged and packed waves"""
    from rvspecfit_amd import _lib
    arm = _arm(1)
    L = _lib.lib()
    a, lib = arm.batch.arms[0], arm.libs['gold_b']
    polys = orc.get_poly_basis(arm.lam, 1)
    polysT = torch.zeros((2, 1), dtype=torch.float64, device=arm.dev)
    polysT[0, 0] = float(polys[0, 0])
    work = a.work(lib)
    js, jt = arm.jobs()
    pen = torch.zeros(2 * S, dtype=torch.float64, device=arm.dev)

    def grid(vels, pack):
        v = torch.as_tensor(np.ascontiguousarray(vels)).to(arm.dev)
        out = torch.empty((2 * S, len(vels)), dtype=torch.float64, device=arm.dev)
        st = torch.zeros(2 * S, dtype=torch.int32, device=arm.dev)
        rc = L.rvs_chisq_grid_g(
            _lib.ptr(a.lam), _lib.ptr(polysT), _lib.ptr(work), 1, 1, a.S, None, 1,
            a.basis_stride(1), _lib.ptr(lib.knots), _lib.ptr(arm.coefs[0]),
            lib.ntp, 2, int(lib.log_step), _lib.ptr(js), _lib.ptr(jt), 2 * S,
            _lib.ptr(v), 0, len(vels), _lib.ptr(pen), float(arm.batch.badchi), 0.0,
            pack, None, _lib.ptr(out), _lib.ptr(st), _lib.stream())
        _lib.check(rc, 'rvs_chisq_grid_g')
        return out.cpu().numpy(), st.cpu().numpy()
    ref, sref = grid(VELS, -1)
    assert not sref.any()
    arm.check_truth(ref, 1, (0, 64, 128), what='raw call')
    for nv in NV:
        got, st = grid(VELS[:nv], 1)
        np.testing.assert_array_equal(got, ref[:, :nv])
        rev, srev = grid(VELS[:nv][::-1], 1)
        np.testing.assert_array_equal(rev[:, ::-1], ref[:, :nv])
        assert not st.any() and not srev.any()


@pytest.mark.parametrize('npoly', [3, 10, 13, 14])
def test_linear_knots(npoly):
    """the other instance of the resampling (and of the pixel loop)"""
    arm = _arm(37, linear=True)
    _placements(arm, npoly, (0, 64, 128))


@pytest.mark.parametrize('npoly', NPOLY)
def test_grid_set_keeps_plain_rows(npoly):
    """assertion 3: two identical grids -- the call is a grid set, the kernels
    read rows of npoly doubles at polys_stride and multiply P_j w first"""
    arm = _arm(37)
    ref, sref = arm.grid(VELS, npoly, pack=-1)
    a, sa = arm.grid(VELS, npoly, batch=arm.batch2[(0, 1, 0, 1)])
    b, sb = arm.grid(VELS, npoly, batch=arm.batch2[(1, 0, 1, 0)])
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(sa, sb)
    np.testing.assert_array_equal(sa, sref)
    arm.check_truth(a, npoly, (0, 4, 63, 64, 79, 128), what='grid set')
    from rvspecfit_amd import _lib
    if _lib.lib().rvs_chisq_grid_pair_cols(npoly) == 0:
        assert npoly != 10    # (the contract step's npoly has them)
        # K = 0 on one grid as well: the same arithmetic
        np.testing.assert_array_equal(a, ref)
    else:
        # one rounding in front of each FMA either way: the two forms differ by
        # rounding errors of the sums, far inside the tolerance against the truth
        d = np.max(np.abs(a - ref) / np.maximum(np.abs(ref), arm.npix))
        print('npoly %d: grid set against one grid %.3g, %d of %d values differ'
              % (npoly, d, int((a != ref).sum()), a.size))
        assert d < TOL
        # ... and they DO differ: a grid set that ran the pair-column arithmetic
        # would give the one-grid bits in all 8 x 129 values
        assert (a != ref).any()


def test_node_table_two_nodes_sixteen_jobs():
    """one table call at the gate's own threshold: 2 node templates x 16 jobs
    each (engine.CG_TAB_MIN_JOBS = 16 jobs per node), 80 velocities"""
    arm = _arm(130)
    ref, sref = arm.grid(VELS[:80], 10, pack=-1, J=32)
    tab, stab = arm.grid(VELS[:80], 10, tab=16, pack=1, J=32)
    np.testing.assert_array_equal(tab, ref)
    np.testing.assert_array_equal(stab, sref)
    # (jobs j and j + 8 are the same spectrum and template)
    np.testing.assert_array_equal(tab[:8], tab[8:16])
    arm.check_truth(tab, 10, (0, 63, 64, 79), what='table 2 x 16')


def test_row_buffer_between_calls():
    """assertion 4: the rows are rebuilt at the head of every call, in a buffer
    that is kept between them -- a long arm, a short one, another npoly, back"""
    big, small = _arm(130), _arm(37)
    alone = {}
    for arm, npoly in ((big, 10), (small, 10), (small, 6), (big, 13), (big, 2)):
        torch.cuda.synchronize()
        alone[(arm.npix, npoly)] = arm.grid(VELS[:80], npoly, tab=1)
        torch.cuda.synchronize()
    order = [(big, 10), (small, 6), (big, 2), (small, 10), (big, 13), (small, 10),
             (big, 10)]
    got = [arm.grid(VELS[:80], npoly, tab=1, defer_redo=True)
           for arm, npoly in order]      # queued back to back, no look in between
    for (arm, npoly), (chisq, st, finish) in zip(order, got):
        assert finish() == 0
        np.testing.assert_array_equal(chisq.cpu().numpy(),
                                      alone[(arm.npix, npoly)][0])
        np.testing.assert_array_equal(st.cpu().numpy(),
                                      alone[(arm.npix, npoly)][1])


def test_two_host_threads_on_one_stream():
    """two host threads that share ONE stream (desi_fit.proc_many's fit threads on
    the default stream), arms of different length, different npoly: a call's row
    kernel and grid kernels are queued as a unit, so each thread gets what it
    gets alone -- not the rows the other thread built in between"""
    import threading
    from rvspecfit_amd import _lib
    on = [p for p in range(1, 17) if _lib.lib().rvs_chisq_grid_pair_cols(p) > 0]
    assert 10 in on and max(on) <= 13
    # (both calls build rows in the stream's buffer; two npoly where two have them)
    work = [(_arm(130), on[-1]), (_arm(37), on[0])]
    alone = [arm.grid(VELS[:80], npoly, tab=-1) for arm, npoly in work]
    stream = torch.cuda.Stream()
    bad, errs = [0, 0], []
    start = threading.Barrier(2)

    def run(k):
        arm, npoly = work[k]
        try:
            with torch.cuda.stream(stream):
                start.wait()
                got = [arm.grid(VELS[:80], npoly, defer_redo=True, knobs=False)
                       for _ in range(150)]
                stream.synchronize()
            for chisq, st, _ in got:
                bad[k] += int(not (np.array_equal(chisq.cpu().numpy(), alone[k][0])
                                   and np.array_equal(st.cpu().numpy(),
                                                      alone[k][1])))
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=run, args=(k, )) for k in range(2)]
    with _knobs(-1, 1):     # (set once, around the threads)
        for t in th:
            t.start()
        for t in th:
            t.join()
    assert not errs, errs
    assert bad == [0, 0], bad


@pytest.mark.parametrize('npoly', [10, 13])
def test_illcond_still_flagged_and_redone(npoly):
    """a spectrum with half its pixels at 1e6-fold errors: the kernels flag its
    jobs (the same jobs wherever they run) and the engine re-evaluates them"""
    from rvspecfit_amd import _lib
    arm = _arm(130, illcond=True)
    out, status, finish = arm.grid(VELS[:80], npoly, pack=1, defer_redo=True)
    raw, st0 = out.cpu().numpy(), status.cpu().numpy()   # (copies)
    hit = np.array([j % S == 1 for j in range(2 * S)])
    assert np.all(st0[hit] & _lib.ST_ILLCOND) and not np.any(st0[~hit])
    assert finish() == int(hit.sum())           # the redo path, in place
    chisq, st = out.cpu().numpy(), status.cpu().numpy()
    assert np.all(st[hit] & _lib.ST_ILLCOND) and not np.any(st[~hit])
    np.testing.assert_array_equal(chisq[~hit], raw[~hit])
    arm.check_truth(chisq, npoly, (0, 63, 64, 79), what='1e6-fold errors')
    # the flags of the table and of the ragged wave are the same
    for kw in (dict(tab=1, pack=1), dict(pack=-1)):
        r2, s2, _ = arm.grid(VELS[:80], npoly, defer_redo=True, **kw)
        np.testing.assert_array_equal(s2.cpu().numpy(), st0)
        np.testing.assert_array_equal(r2.cpu().numpy(), raw)
