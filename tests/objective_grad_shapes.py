"""The cases of tests/test_objective_grad_shapes_cpu.py and ..._gpu.py: the shapes at
which rvs_objective_grad (csrc/objective_grad.hip) takes another path --
chunk geometry of the Thomas sweeps, the production sizes and the LDS limit, the two
packings of the third buffer, every npoly, grids of 1-3 dimensions, linear knots, arms
of very different length in one launch.  No tests here.

Libraries, all from the committed fixtures lib_gold_b.npz and lib_sdss1.npz:
  cut(ntp, off)    columns [off, off + ntp) of gold_b (off: the window of largest flux
                   contrast that fits, 535 for the short ones)
  fine(ntp)        the gold_b rows resampled (np.interp) onto a log-uniform grid of ntp
                   knots over the same range, float32
  lowdim(name, nd) the first nd dimensions of the grid, the others fixed at node 1
  linear(name)     the same rows on a LINEAR wavelength grid (log_step False)
  sdss1()          lib_sdss1.npz: 5971 knots on a 3^4 grid

Spectra: the library's own template at parameters 2 % off the case's first query,
resampled at the placing velocity, times a linear continuum, plus seeded Gaussian noise
(S/N 10 and 20); pixels on a linspace from inside the first knot interval to inside the
last one at that velocity, so that the status is 0 and both end intervals are used.
Errors are finite and constant."""
import os

import numpy as np

from conftest import GOLD, GOLD_CONFIG, gold_lib_dict
from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import objective_adjoint_restated as adj
import vsini_grad_truth as vtruth

ROOT = 'golden-grad-shapes://'
VEL = 12.3
# strictly inside a cell of gold_b's 4^4 grid AND of sdss1's 3^4 grid, >= 1 % of the
# cell width from every face (cell_margin)
Q0 = (6000.0, 2.5, -0.4, 0.1)
Q2 = (6900.0, 1.5, -0.2, 0.05)
QLAST = (7200.0, 3.5, -0.3, 0.3)      # gold_b: the last cell of every axis
BANDED_ABOVE = 2000                   # knots: truth.banded_spline

_dicts = {}
_olibs = {}


def _put(name, make):
    if name not in _dicts:
        _dicts[name] = make()
    return name


def _gold_b():
    return {k: v for k, v in gold_lib_dict('gold_b').items() if not k.startswith('ccf')}


def cut(ntp, off=None):
    off = min(535, 977 - ntp) if off is None else off

    def make():
        d = _gold_b()
        d.update(lam=np.asarray(d['lam'])[off:off + ntp],
                 dats=np.ascontiguousarray(np.asarray(d['dats'])[:, off:off + ntp]))
        return d
    return _put('cut%d_%d' % (ntp, off), make)


def fine(ntp):
    def make():
        d = _gold_b()
        lam0 = np.asarray(d['lam'], dtype=np.float64)
        lam = np.exp(np.linspace(np.log(lam0[0]), np.log(lam0[-1]), ntp))
        rows = np.asarray(d['dats'], dtype=np.float64)
        d.update(lam=lam, dats=np.stack([np.interp(lam, lam0, r) for r in rows])
                 .astype(np.float32))
        return d
    return _put('fine%d' % ntp, make)


def lowdim(name, ndim):
    def make():
        d = _dicts[name]
        idg = np.asarray(d['idgrid'])
        sub = idg[(Ellipsis, ) + (1, ) * (4 - ndim)]      # fix the last dimensions
        rows = sub.ravel()
        keep = rows[rows >= 0]
        new = np.full(rows.shape, -1, dtype=np.int64)
        new[rows >= 0] = np.arange(len(keep))
        dd = {k: v for k, v in d.items() if not k.startswith('uvec')}
        dd.update(dats=np.asarray(d['dats'])[keep], vec=np.asarray(d['vec'])[:ndim, keep],
                  idgrid=new.reshape(sub.shape),
                  parnames=np.asarray(d['parnames'])[:ndim])
        for i in range(ndim):
            dd['uvec%d' % i] = d['uvec%d' % i]
        return dd
    return _put('%s_nd%d' % (name, ndim), make)


def linear(name):
    def make():
        d = dict(_dicts[name])
        lam_log = np.asarray(d['lam'], dtype=np.float64)
        d['lam'] = np.linspace(lam_log[0], lam_log[-1], len(lam_log))
        d['log_step'] = np.array(False)
        return d
    return _put(name + '_lin', make)


def sdss1():
    def make():
        d = dict(np.load(os.path.join(GOLD, 'lib_sdss1.npz')))
        return {k: v for k, v in d.items() if not k.startswith('ccf')}
    return _put('sdss1', make)


def lib_dict(name):
    return _dicts[name]


def olib(name):
    if name not in _olibs:
        _olibs[name] = orc.Library(_dicts[name])
    return _olibs[name]


def cell_margin(lib, par):
    """the query's smallest distance to a face of its cell, in cell widths; -1 where the
    template is not the polylinear one (outside the grid, a missing vertex)"""
    if float(lib.outside_flag(np.asarray(par, dtype=np.float64))) != 0:
        return -1.0
    mp = lib.map_params(par)
    pos = lib.cell(mp)
    x = np.array([(mp[d] - lib.uvecs[d][pos[d]]) /
                  (lib.uvecs[d][pos[d] + 1] - lib.uvecs[d][pos[d]])
                  for d in range(lib.ndim)])
    return float(min(x.min(), (1 - x).min()))


def doppler(vel):
    b = vel / truth.C_KMS
    return np.sqrt((1 - b) / (1 + b))


# Seeds that replace a case's default one: with the default the numpy restatement of
# the adjoint method was further than 6e-13 from the autograd truth on some job (a
# component near a zero of its own: short templates give gradients of 1e-2 whose feh and
# alpha components are what log det A leaves over) -- the input was replaced, not the
# cap (tests/test_objective_grad_shapes_cpu.py).  With these every case is within 8e-13.
SEEDS = {'chunk-cut32': 29132, 'chunk-cut33': 7933, 'chunk-cut41': 9241,
         'chunk-cut873': 1073, 'prod-sdss1': 113, 'pack-cut64-32': 1421,
         'pack-cut65-32': 1622, 'pack-cut33-16': 223, 'pack-cut32-kmax13': 124,
         'p4-cut263': 134, 'p7-cut263': 137, 'p5-cut32-npix5': 245,
         'p1-cut32-npix2': 1541}


class Case:
    """one launch: arms [(library name, npix)], nspec spectra, jobs [(spectrum, vel,
    parameters, vsini in km/s or None)].  R (template pixels of the FIRST arm) -> vsini;
    in_cell: every job is held to the autograd truth and is part of the conditioning
    cap"""

    def __init__(self, name, group, arms, npoly, Rs=(None, ), vsini_grad=False,
                 queries=(Q0, Q2), nspec=2, seed=1, in_cell=True, jobs=None, rbf=True):
        self.name, self.group, self.arms, self.npoly = name, group, list(arms), npoly
        self.rbf = rbf          # rbf_continuum; False: the Chebyshev basis
        self.vsini_grad, self.nspec, self.in_cell = vsini_grad, nspec, in_cell
        self.seed = SEEDS.get(name, seed)
        self.snr = (10.0, 20.0, 15.0)[:nspec]
        lib0 = olib(self.arms[0][0])
        nd = lib0.ndim
        self.ndim = nd
        self.base = tuple(queries[0][:nd])
        self.R = Rs
        if jobs is None:
            jobs = []
            for R in Rs:
                for s in range(nspec):
                    jobs.append((s, VEL, tuple(queries[s % len(queries)][:nd]),
                                 self.vsini(R)))
        self.jobs = jobs

    def vsini(self, R):
        return None if R is None else vtruth.vsini_for(olib(self.arms[0][0]), R)

    def __repr__(self):
        return self.name


_spec_cache = {}


def spectra(case):
    """[spectrum][arm] -> (name, lam, spec, espec), seeded by the case"""
    if case.name in _spec_cache:
        return _spec_cache[case.name]
    rng = np.random.default_rng(case.seed)
    f = doppler(VEL)
    out = [[] for _ in range(case.nspec)]
    for name, npix in case.arms:
        lib = olib(name)
        kn = lib.lam
        lam = np.linspace((kn[0] + 0.3 * (kn[1] - kn[0])) / f,
                          (kn[-1] - 0.4 * (kn[-1] - kn[-2])) / f, npix)
        assert kn[0] < lam[0] * f < kn[1] and kn[-2] < lam[-1] * f < kn[-1]
        t = lib.eval(np.array([1.02 * q for q in case.base]))
        m = np.interp(lam * f, kn, t)
        x = np.linspace(-1.0, 1.0, npix)
        for s in range(case.nspec):
            sig = float(np.mean(m)) / case.snr[s]
            spec = m * (1 + 0.2 * x) + sig * rng.standard_normal(npix)
            out[s].append((name, lam, spec, np.full(npix, sig)))
    _spec_cache[case.name] = out
    return out


def specdata(case, cls):
    return [[cls(*a) for a in sp] for sp in spectra(case)]


def olibs(case):
    return {n: olib(n) for n, _ in case.arms}


_truth_cache = {}


def truth_job(case, j):
    """(value, gradient [1 + ndim (+ 1)]) of job j by autograd, computed once"""
    key = (case.name, j)
    if key not in _truth_cache:
        s, vel, par, vs = case.jobs[j]
        sds = specdata(case, orc.SpecData)[s]
        with truth.banded_spline(BANDED_ABOVE):
            if case.vsini_grad:
                r = vtruth.chisq_and_grad_vsini(sds, olibs(case), vel, par, vs or 0.0,
                                                npoly=case.npoly, rbf=case.rbf)
            else:
                r = truth.chisq_and_grad(sds, olibs(case), vel, par, vs,
                                         npoly=case.npoly, rbf=case.rbf)
        _truth_cache[key] = r
    return _truth_cache[key]


def restated_job(case, j):
    s, vel, par, vs = case.jobs[j]
    return adj.chisq_and_grad(specdata(case, orc.SpecData)[s], olibs(case), vel, par, vs,
                              npoly=case.npoly, rbf=case.rbf, vsini_grad=case.vsini_grad)


def rel_err(g, ref):
    """the project's metric: |g - ref| / max(|ref_k|, 1e-6 |ref|_inf)"""
    g, ref = np.asarray(g), np.asarray(ref)
    return np.abs(g - ref) / np.maximum(np.abs(ref), 1e-6 * np.abs(ref).max())


# ---- the cases ------------------------------------------------------------------------
def _chunk():
    # m = ntp - 2 unknowns in chunks of 13 rows per thread: 30 -> 3 threads, last chunk
    # of 4; 31; 39 = 3 x 13; 260 = 20 x 13 and one more row; 832 = 64 x 13, an exact
    # wave fill, then 1 row, 1, 2 and 3 full chunks into wave 1; 5824 = 448 x 13, wave 7
    # empty, then wave 7 with one row
    out = [Case('chunk-cut%d' % n, 'chunk', [(cut(n), n // 2)], 5, Rs=(None, 1.6), seed=n)
           for n in (32, 33, 41, 262, 263, 834, 835, 847, 860, 873)]
    out += [Case('chunk-fine%d' % n, 'chunk', [(fine(n), n // 2)], 5, Rs=(None, 1.6),
                 seed=n) for n in (5826, 5827)]
    return out


def _production():
    kw = dict(npoly=10, Rs=(0.7, 9.3), vsini_grad=True)
    return [
        Case('prod-desi', 'production', [(fine(6215), 2751), (fine(5303), 2326),
                                         (fine(6449), 2881)], seed=11, **kw),
        Case('prod-lds-limit', 'production', [(fine(6485), 3242)], seed=12, **kw),
        Case('prod-sdss1', 'production', [(sdss1(), 2900)], seed=13, **kw),
    ]


def _packing():
    kw = dict(npoly=5, vsini_grad=True)
    return [
        Case('pack-cut64-32', 'packing', [(cut(64), 32)], Rs=(9.3, ), seed=21, **kw),
        Case('pack-cut65-32', 'packing', [(cut(65), 32)], Rs=(9.3, ), seed=22, **kw),
        Case('pack-cut33-16', 'packing', [(cut(33), 16)], Rs=(9.3, ), seed=23, **kw),
        # kmax = ceil(R + 1) = 13: 2 (kmax + 3) = 32 = ntp, the last admitted
        Case('pack-cut32-kmax13', 'packing', [(cut(32), 16)], Rs=(11.5, ), seed=24, **kw),
    ]


def _every_p():
    out = [Case('p%d-cut263' % p, 'every_p', [(cut(263), 131)], p, Rs=(None, 1.6),
                seed=30 + p) for p in range(1, 11)]
    # npix = npoly = 10 with the Chebyshev continuum: the pixels of a linspace are
    # symmetric about the centre, 10 of them span 5 even functions, and the default basis
    # (1, x, x^2, 7 Gaussians on symmetric centres) holds 6 -- it is exactly singular
    # there (condition 2e16, log|det R| is rounding noise: numpy's QR and SVD differ by
    # 0.36), so no value can be held to a truth; the Chebyshev one has condition 15
    out += [Case('p%d-cut32-npix%d' % (p, n), 'every_p', [(cut(32), n)], p, seed=40 + p,
                 rbf=(n, p) != (10, 10))
            for n, p in ((2, 2), (5, 5), (10, 10), (2, 1))]
    return out


def _dims():
    out = []
    for nd in (1, 2, 3):
        name = lowdim(cut(262), nd)
        for vg in (False, True):
            out.append(Case('nd%d%s' % (nd, '-vsini' if vg else ''), 'dims',
                            [(name, 131)], 7, Rs=((1.6, ) if vg else (None, )),
                            vsini_grad=vg, queries=(Q0, QLAST), seed=50 + nd))
    return out


def _linear():
    return [Case('linear-cut263', 'linear', [(linear(cut(263)), 131)], 10, seed=61)]


def _mixed():
    # R = 1 on the 32 knots is R = 6.6 on the 6485: another kmax per arm
    return [Case('mixed-cut32-fine6485', 'mixed', [(cut(32), 16), (fine(6485), 3242)], 5,
                 Rs=(None, 1.0), seed=71)]


REFUSED_SEED = 1024


def _refused_plain():
    # the jobs of the refusal test (R = 12.5 on 32 knots) WITHOUT rotation: what the
    # kernel computes when it refuses the rotational kernel
    return [Case('refused-plain', 'refused_plain', [(cut(32), 16)], 5, seed=REFUSED_SEED)]


_cases = {}


def cases(group=None):
    if not _cases:
        for c in (_chunk() + _production() + _packing() + _every_p() + _dims() +
                  _linear() + _mixed() + _refused_plain()):
            assert c.name not in _cases
            _cases[c.name] = c
    return [c for c in _cases.values() if group is None or c.group == group]


def names(group=None):
    return [c.name for c in cases(group)]


def case(name):
    cases()
    return _cases[name]


def config():
    return dict(GOLD_CONFIG, template_lib=ROOT)
