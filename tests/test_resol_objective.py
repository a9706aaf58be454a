"""Resolution matrices inside the one-kernel objective (objective_kernel<.., RESOL>,
csrc/objective.hip): rvs_objective_fused / rvs_objective_from_template apply the
band to the pixels' spline values in LDS.  Held against the chain of stand-alone
kernels (engine.FUSED_OBJECTIVE_RESOL = False: rvs_chisq_point with the same taps,
range tests per term) and the reference's get_chisq values of resol_cases.npz."""
import os

import numpy as np
import pytest

from conftest import GOLD, GOLD_CONFIG, gold_lib_dict, gold_specdata

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------
# CPU: the condition both the launcher and engine.can_fuse_objective go by
# --------------------------------------------------------------------------
def test_objective_resol_ok_truth_table():
    """rvs_objective_resol_ok(npoly, npix, ntp, nd) is host arithmetic (no device):
    nd odd <= 33, 2 npix <= ntp, npix + nd - 1 <= ntp, and from npoly = 11 on the
    wave totals (8 rows of npoly (npoly + 3) / 2 + 1 sums) inside one template buffer"""
    from rvspecfit_amd import _lib
    ok = _lib.lib().rvs_objective_resol_ok
    # the three DESI arms with DESI's 11 diagonals
    for npix, ntp in ((2751, 6215), (2326, 5303), (2881, 6449)):
        for npoly in (1, 5, 10, 15, 16):
            assert ok(npoly, npix, ntp, 11) == 1
    for nd in range(-1, 40):
        assert ok(10, 351, 937, nd) == int(nd >= 1 and nd % 2 == 1 and nd <= 33), nd
    assert ok(10, 351, 937, 377) == 0            # R = 50 on SDSS: the chain
    assert ok(10, 3842, 5971, 11) == 0           # 2 npix > ntp: not the cached form
    assert ok(10, 468, 937, 11) == 1 and ok(10, 469, 937, 11) == 0
    assert ok(10, 16, 32, 33) == 0 and ok(10, 16, 48, 33) == 1   # npix + nd - 1 <= ntp
    for npoly in range(11, 17):
        need = 8 * (npoly * (npoly + 3) // 2 + 1)
        assert ok(npoly, 100, need, 11) == 1 and ok(npoly, 100, need - 1, 11) == 0
    assert ok(10, 100, 300, 11) == 1             # (no such bound up to npoly = 10)
    assert ok(0, 100, 937, 11) == 0 and ok(17, 100, 937, 11) == 0
    assert ok(10, 0, 937, 11) == 0 and ok(10, 10, 31, 1) == 0 and ok(10, 10, 8193, 1) == 0


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
@pytest.fixture(scope='module')
def gpu():
    import torch
    from rvspecfit_amd import _lib
    _lib.require_gpu()
    _lib.lib()
    return torch.device('cuda')


@pytest.fixture(scope='module')
def config(gpu):
    from rvspecfit_amd import spec_inter
    from rvspecfit_amd.library import TemplateLibrary
    cfg = dict(GOLD_CONFIG, template_lib='golden://')
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, gold_lib_dict(n)), 'golden://')
    return cfg


@pytest.fixture(scope='module')
def rcases():
    return dict(np.load(os.path.join(GOLD, 'resol_cases.npz')))


def _dia(g, key, n):
    import scipy.sparse
    return scipy.sparse.dia_matrix((g[key + '/data'], g[key + '/offsets']), shape=(n, n))


def _band(n, nd, seed):
    """a banded matrix of nd diagonals whose every entry -- the first and last
    (nd - 1) / 2 rows included -- is non-trivial; rows sum to one"""
    import scipy.sparse
    from rvspecfit_amd import spec_fit
    rng = np.random.RandomState(seed)
    h = (nd - 1) // 2
    offs = np.arange(-h, h + 1)
    data = rng.uniform(0.3, 1.0, (nd, n)) * np.exp(-0.5 * (offs[:, None] / (0.4 * h + 0.5))**2)
    M = scipy.sparse.dia_matrix((data, offs), shape=(n, n)).tocsr()
    M = scipy.sparse.diags(1.0 / np.asarray(M.sum(axis=1)).ravel()) @ M
    return spec_fit.ResolMatrix(scipy.sparse.dia_matrix(M))


def _both(fn):
    """fn() with the band inside the kernel and on the chain"""
    from rvspecfit_amd import engine
    out = {}
    for on in (True, False):
        engine.FUSED_OBJECTIVE_RESOL = on
        try:
            with np.errstate(all='ignore'):
                out[on] = fn()
        finally:
            engine.FUSED_OBJECTIVE_RESOL = True
    return out[True], out[False]


def _close(c1, c0, tol=1e-11):
    import torch
    sc = torch.clamp(c0.abs(), min=1e3)
    fin = torch.isfinite(c0)
    assert torch.equal(fin, torch.isfinite(c1))
    return float(((c1 - c0).abs() / sc)[fin].max()) < tol


def _jobs(J, seed, S=1, rot=True):
    import torch
    rng = np.random.RandomState(seed)
    par = np.stack([rng.uniform(5000, 6800, J), rng.uniform(1.5, 4.5, J),
                    rng.uniform(-1.5, -0.1, J), rng.uniform(0.0, 0.4, J)], 1)
    par[::17, 0] = 9000.0          # points outside the grid: nearest neighbour
    vs = torch.as_tensor(rng.uniform(0, 120, J)).to('cuda') if rot else None
    return (torch.as_tensor(rng.randint(0, S, J)).to('cuda'),
            torch.as_tensor(rng.uniform(-300, 300, J)).to('cuda'),
            torch.as_tensor(par).to('cuda'), vs)


@pytest.mark.gpu
@pytest.mark.parametrize('tag', ['c1', 'c2'])
def test_objective_fused_with_resolution(cases, rcases, config, tag):
    """`resol_params` (one matrix per arm, taps_stride 0: 13 diagonals) and the
    spectra's own matrices (9): the kernel against the chain and against the
    reference's get_chisq values"""
    import torch
    from rvspecfit_amd import engine, spec_fit, spec_inter
    g = rcases
    sds = gold_specdata(cases, tag, spec_fit.SpecData)
    rp = {sd.name: spec_fit.ResolMatrix(_dia(g, '%s/rp/%s' % (tag, sd.name), len(sd.lam)))
          for sd in sds}
    sds2 = [spec_fit.SpecData(sd.name, sd.lam, sd.spec, sd.espec, badmask=sd.badmask,
                              resolution=spec_fit.ResolMatrix(
                                  _dia(g, '%s/own/%s' % (tag, sd.name), len(sd.lam))))
            for sd in sds]
    opt = dict(npoly=10)
    for which, ss, kw in (('rp', sds, dict(resol_params=rp)), ('own', sds2, {})):
        b, _ = spec_fit.as_batch(ss)
        libs = spec_inter.get_libs(b.names, config)
        rs = spec_fit._resols(b, kw.get('resol_params'))
        assert engine.can_fuse_objective(b, libs, rs, npoly=10)
        for rot in (False, True):
            ii = [i for i in range(3)
                  if np.isfinite(g['%s/rp/t%d/vsini' % (tag, i)]) == rot]
            if not ii:
                continue
            vel = torch.as_tensor([float(g['%s/rp/t%d/vel' % (tag, i)]) for i in ii],
                                  dtype=torch.float64).to('cuda')
            par = torch.as_tensor(np.array([g['%s/rp/t%d/param' % (tag, i)]
                                            for i in ii])).to('cuda')
            vs = torch.as_tensor([float(g['%s/rp/t%d/vsini' % (tag, i)]) for i in ii],
                                 dtype=torch.float64).to('cuda') if rot else None
            idx = torch.zeros(len(ii), dtype=torch.long, device='cuda')
            (c1, s1), (c0, s0) = _both(lambda: spec_fit.chisq_jobs(
                b, idx, vel, par, vs, opt, config, **kw))
            assert torch.equal(s0, s1)
            assert _close(c1, c0), (which, rot, c1, c0)
            for k, i in enumerate(ii):
                want = float(g['%s/%s/t%d/value' % (tag, which, i)])
                assert abs(c1[k].item() - want) < 1e-7 * max(abs(want), 1e3), (which, i)


@pytest.mark.gpu
@pytest.mark.parametrize('nd', [1, 9, 11, 21, 33])
def test_objective_band_widths_edges_and_launch_forms(cases, config, nd):
    """bands of 1 ... 33 diagonals with non-trivial first and last rows (the chain's
    point kernel tests every term's pixel index, the objective kernel multiplies zeros
    it keeps on both sides of the spline values), per-spectrum matrices of a
    three-spectrum batch; npoly 5 / 10 / 12 (one pass, one pass, split passes with
    the wave totals in the template buffer -- 15 needs 1088 knots for them, the golden
    arms have 977 and 781: the chain); launches with the cell search in the
    block (J narm <= obj_inblk_max), with cell records, and in cell order (J >= 512);
    points outside the grid; with and without rotation; a device job count"""
    import torch
    from rvspecfit_amd import engine, spec_fit, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    base = gold_specdata(cases, 'c1', spec_fit.SpecData)
    rng = np.random.RandomState(nd)
    many = []
    for s in range(3):
        many.append([spec_fit.SpecData(
            sd.name, sd.lam, sd.spec * (1 + 0.01 * rng.normal(size=len(sd.lam))),
            sd.espec, badmask=sd.badmask,
            resolution=_band(len(sd.lam), nd, 100 * nd + 10 * s + ia))
            for ia, sd in enumerate(base)])
    b = SpecBatch.from_specdata(many)
    libs = spec_inter.get_libs(b.names, config)
    assert all(a.resol['nd'] == nd and a.resol['stride'] == a.npix * nd for a in b.arms)
    assert not engine.can_fuse_objective(b, libs, None, npoly=15)
    for npoly in (5, 10, 12):
        assert engine.can_fuse_objective(b, libs, None, npoly=npoly)
        engine.FUSED_OBJECTIVE_RESOL = False
        try:
            assert not engine.can_fuse_objective(b, libs, None, npoly=npoly)
        finally:
            engine.FUSED_OBJECTIVE_RESOL = True
        for J, rot in ((40, True), (400, False), (600, True)):
            if npoly != 10 and J == 400:
                continue
            idx, vel, par, vs = _jobs(J, J + nd, S=3, rot=rot)
            (c1, s1), (c0, s0) = _both(lambda: spec_fit.chisq_jobs(
                b, idx, vel, par, vs, dict(npoly=npoly), config))
            assert torch.equal(s0, s1), (npoly, J)
            assert torch.isfinite(c1).all()
            assert _close(c1, c0), (npoly, J, float((c1 - c0).abs().max()))
    # the job count on the device (what the lock-step optimiser passes)
    J = 600
    idx, vel, par, vs = _jobs(J, 7, S=3)
    kw = dict(npoly=10, rbf=True, job_spec=idx.to(torch.int32))
    with np.errstate(all='ignore'):
        c1, s1 = engine.objective_fused(b, libs, par, vs, vel, **kw)
        for n in (1, 300, 555):
            cnt = torch.tensor([n], dtype=torch.int32, device='cuda')
            out = torch.full((J, ), -7.0, dtype=torch.float64, device='cuda')
            c2, s2 = engine.objective_fused(b, libs, par, vs, vel, njobs=cnt, out=out, **kw)
            assert torch.equal(c2[:n], c1[:n]) and torch.equal(s2[:n], s1[:n])
            assert (c2[n:] == -7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize('nd', [35, 377])
def test_wide_bands_keep_the_chain(cases, config, nd):
    """more than 33 diagonals (377: R = 50 on an SDSS spectrum): not admitted, the
    launcher returns an argument error without launching, chisq_jobs computes what it
    did before (the chain)"""
    import torch
    from rvspecfit_amd import _lib, engine, spec_fit, spec_inter
    sds = gold_specdata(cases, 'c1', spec_fit.SpecData)
    # (377 diagonals need a wider matrix than the 301 / 401 pixels have room for in
    # their corners only: the band is simply full there)
    rp = {sd.name: _band(len(sd.lam), nd, nd) for sd in sds}
    b, _ = spec_fit.as_batch(sds)
    libs = spec_inter.get_libs(b.names, config)
    rs = spec_fit._resols(b, rp)
    assert rs[0]['nd'] == nd
    assert not engine.can_fuse_objective(b, libs, rs, npoly=10)
    idx, vel, par, vs = _jobs(12, nd)
    with pytest.raises(_lib.RvsGpuError):
        engine.objective_fused(b, libs, par, vs, vel, npoly=10,
                               job_spec=idx.to(torch.int32), resols=rs)
    (c1, s1), (c0, s0) = _both(lambda: spec_fit.chisq_jobs(
        b, idx, vel, par, vs, dict(npoly=10), config, resol_params=rp))
    assert torch.equal(c1, c0) and torch.equal(s1, s0) and torch.isfinite(c1).all()


@pytest.mark.gpu
def test_objective_resolution_on_a_grid_set(cases, config):
    """spectra of one arm on wavelength grids of their own (different lengths), each
    with its own matrix of 9 ... 21 diagonals: rows and taps behind a spectrum's own
    pixels are zero, the batch's band is the widest"""
    import torch
    from rvspecfit_amd import engine, spec_fit, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    sd = [s for s in gold_specdata(cases, 'c1', spec_fit.SpecData) if s.name == 'gold_r'][0]
    cuts = [(0, 301, 9), (0, 280, 13), (12, 290, 21), (5, 301, 11)]
    sds = [[spec_fit.SpecData('gold_r', sd.lam[a:z], sd.spec[a:z], sd.espec[a:z],
                              badmask=sd.badmask[a:z],
                              resolution=_band(z - a, nd, 50 + i))]
           for i, (a, z, nd) in enumerate(cuts)]
    b = SpecBatch.from_specdata(sds)
    arm = b.arms[0]
    assert arm.G > 1 and arm.resol['nd'] == 21
    libs = spec_inter.get_libs(b.names, config)
    assert engine.can_fuse_objective(b, libs, None, npoly=10)
    for J in (60, 900):
        idx, vel, par, vs = _jobs(J, J, S=len(cuts))
        (c1, s1), (c0, s0) = _both(lambda: spec_fit.chisq_jobs(
            b, idx, vel, par, vs, dict(npoly=10), config))
        assert torch.equal(s0, s1) and torch.isfinite(c1).all()
        assert _close(c1, c0), J
    # a spectrum of the set alone has the value it has in the batch
    one, _ = spec_fit.as_batch(sds[2])
    idx, vel, par, vs = _jobs(20, 3)
    with np.errstate(all='ignore'):
        ca, _s = spec_fit.chisq_jobs(one, idx, vel, par, vs, dict(npoly=10), config)
        cb, _s = spec_fit.chisq_jobs(b, idx + 2, vel, par, vs, dict(npoly=10), config)
    assert _close(cb, ca)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['triangulation', 'nn'])
def test_objective_from_template_with_resolution(cases, gpu, kind):
    """the same band behind a template row that an evaluator's own kernel wrote
    (rvs_objective_from_template): the golden Delaunay library and the golden MLP"""
    import torch
    from rvspecfit_amd import engine, spec_fit, spec_inter
    from rvspecfit_amd.library import TemplateLibrary
    rng = np.random.RandomState(21)
    if kind == 'triangulation':
        cfg = dict(GOLD_CONFIG, template_lib='golden-tri://')
        for n in ('gold_b', 'gold_r'):
            d = np.load(os.path.join(GOLD, 'lib_tri_%s.npz' % n))
            spec_inter.register_library(TemplateLibrary(n, d), 'golden-tri://')
        base = gold_specdata(cases, 'c1', spec_fit.SpecData)
        sds = [spec_fit.SpecData(sd.name, sd.lam, sd.spec, sd.espec, badmask=sd.badmask,
                                 resolution=_band(len(sd.lam), 11, 3 + i))
               for i, sd in enumerate(base)]
        npoly = 10
    else:
        from test_gpu_parity import _nn_lib
        d = dict(np.load(os.path.join(GOLD, 'nn_case.npz')))
        lam = np.exp(np.linspace(np.log(3950.), np.log(5060.), int(d['dims'][-1])))
        lib = _nn_lib(d, lam)
        lib.name = 'aat_580v'
        spec_inter.register_library(lib, 'golden-nn://')
        cfg = dict(GOLD_CONFIG, template_lib='golden-nn://')
        npx = min(1000, lib.ntp // 2)
        wave = np.linspace(4000, 5000, npx)
        err = np.ones(npx) * 0.1
        sds = [spec_fit.SpecData('aat_580v', wave, rng.normal(wave * 0 + 1, err), err,
                                 resolution=_band(npx, 11, 5))]
        npoly = 5
    b, _ = spec_fit.as_batch(sds)
    libs = spec_inter.get_libs(b.names, cfg)
    assert engine.can_fuse_objective(b, libs, None, npoly=npoly, from_template=True)
    assert not engine.can_fuse_objective(b, libs, None, npoly=npoly)
    J = 24
    par = torch.as_tensor(np.stack([rng.uniform(5000, 6500, J), rng.uniform(1.5, 4, J),
                                    rng.uniform(-1.5, -0.2, J), rng.uniform(0, 0.4, J)],
                                   axis=1)).to('cuda')
    vel = torch.as_tensor(rng.uniform(-300, 300, J)).to('cuda')
    idx = torch.zeros(J, dtype=torch.long, device='cuda')
    for vs in (None, torch.as_tensor(rng.uniform(1, 200, J)).to('cuda')):
        (c1, s1), (c0, s0) = _both(lambda: spec_fit.chisq_jobs(
            b, idx, vel, par, vs, dict(npoly=npoly), cfg))
        assert torch.equal(s0, s1)
        assert torch.isfinite(c1).any()
        assert _close(c1, c0)


@pytest.mark.gpu
def test_process_with_resolution_runs_on_the_device_optimiser():
    """vel_fit.process of three DESI fibres with their resolution matrices and the
    second minimiser: with the band in the kernel the rounds of Nelder-Mead and BFGS
    are driven inside the library (rvs_nm_run / rvs_bfgs_run) and the batch may split
    into concurrent halves; the fit is the chain's"""
    from rvspecfit_amd import fits_min as F, vel_fit, engine, spec_inter
    from rvspecfit_amd.desi import desi_fit as D
    from rvspecfit_amd.library import TemplateLibrary
    for n in ('desi_b', 'desi_r', 'desi_z'):
        spec_inter.register_library(
            TemplateLibrary(n, np.load(os.path.join(GOLD, 'lib_%s.npz' % n))),
            'golden-desi://')
    sig0 = dict(b=0.5, r=0.5, z=0.55)
    cfg = dict(template_lib='golden-desi://', min_vel=-1000, max_vel=1000,
               min_vel_step=0.2, vel_step0=5, min_vsini=0.1, max_vsini=500,
               second_minimizer=True, lsf_sigma0_angstrom=sig0)
    FP = F.open(os.path.join(GOLD, 'coadd-golden.fits'))
    fl, iv, ms, wv, rs = D.read_data(FP, ['b', 'r', 'z'])
    cond = D.get_specdata_batch(wv, fl, iv, ms, rs, [0, 2, 11], ['b', 'r', 'z'],
                                use_resolution_matrix=True, lsf_sigma0_angstrom=sig0)
    batch = D._arm_batch(cond, ['b', 'r', 'z'], (True, True, True), np.arange(3), wv,
                         'cuda')
    assert all(a.resol is not None and a.resol['nd'] == 11 for a in batch.arms)
    libs = spec_inter.get_libs(batch.names, cfg)
    p0 = dict(teff=5200., logg=2.5, feh=-1., alpha=0.2, vsini=10.)
    opt = dict(npoly=10)
    res, flags = {}, {}
    for on in (True, False):
        engine.FUSED_OBJECTIVE_RESOL = on
        try:
            flags[on] = (engine.can_fuse_objective(batch, libs, None, npoly=10),
                         vel_fit._rounds_run_in_c(batch, cfg, None, opt))
            res[on] = vel_fit.process(batch, dict(p0), config=cfg, options=opt)
        finally:
            engine.FUSED_OBJECTIVE_RESOL = True
    assert flags[True] == (True, True) and flags[False] == (False, False)
    a, c = res[True], res[False]
    msg = 'kernel: nm_rounds %s objective_evals %s; chain: nm_rounds %s objective_evals %s' % (
        a['nm_rounds'], a['objective_evals'], c['nm_rounds'], c['objective_evals'])
    na = lambda r, k: np.asarray(r[k].cpu().numpy(), dtype=float)
    same = (np.array_equal(na(a, 'nm_nit'), na(c, 'nm_nit')) and
            np.array_equal(na(a, 'nm_nfev'), na(c, 'nm_nfev')))
    print(msg, 'same path' if same else 'paths differ')
    assert np.allclose(na(a, 'chisq'), na(c, 'chisq'), rtol=1e-6, atol=0), msg
    assert np.allclose(na(a, 'vel'), na(c, 'vel'), atol=1e-3, rtol=0), msg
