"""rvs_vsini_convolve_grad and the vsini component of the analytic gradient
(build_templates(vsini_tangent=True), get_chisq_grad / chisq_grad_jobs /
chisq_func0_grad(vsini_grad=True), chisq_func_grad) against tests/vsini_grad_truth.py
(float64 on the CPU, pinned to the oracle by test_vsini_grad_cpu.py): the golden arms
gold_b / gold_r and the three spectra of chisq_grad_truth.SPECTRA."""

import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG, gold_lib_dict
from oracle import rvs_oracle as orc

import chisq_grad_truth as truth
import vsini_grad_truth as vtruth

pytestmark = pytest.mark.gpu
NPOLY = [5, 10, 16]

# NOT YET MEASURED on an MI355X: no GPU could be had while this file was written, so
# both bounds below come from the number format, not from a run.  They are to be replaced
# by 10 x the largest error seen (as MEASURED_REL_ERR of test_chisq_grad_gpu.py is) at
# the first run; every test prints its figures before it asserts.
#
# Tangent row of rvs_vsini_convolve_grad against numpy's convolve(in, dw/dvsini, 'same')
# of the CPU taps, relative to max |row|.  W'_k is a difference of two values of the
# primitive of x K (size <= 0.2, so ~1e-16 absolute), W' - w S' loses at most two digits
# at R = 40 (terms ~1e-2, result ~3e-4 per unit of S), the 2 kmax + 1 <= 83 products
# of a row add in float64 fma: ~1e-13 of the row's largest entry expected, ~4e-13 if
# every tap error aligned.  Bound: 1e-12.
FIR_REL_ERR_BOUND = 1e-12
# Gradient against the truth, relative to max(|g_k|, 1e-6 max_k |g_k|): the vsini row
# goes through the spline and the sums of point_grad_block_kernel as the parameter
# rows do, with taps good to the above, so the bound of test_chisq_grad_gpu.py for
# those kernels (10 x 5.84e-13 measured there on an MI355X) is asked of all six
# components.
REL_ERR_BOUND = 10 * 5.84e-13

# (job of truth.JOBS whose spectrum, velocity and in-cell parameters are used, arm
# whose lnstep sets the scale, R on that arm): R < 1, 1 < R < 2, R > 5, R within 1e-3
# of an integer on the blue and on the red arm; the last job is not broadened
VJOBS = [(0, 'gold_b', 0.6), (1, 'gold_b', 1.5), (2, 'gold_b', 7.3),
         (3, 'gold_b', 2.0005), (4, 'gold_r', 1.0003), (0, 'gold_b', 0.0)]
J = len(VJOBS)


@pytest.fixture(scope='module')
def setup(cases):
    from rvspecfit_amd import _lib, spec_inter, spec_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    cfg = dict(GOLD_CONFIG, template_lib='golden://')
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, gold_lib_dict(n)), 'golden://')
    sds = truth.spectra(cases, spec_fit.SpecData)
    batch = SpecBatch.from_specdata(sds)
    libs = spec_inter.get_libs(batch.names, cfg)
    dev = batch.device
    f64 = dict(dtype=torch.float64, device=dev)
    vs = [r * orc.SPEED_OF_LIGHT * libs[a].lnstep for _, a, r in VJOBS]
    for (j, a, r), v in zip(VJOBS, vs):
        print('job %d (arm %s R %g): vsini %.6f km/s, R %s' % (
            j, a, r, v, ' '.join('%s %.6f' % (n, v / orc.SPEED_OF_LIGHT / libs[n].lnstep)
                                 for n in libs)))
    jobs = [truth.JOBS[j] for j, _, _ in VJOBS]
    return dict(cfg=cfg, sds=sds, batch=batch, libs=libs, dev=dev, vs_list=vs,
                idx=torch.tensor([j[0] for j in jobs], device=dev),
                vel=torch.tensor([j[1] for j in jobs], **f64),
                par=torch.tensor([j[2] for j in jobs], **f64),
                vs=torch.tensor(vs, **f64))


@pytest.fixture(scope='module')
def olibs():
    return {n: orc.Library(gold_lib_dict(n)) for n in ('gold_b', 'gold_r')}


_want = {}


def _truth(cases, olibs, su, npoly):
    if npoly not in _want:
        sp = truth.spectra(cases, orc.SpecData)
        _want[npoly] = [vtruth.chisq_and_grad_vsini(
            sp[truth.JOBS[j][0]], olibs, truth.JOBS[j][1], truth.JOBS[j][2], v,
            npoly=npoly) for (j, _, _), v in zip(VJOBS, su['vs_list'])]
    return _want[npoly]


# ---- 1. the FIR kernel ------------------------------------------------------------
LNSTEP = 1e-4
FIR_R = [0.3, 1.0, 2.0, 2.5, 7.3, 40.0]


def _convolve_grad(templ, vsini, outside=None, lnstep=LNSTEP):
    from rvspecfit_amd import _lib
    B, R, ntp = templ.shape
    out = torch.full((B, R + 1, ntp), float('nan'), dtype=torch.float64,
                     device=templ.device)
    rc = _lib.lib().rvs_vsini_convolve_grad(_lib.ptr(templ), _lib.ptr(vsini),
                                            _lib.ptr(outside), lnstep, 0.6, ntp, R, B,
                                            _lib.ptr(out), _lib.stream())
    _lib.check(rc, 'rvs_vsini_convolve_grad')
    return out


def _convolve(templ, vsini, outside=None, lnstep=LNSTEP):
    """rvs_vsini_convolve on the same rows: one vsini / outside per row"""
    from rvspecfit_amd import _lib
    B, R, ntp = templ.shape
    out = torch.empty_like(templ)
    rc = _lib.lib().rvs_vsini_convolve(
        _lib.ptr(templ), _lib.ptr(vsini.repeat_interleave(R)),
        _lib.ptr(None if outside is None else outside.repeat_interleave(R)), lnstep,
        0.6, ntp, B * R, _lib.ptr(out), _lib.stream())
    _lib.check(rc, 'rvs_vsini_convolve')
    return out


def test_fir_kernel(setup):
    """B = 4 jobs of R = 3 rows, ntp = 96, every job at another tap width: rows < R are
    the bits of rvs_vsini_convolve; row R is numpy's 'same' convolution of row 0 with
    the CPU truth's dw/dvsini.  R = 40 is wider than half the row, 1.0 and 2.0 sit on
    the change of the tap count."""
    dev = setup['dev']
    rng = np.random.default_rng(20261017)
    worst = 0.0
    for rv in (FIR_R[:4], FIR_R[2:]):
        x = rng.standard_normal((4, 3, 96)) + 1.0
        vs = np.array(rv) * orc.SPEED_OF_LIGHT * LNSTEP
        t = torch.as_tensor(x).to(dev)
        v = torch.as_tensor(vs).to(dev)
        out = _convolve_grad(t, v)
        assert torch.equal(out[:, :3], _convolve(t, v))
        got = out[:, 3].cpu().numpy()
        for b in range(4):
            R = (vs[b] / orc.SPEED_OF_LIGHT) / LNSTEP      # as the kernel forms it
            _, dw = vtruth.taps(R)
            ref = np.convolve(x[b, 0], dw / (orc.SPEED_OF_LIGHT * LNSTEP), 'same')
            err = np.abs(got[b] - ref).max() / np.abs(ref).max()
            print('R %.17g taps %d max |row| %.4g relative error %.3g'
                  % (R, len(dw), np.abs(ref).max(), err))
            worst = max(worst, err)
    print('largest relative error of the tangent row %.3g' % worst)
    assert worst <= FIR_REL_ERR_BOUND


def test_fir_kernel_copy_cases(setup):
    """vsini 0, -1, NaN, a non-finite outside flag, more taps than the kernel keeps:
    rows < R are the input's bits, row R has no nonzero entry"""
    dev = setup['dev']
    rng = np.random.default_rng(7)
    t = torch.as_tensor(rng.standard_normal((5, 3, 96))).to(dev)
    v = torch.tensor([0.0, -1.0, float('nan'), 30.0,
                      2100 * orc.SPEED_OF_LIGHT * LNSTEP], dtype=torch.float64,
                     device=dev)
    o = torch.tensor([0.0, 0.0, 0.0, float('nan'), 0.0], dtype=torch.float64,
                     device=dev)
    out = _convolve_grad(t, v, o)
    assert torch.equal(out[:, :3], t)
    assert not out[:, 3].ne(0).any()          # (NaN != 0 counts as nonzero)
    assert torch.equal(out[:, :3], _convolve(t, v, o))
    # the same vsini = 30 without the flag is broadened
    out2 = _convolve_grad(t[3:4], v[3:4])
    assert out2[0, 3].ne(0).any() and not torch.equal(out2[0, :3], t[3])


# ---- 2. the gradient against the truth --------------------------------------------
def _grad_jobs(su, npoly, vsini_grad=True, order=None):
    from rvspecfit_amd import spec_fit
    sel = torch.tensor(list(range(J)) if order is None else order, device=su['dev'])
    return spec_fit.chisq_grad_jobs(su['batch'], su['idx'][sel], su['vel'][sel],
                                    su['par'][sel], su['vs'][sel], dict(npoly=npoly),
                                    su['cfg'], vsini_grad=vsini_grad)


def _forward_difference(su, npoly):
    """scipy's forward difference, step 1.49e-8 * max(|x|, 1), of engine.chisq_point
    in x = (vel, *params, vsini), templates rebuilt at every point"""
    from rvspecfit_amd import engine
    b, libs = su['batch'], su['libs']
    x = torch.cat([su['vel'][:, None], su['par'], su['vs'][:, None]], dim=1)  # [J, 6]
    n = x.shape[1]
    h = 1.4901161193847656e-08 * torch.clamp(x.abs(), min=1.0)
    pts = x[:, None, :].repeat(1, n + 1, 1)
    for k in range(n):
        pts[:, 1 + k, k] += h[:, k]
    h = pts[:, 1:, :].diagonal(dim1=1, dim2=2) - x                   # as rounded
    pts = pts.reshape(J * (n + 1), n)
    cf, og = [], []
    for arm in b.arms:
        c, o = engine.build_templates(libs[arm.name], pts[:, 1:-1].contiguous(),
                                      pts[:, -1].contiguous())
        cf.append(c)
        og.append(o)
    js = su['idx'].repeat_interleave(n + 1).to(torch.int32).contiguous()
    f, _ = engine.chisq_point(b, libs, cf, og, pts[:, 0].contiguous(), npoly=npoly,
                              rbf=True, job_spec=js)
    f = f.reshape(J, n + 1)
    return ((f[:, 1:] - f[:, :1]) / h).cpu().numpy()


@pytest.mark.parametrize('npoly', NPOLY)
def test_gradient_against_the_truth(cases, setup, olibs, npoly):
    """per component, the new one included: the analytic gradient is no further from
    the truth than scipy's forward difference of engine.chisq_point, and within
    REL_ERR_BOUND of it relative to max(|g_k|, 1e-6 |g|_inf); the job that is not
    broadened has a vsini component of exactly 0; the first 1 + ndim columns are the
    bits of the call without vsini_grad"""
    want = _truth(cases, olibs, setup, npoly)
    chi, grad, st = _grad_jobs(setup, npoly)
    chi0, grad0, st0 = _grad_jobs(setup, npoly, vsini_grad=False)
    assert grad.shape == (J, 6) and grad0.shape == (J, 5)
    assert torch.equal(grad[:, :5], grad0) and torch.equal(chi, chi0)
    assert torch.equal(st, st0)
    grad = grad.cpu().numpy()
    fd = _forward_difference(setup, npoly)
    worst = 0.0
    bad = []
    for j in range(J):
        val, g = want[j]
        assert int(st[j].item()) == 0
        assert abs(chi[j].item() - val) <= 1e-7 * abs(val)
        scale = np.maximum(np.abs(g), 1e-6 * np.abs(g).max())
        e_an, e_fd = np.abs(grad[j] - g), np.abs(fd[j] - g)
        for k in range(6):
            print('npoly %d job %d comp %d truth %.12g analytic err %.3g (rel %.3g) '
                  'forward-difference err %.3g' % (npoly, j, k, g[k], e_an[k],
                                                   e_an[k] / scale[k], e_fd[k]))
            if not (e_an[k] <= e_fd[k] and e_an[k] <= REL_ERR_BOUND * scale[k]):
                bad.append((j, k, e_an[k], e_fd[k], e_an[k] / scale[k]))
        worst = max(worst, float((e_an / scale).max()))
    print('npoly %d largest relative error %.3g' % (npoly, worst))
    assert grad[J - 1, 5] == 0.0 and want[J - 1][1][5] == 0.0
    assert not bad, bad


# ---- 3. determinism ----------------------------------------------------------------
def test_determinism(setup):
    """two calls: the same bits; the jobs permuted: the permuted rows, bit for bit"""
    chi, grad, st = _grad_jobs(setup, 10)
    chi2, grad2, st2 = _grad_jobs(setup, 10)
    assert torch.equal(grad, grad2) and torch.equal(chi, chi2)
    perm = [4, 2, 5, 0, 1, 3]
    chi3, grad3, st3 = _grad_jobs(setup, 10, order=perm)
    sel = torch.tensor(perm, device=setup['dev'])
    assert torch.equal(grad3, grad[sel]) and torch.equal(chi3, chi[sel])
    assert torch.equal(st3, st[sel])


# ---- 4. the public interface -------------------------------------------------------
def test_public_shapes_and_single_spectrum(setup):
    from rvspecfit_amd import engine, spec_fit
    su = setup
    opt = dict(npoly=10)
    chi, grad, st = _grad_jobs(su, 10)
    assert chi.shape == (J, ) and grad.shape == (J, 6)
    # spectra 0, 1, 2 are those of jobs 0, 1, 2
    cb, gb = spec_fit.get_chisq_grad(su['batch'], su['vel'][:3], su['par'][:3],
                                     su['vs'][:3], options=opt, config=su['cfg'],
                                     vsini_grad=True)
    assert cb.shape == (3, ) and gb.shape == (3, 6)
    assert torch.equal(gb, grad[:3]) and torch.equal(cb, chi[:3])
    for s in range(3):
        _, vel, par, _ = truth.JOBS[VJOBS[s][0]]
        c1, g1 = spec_fit.get_chisq_grad(su['sds'][s], vel, par, (su['vs_list'][s], ),
                                         options=opt, config=su['cfg'],
                                         vsini_grad=True)
        assert isinstance(c1, float) and g1.shape == (6, )
        assert c1 == cb[s].item() and (g1 == gb[s].cpu().numpy()).all()
        c0, g0 = spec_fit.get_chisq_grad(su['sds'][s], vel, par, (su['vs_list'][s], ),
                                         options=opt, config=su['cfg'])
        assert c0 == c1 and g0.shape == (5, ) and (g0 == g1[:5]).all()
    # no rotation: nothing to differentiate by
    _, vel, par, _ = truth.JOBS[0]
    with pytest.raises(ValueError, match='vsini'):
        spec_fit.get_chisq_grad(su['sds'][0], vel, par, None, options=opt,
                                config=su['cfg'], vsini_grad=True)
    with pytest.raises(ValueError, match='vsini'):
        spec_fit.chisq_grad_jobs(su['batch'], su['idx'], su['vel'], su['par'], None,
                                 opt, su['cfg'], vsini_grad=True)
    lib = su['libs']['gold_b']
    with pytest.raises(ValueError, match='vsini'):
        engine.build_templates(lib, su['par'], None, tangents=True, vsini_tangent=True)
    # the rows of build_templates: the vsini row is last, the others are unchanged
    c1, o1, t1 = engine.build_templates(lib, su['par'], su['vs'], return_templ=True,
                                        tangents=True, vsini_tangent=True)
    c0, o0, t0 = engine.build_templates(lib, su['par'], su['vs'], return_templ=True,
                                        tangents=True)
    assert c1.shape == (J, 6, lib.ntp, 4) and t1.shape == (J, 6, lib.ntp)
    assert torch.equal(t1[:, :5], t0) and torch.equal(c1[:, :5], c0)
    # six parameters and vsini: one tangent more than the kernel takes

    class Lib6:
        ndim, kind = 6, 'regulargrid'
    b1 = su['batch']
    with pytest.raises(ValueError, match=r'vsini.*ndim = 6'):
        engine.check_grad_scope(b1, {n: Lib6 for n in b1.names}, 10, vsini_grad=True)
    engine.check_grad_scope(b1, {n: Lib6 for n in b1.names}, 10)


def _func_args(su, fix=None, priors=None):
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.spec_inter import getSpecParams
    names = list(getSpecParams('gold_b', su['cfg']))
    _, vel, par, _ = truth.JOBS[0]
    pd0 = dict(zip(names, par))
    mapper = vel_fit.ParamMapper(names, pd0, fix or [],
                                 vel_fit.VSiniMapper(su['cfg']['max_vsini']),
                                 fitVsini=True)
    args = dict(specdata=su['sds'][0], paramMapper=mapper, options=dict(npoly=10),
                config=su['cfg'], priors=priors, min_vel=su['cfg']['min_vel'],
                max_vel=su['cfg']['max_vel'])
    return args, names, vel, par


def test_chisq_func_grad(setup):
    from rvspecfit_amd import spec_fit, vel_fit
    su = setup
    args, names, vel, par = _func_args(su)
    vs = su['vs_list'][1]
    p = np.array([vel, vs] + list(par))
    f, g = vel_fit.chisq_func_grad(p, args)
    ref = vel_fit.chisq_func(p, args)
    assert isinstance(f, float) and g.shape == (6, )
    assert abs(f - ref) < 1e-11 * max(abs(ref), 1e3), (f, ref)
    # the optimiser's order (vel, vsini, parameters) of the physical gradient
    _, gp = spec_fit.get_chisq_grad(su['sds'][0], vel, par, (vs, ),
                                    options=args['options'], config=su['cfg'],
                                    vsini_grad=True)
    assert args['paramMapper'].get_fitted_params() == ['vel', 'vsini'] + names
    assert (g == gp[[0, 5, 1, 2, 3, 4]]).all() and g[1] != 0
    f0, g0 = vel_fit.chisq_func0_grad(args['paramMapper'].forward(p), args,
                                      vsini_grad=True)
    assert f0 == f and (g0 == gp).all()
    # a fixed parameter is dropped
    argf, _, _, _ = _func_args(su, fix=['alpha'])
    ia = names.index('alpha')
    keep = [i for i in range(4) if i != ia]
    pf = np.array([vel, vs] + [par[i] for i in keep])
    ff, gf = vel_fit.chisq_func_grad(pf, argf)
    assert argf['paramMapper'].get_fitted_params() == \
        ['vel', 'vsini'] + [names[i] for i in keep]
    assert ff == f and gf.shape == (5, )
    assert (gf == g[[0, 1] + [2 + i for i in keep]]).all()
    # the clamp of VSiniMapper: no physical derivative, the penalty's alone
    p[1] = -2.0
    f, gm = vel_fit.chisq_func_grad(p, args)
    ref = vel_fit.chisq_func(p, args)
    assert gm[1] == -4.0 and abs(f - ref) < 1e-11 * max(abs(ref), 1e3)
    p[1] = su['cfg']['max_vsini'] + 3.0
    f, gm = vel_fit.chisq_func_grad(p, args)
    ref = vel_fit.chisq_func(p, args)
    assert gm[1] == 6.0 and abs(f - ref) < 1e-11 * max(abs(ref), 1e3)
    # where chisq_func refuses the point
    p[1] = vs
    p[0] = su['cfg']['max_vel'] + 1.0
    f, gm = vel_fit.chisq_func_grad(p, args)
    assert f == 1e30 == vel_fit.chisq_func(p, args)
    assert gm.shape == (6, ) and not gm.any()
    p[0] = vel
    p[3] = float('nan')
    f, gm = vel_fit.chisq_func_grad(p, args)
    assert f == 1e30 and not gm.any()
    # a Normal prior on teff adds 2 (p - mu) / sigma^2 to that component only
    p = np.array([vel, vs] + list(par))
    mu, sig = 5800.0, 150.0
    argp, _, _, _ = _func_args(su, priors={'teff': (mu, sig)})
    f1, g1 = vel_fit.chisq_func_grad(p, argp)
    it = names.index('teff')
    d = g1 - g
    assert d[2 + it] == pytest.approx(2 * (par[it] - mu) / sig**2, rel=1e-9)
    d[2 + it] = 0
    assert not d.any()
    assert f1 - (f0) == pytest.approx(((par[it] - mu) / sig)**2, rel=1e-9)
