"""rvs_template_tri_grad / rvs_template_tri_buckets_grad and the analytic gradient above
them on Delaunay libraries, against tests/tri_grad_truth.py (float64 torch + autograd on
the CPU, itself pinned to the oracle by test_tri_grad_cpu.py): J = 8 jobs over 3 spectra
on the two golden Delaunay arms (ndim 4, 5718 simplices, ntp 977 / 781), npoly 5, 10
and 16, and small synthetic triangulations through the C entry points."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLD, GOLD_CONFIG
from oracle import rvs_oracle as orc

import tri_grad_truth as ttruth

pytestmark = pytest.mark.gpu
NPOLY = [5, 10, 16]
J = len(ttruth.JOBS)
ND = 4

# Tangent rows of the golden libraries against the truth's autograd rows, relative to
# the row's largest entry (rows of ~5e-5 per K up to ~0.4 per dex).
#   CPU figure: a plain-numpy restatement of the same sums differs from the truth by
#     at most 4.05e-15 of the row's largest entry, 5.0e-16 absolute
#     (test_tri_grad_cpu.py::test_numpy_restatement_of_the_tangent_rows) -- sum_i db_i
#     = 0, so the sums cancel the level of the log-flux rows and keep ~1.5 digits less
#     than the 1.4e-16 absolute of the polylinear rows.
#   MI355X figure: NOT MEASURED YET (no device run while this file was written).
# Until a device run exists the bound is 10 x the CPU figure; it is then to be replaced
# by 10 x the largest error seen.  The test prints every figure before it asserts.
TANGENT_REL_CPU = 4.05e-15
TANGENT_REL_BOUND = 10 * TANGENT_REL_CPU

# Gradient against the truth, relative to max(|g_k|, 1e-6 max_k |g_k|): everything
# behind the template stage is the code test_chisq_grad_gpu.py measured on the
# regular-grid kernels (5.84e-13 on an MI355X), so the starting bound is that file's,
# 10 x 5.84e-13; to be replaced by 10 x the largest error measured here.
#   MI355X figure: NOT MEASURED YET.
REL_ERR_BOUND = 10 * 5.84e-13


def _same(a, b):
    """bit-for-bit, NaN == NaN"""
    return torch.equal(a.isnan(), b.isnan()) and \
        torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


@pytest.fixture(scope='module')
def setup(cases):
    from rvspecfit_amd import _lib, spec_inter, spec_fit
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    cfg = dict(GOLD_CONFIG, template_lib='golden-tri://')
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, ttruth.tri_lib_dict(n)),
                                    'golden-tri://')
    sds = ttruth.spectra(cases, spec_fit.SpecData)
    batch = SpecBatch.from_specdata(sds)
    libs = spec_inter.get_libs(batch.names, cfg)
    assert all(l.kind == 'triangulation' and l._tri_bk is not None
               for l in libs.values())
    dev = batch.device
    f64 = dict(dtype=torch.float64, device=dev)
    return dict(cfg=cfg, sds=sds, batch=batch, libs=libs, dev=dev,
                idx=torch.tensor([j[0] for j in ttruth.JOBS], device=dev),
                vel=torch.tensor([j[1] for j in ttruth.JOBS], **f64),
                par=torch.tensor([j[2] for j in ttruth.JOBS], **f64),
                vs=torch.tensor([j[3] or 0.0 for j in ttruth.JOBS], **f64))


@pytest.fixture(scope='module')
def olibs():
    return ttruth.oracle_libs()


# ---- 1. the template kernel on the golden arms ---------------------------------------
def test_template_rows(setup, olibs):
    """row 0, outside flag, simplex ids and weights are the bits of eval_batch; the
    tangent rows are the truth's dt/dp inside a simplex; every row is NaN where no
    simplex holds the point (outside the hull, non-finite mapped parameter)"""
    par = setup['par']
    worst = 0.0
    for name, lib in setup['libs'].items():
        t0, o0, s0, w0 = lib.eval_batch(par, details=True)
        tg, og, sg, wg = lib.eval_batch_grad(par, details=True)
        assert tg.shape == (J, 1 + ND, lib.ntp)
        assert _same(tg[:, 0], t0) and _same(og, o0)
        assert torch.equal(sg, s0) and torch.equal(wg, w0)
        t2, o2 = lib.eval_batch_grad(par)
        assert _same(t2, tg) and _same(o2, og)
        for j in (ttruth.NO_SIMPLEX, ttruth.NONFINITE):
            assert int(sg[j].item()) == 0x7fffffff
            assert tg[j].isnan().all() and og[j].isnan()
        fin = torch.tensor(ttruth.INSIDE, device=setup['dev'])
        assert torch.isfinite(tg[fin]).all() and not og[fin].any()
        assert torch.equal(tg[fin, 0], t0[fin])
        tg = tg.cpu().numpy()
        for j in ttruth.INSIDE:
            t, jac = ttruth.template_jacobian(olibs[name], ttruth.JOBS[j][2])
            assert np.abs(tg[j, 0] - t).max() <= 1e-12 * np.abs(t).max()
            for k in range(ND):
                ea = np.abs(tg[j, 1 + k] - jac[k]).max()
                er = ea / np.abs(jac[k]).max()
                print('%s job %d dt/dp_%d max %.3g abs err %.3g rel %.3g'
                      % (name, j, k, np.abs(jac[k]).max(), ea, er))
                worst = max(worst, er)
    print('largest error of a tangent row relative to its largest entry %.3g' % worst)
    assert worst <= TANGENT_REL_BOUND


@pytest.mark.parametrize('B', [1, 15])
def test_locate_paths_agree(setup, B):
    """find_simplex through the bucket grid and by the exhaustive search: identical
    tensors, on the 15 points of tri_cases.npz (three of them in no simplex) and on
    the first alone"""
    from rvspecfit_amd import library
    g = np.load(os.path.join(GOLD, 'tri_cases.npz'))
    P = torch.as_tensor(g['params'][:B]).to(setup['dev'])
    assert P.shape == (B, ND)
    for name, lib in setup['libs'].items():
        a = lib.eval_batch_grad(P, details=True)
        v = lib.eval_batch(P, details=True)
        library.TRI_BUCKETS = False
        try:
            b = lib.eval_batch_grad(P, details=True)
        finally:
            library.TRI_BUCKETS = True
        for x, y in zip(a, b):
            assert x.shape == y.shape and _same(x, y)
        assert _same(a[0][:, 0], v[0]) and _same(a[1], v[1])
        assert torch.equal(a[2], v[2]) and torch.equal(a[3], v[3])
        want = g[name + '/simplex'][:B]
        none = torch.as_tensor(want < 0).to(setup['dev'])
        assert torch.equal(a[2] == 0x7fffffff, none)
        assert a[0][none].isnan().all() and a[1][none].isnan().all()
        assert torch.isfinite(a[0][~none]).all()
        if B == 15:
            assert int(none.sum().item()) == 3


# ---- 2. synthetic triangulations through the C entry points --------------------------
def _transform(verts):
    """scipy's Delaunay.transform of one simplex from its vertices [nd + 1, nd]: the
    inverse of the matrix whose columns are vertex_i - vertex_nd, then vertex_nd"""
    nd = verts.shape[1]
    M = (verts[:nd] - verts[nd]).T
    return np.vstack([np.linalg.inv(M), verts[nd][None, :]])


class _SynthLib:
    """what tri_grad_truth.template and the oracle's find_simplex read"""
    map_params = orc.TriLibrary.map_params
    find_simplex = orc.TriLibrary.find_simplex
    _bary = orc.TriLibrary._bary

    def __init__(self, pts, simplices, dats, extraflags, log_ids, exp):
        self.simplices = np.asarray(simplices, dtype=np.int32)
        self.transform = np.array([_transform(pts[s]) for s in self.simplices])
        self.dats, self.extraflags = dats, extraflags
        self.log_ids, self.exp, self.ndim = list(log_ids), bool(exp), pts.shape[1]


def _call(sl, params, grad, dev):
    """rvs_template_tri(_grad) on the arrays of a _SynthLib"""
    from rvspecfit_amd import _lib
    f64 = dict(dtype=torch.float64, device=dev)
    nd, ntp = sl.ndim, sl.dats.shape[1]
    B = len(params)
    keep = [torch.as_tensor(sl.dats).to(dev).contiguous(),
            torch.as_tensor(sl.simplices).to(dev).contiguous(),
            torch.as_tensor(sl.transform).to(dev).contiguous(),
            torch.as_tensor(sl.extraflags).to(dev).contiguous(),
            torch.as_tensor(np.asarray(params, dtype=np.float64)).to(dev).contiguous()]
    templ = torch.full((B, 1 + nd, ntp) if grad else (B, ntp), -7.0, **f64)
    outside = torch.full((B, ), -7.0, **f64)
    sx = torch.zeros(B, dtype=torch.int32, device=dev)
    wts = torch.zeros((B, nd + 1), **f64)
    log_mask = sum(1 << i for i in sl.log_ids)
    L = _lib.lib()
    rc = (L.rvs_template_tri_grad if grad else L.rvs_template_tri)(
        _lib.ptr(keep[0]), ntp, _lib.ptr(keep[1]), _lib.ptr(keep[2]),
        _lib.ptr(keep[3]), len(sl.simplices), nd, log_mask, int(sl.exp),
        _lib.ptr(keep[4]), B, _lib.ptr(templ), _lib.ptr(outside), _lib.ptr(sx),
        _lib.ptr(wts), _lib.stream())
    _lib.check(rc, 'rvs_template_tri')
    torch.cuda.synchronize()
    return templ, outside, sx, wts


def _check_synthetic(sl, params, dev, nfound):
    """row 0 / outside / simplex / weights: the bits of rvs_template_tri; NaN in every
    row without a simplex; tangent rows against autograd within the rounding of the
    sums, in units of u = 1.1e-16 times S_k = t * sum_i |db_i/dp_k| |L_i|: each of the
    nd + 1 <= 7 products and sums rounds once, the table entries (T s_k, s_k =
    1 / (p_k ln 10), the last row a sum of nd) carry <= 4 more, exp and the product
    with t 2 more -- 13 roundings on the device, as many in the truth, 32 to leave a
    margin; with exp the factor t also carries the rounding of its argument, nd + 2
    roundings of A = sum_i |b_i| |L_i| on either side: (32 + 2 (nd + 2) A) u S_k"""
    nd = sl.ndim
    tg, og, sg, wg = _call(sl, params, True, dev)
    t0, o0, s0, w0 = _call(sl, params, False, dev)
    assert _same(tg[:, 0], t0) and _same(og, o0)
    assert torch.equal(sg, s0) and torch.equal(wg, w0)
    tg, sg = tg.cpu().numpy(), sg.cpu().numpy()
    found = 0
    worst = 0.0
    for j, p in enumerate(params):
        with np.errstate(all='ignore'):
            xid = sl.find_simplex(sl.map_params(np.asarray(p, dtype=np.float64)))
        if xid < 0:
            assert sg[j] == 0x7fffffff and np.isnan(tg[j]).all()
            assert np.isnan(og[j].item())
            continue
        found += 1
        assert sg[j] == xid
        t, jac = ttruth.template_jacobian(sl, p)
        T = sl.transform[xid, :nd, :]
        s = np.array([1.0 / (p[k] * np.log(10.0)) if k in sl.log_ids else 1.0
                      for k in range(nd)])
        db = np.vstack([T * s[None, :], -(T * s[None, :]).sum(axis=0)[None, :]])
        Lr = np.abs(sl.dats[sl.simplices[xid], :])
        bj = sl._bary(sl.map_params(np.asarray(p, dtype=np.float64)), xid)
        A = (np.abs(bj)[:, None] * Lr).sum(axis=0) if sl.exp else 0.0
        for k in range(nd):
            S = (np.abs(db[:, k])[:, None] * Lr).sum(axis=0) * (t if sl.exp else 1.0)
            err = np.abs(tg[j, 1 + k] - jac[k])
            frac = err / ((32 + 2 * (nd + 2) * A) * 1.1e-16 * S)
            worst = max(worst, float(frac.max()))
            assert (frac <= 1).all(), (j, k, float(frac.max()))
    print('ntp %d exp %d log %s: largest error %.3g of its bound'
          % (sl.dats.shape[1], sl.exp, sl.log_ids, worst))
    assert found == nfound


@pytest.mark.parametrize('ntp', [1, 255, 257])
@pytest.mark.parametrize('exp_flag,log_ids', [(1, ()), (1, (0, )), (0, ()), (0, (0, ))])
def test_two_triangles(setup, ntp, exp_flag, log_ids):
    """a square split into two triangles; ntp below, just below and just above the 256
    threads of a block; with and without exp; with and without a log-mapped parameter"""
    rng = np.random.default_rng(100 * ntp + 10 * exp_flag + len(log_ids))
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    sl = _SynthLib(pts, [[0, 1, 2], [1, 3, 2]],
                   0.5 * rng.standard_normal((4, ntp)) - 2.0,
                   np.array([0.0, 0.0, 0.0, 1.0]), log_ids, exp_flag)
    q = np.array([[0.2, 0.3], [0.6, 0.1], [0.7, 0.8], [0.45, 0.9], [0.31, 0.32],
                  [1.5, 0.5], [0.5, -0.2]])       # mapped; the last two outside
    params = q.copy()
    if 0 in log_ids:
        params[:, 0] = 10.0**q[:, 0]
    _check_synthetic(sl, params, setup['dev'], nfound=5)


def test_six_dimensions(setup):
    """one simplex in six dimensions (the most the kernel takes), two log-mapped
    parameters, ntp = 300"""
    rng = np.random.default_rng(6)
    nd = 6
    pts = np.vstack([np.full(nd, 0.1), 0.1 + np.diag(rng.uniform(0.5, 2.0, nd))])
    pts += 0.05 * rng.standard_normal(pts.shape)
    sl = _SynthLib(pts, [list(range(nd + 1))], 0.5 * rng.standard_normal((7, 300)) - 2.0,
                   rng.integers(0, 2, 7).astype(np.float64), (0, 3), 1)
    b = rng.dirichlet(np.ones(nd + 1), size=3)
    q = np.vstack([b @ pts, pts.mean(axis=0)[None, :] + 5.0])    # the last one outside
    params = q.copy()
    for i in sl.log_ids:
        params[:, i] = 10.0**q[:, i]
    _check_synthetic(sl, params, setup['dev'], nfound=3)


# ---- 3. the gradient against the truth ----------------------------------------------
def _grad_jobs(su, npoly, vsini_grad=False, order=None):
    from rvspecfit_amd import spec_fit
    sel = torch.tensor(list(range(J)) if order is None else order, device=su['dev'])
    return spec_fit.chisq_grad_jobs(su['batch'], su['idx'][sel], su['vel'][sel],
                                    su['par'][sel], su['vs'][sel], dict(npoly=npoly),
                                    su['cfg'], vsini_grad=vsini_grad)


def _rel_err(got, g):
    scale = np.maximum(np.abs(g), 1e-6 * np.abs(g).max())
    return np.abs(got - g) / scale


@pytest.mark.parametrize('npoly', NPOLY)
def test_gradient_against_the_truth(cases, setup, olibs, npoly):
    """chisq_grad_jobs on all jobs and get_chisq_grad on the batch (spectra 0, 1, 2 at
    jobs 0, 1, 2): the in-simplex jobs within REL_ERR_BOUND of the truth relative to
    max(|g_k|, 1e-6 |g|_inf); the value is chisq_jobs', to 1e-11 max(|value|, 1e3); the
    jobs without a simplex: 1000 badchi per arm, no gradient"""
    from rvspecfit_amd import spec_fit
    su = setup
    opt = dict(npoly=npoly)
    want = ttruth.truth_jobs(cases, olibs, npoly)
    chi, grad, st = _grad_jobs(su, npoly)
    ref, rst = spec_fit.chisq_jobs(su['batch'], su['idx'], su['vel'], su['par'],
                                   su['vs'], opt, su['cfg'])
    assert chi.shape == (J, ) and grad.shape == (J, 1 + ND)
    g_all = grad.cpu().numpy()
    worst = 0.0
    for j in range(J):
        a, b = chi[j].item(), ref[j].item()
        print('npoly %d job %d value %.12g chisq_jobs %.12g truth %.12g'
              % (npoly, j, a, b, want[j][0]))
        assert abs(a - b) < 1e-11 * max(abs(b), 1e3), (j, a, b)
    for j in ttruth.INSIDE:
        val, g = want[j]
        assert int(st[j].item()) == 0
        assert abs(chi[j].item() - val) <= 1e-7 * abs(val)
        rel = _rel_err(g_all[j], g)
        for k in range(1 + ND):
            print('npoly %d job %d comp %d truth %.12g got %.12g rel err %.3g'
                  % (npoly, j, k, g[k], g_all[j, k], rel[k]))
        worst = max(worst, float(rel.max()))
    for j in (ttruth.NO_SIMPLEX, ttruth.NONFINITE):
        assert chi[j].item() == 2 * 1000.0 * su['batch'].badchi == want[j][0]
        assert not g_all[j].any()
    cb, gb = spec_fit.get_chisq_grad(su['batch'], su['vel'][:3], su['par'][:3],
                                     options=opt, config=su['cfg'])
    assert cb.shape == (3, ) and gb.shape == (3, 1 + ND)
    gb = gb.cpu().numpy()
    for s in range(3):
        val, g = want[s]
        assert abs(cb[s].item() - val) <= 1e-7 * abs(val)
        rel = _rel_err(gb[s], g)
        print('npoly %d get_chisq_grad spectrum %d largest rel err %.3g'
              % (npoly, s, rel.max()))
        worst = max(worst, float(rel.max()))
    print('npoly %d largest relative error %.3g (bound %.3g)'
          % (npoly, worst, REL_ERR_BOUND))
    assert worst <= REL_ERR_BOUND


def test_single_spectrum_form(setup):
    """get_chisq_grad of one spectrum: (float, ndarray), the numbers of the batch and
    of the job forms; the broadened job through rot_params"""
    from rvspecfit_amd import spec_fit
    su = setup
    opt = dict(npoly=10)
    chi, grad, st = _grad_jobs(su, 10)
    cb, gb = spec_fit.get_chisq_grad(su['batch'], su['vel'][:3], su['par'][:3],
                                     options=opt, config=su['cfg'])
    for s in range(3):
        _, vel, par, _ = ttruth.JOBS[s]
        c1, g1 = spec_fit.get_chisq_grad(su['sds'][s], vel, par, options=opt,
                                         config=su['cfg'])
        assert isinstance(c1, float) and g1.shape == (1 + ND, )
        assert c1 == cb[s].item() and (g1 == gb[s].cpu().numpy()).all()
    j = ttruth.BROADENED
    s, vel, par, vs = ttruth.JOBS[j]
    c3, g3 = spec_fit.get_chisq_grad(su['sds'][s], vel, par, (vs, ), options=opt,
                                     config=su['cfg'])
    assert c3 == chi[j].item() and (g3 == grad[j].cpu().numpy()).all()


def test_vsini_component(cases, setup, olibs):
    """vsini_grad=True: the first 1 + ndim components are the bits of the call without
    it; on the broadened job all six agree with the truth; the vsini component of an
    unbroadened in-simplex job is exactly 0"""
    from rvspecfit_amd import engine
    su = setup
    npoly = 10
    chi, grad, st = _grad_jobs(su, npoly, vsini_grad=True)
    chi0, grad0, st0 = _grad_jobs(su, npoly)
    assert grad.shape == (J, 2 + ND) and grad0.shape == (J, 1 + ND)
    assert torch.equal(grad[:, :1 + ND], grad0) and torch.equal(chi, chi0)
    assert torch.equal(st, st0)
    j = ttruth.BROADENED
    s, vel, par, vs = ttruth.JOBS[j]
    sds = ttruth.spectra(cases, orc.SpecData)[s]
    val, g = ttruth.chisq_and_grad(sds, olibs, vel, par, vs, npoly=npoly,
                                   vsini_grad=True)
    rel = _rel_err(grad[j].cpu().numpy(), g)
    for k in range(2 + ND):
        print('broadened job comp %d truth %.12g got %.12g rel err %.3g'
              % (k, g[k], grad[j, k].item(), rel[k]))
    assert g[1 + ND] != 0 and rel.max() <= REL_ERR_BOUND
    assert grad[0, 1 + ND].item() == 0.0
    # the rows of build_templates: the vsini row is last, the others are unchanged
    lib = su['libs']['gold_b']
    c1, o1, t1 = engine.build_templates(lib, su['par'], su['vs'], return_templ=True,
                                        tangents=True, vsini_tangent=True)
    c0, o0, t0 = engine.build_templates(lib, su['par'], su['vs'], return_templ=True,
                                        tangents=True)
    assert c1.shape == (J, 2 + ND, lib.ntp, 4) and t1.shape == (J, 2 + ND, lib.ntp)
    assert _same(t1[:, :1 + ND], t0) and _same(c1[:, :1 + ND], c0)


def test_determinism(setup):
    """two calls: the same bits; the jobs permuted: the permuted rows, bit for bit"""
    chi, grad, st = _grad_jobs(setup, 10)
    chi2, grad2, st2 = _grad_jobs(setup, 10)
    assert torch.equal(grad, grad2) and torch.equal(chi, chi2)
    perm = [4, 2, 6, 0, 7, 5, 1, 3]
    chi3, grad3, st3 = _grad_jobs(setup, 10, order=perm)
    sel = torch.tensor(perm, device=setup['dev'])
    assert torch.equal(grad3, grad[sel]) and torch.equal(chi3, chi[sel])
    assert torch.equal(st3, st[sel])


def test_chisq_func_grad(setup):
    """vel_fit.chisq_func_grad on the Delaunay setup: the value of chisq_func, the
    gradient of get_chisq_grad(vsini_grad=True) in the optimiser's order, consistent
    with chisq_func0_grad; a Normal prior adds its own term to its component only"""
    from rvspecfit_amd import spec_fit, vel_fit
    from rvspecfit_amd.spec_inter import getSpecParams
    su = setup
    names = list(getSpecParams('gold_b', su['cfg']))
    _, vel, par, _ = ttruth.JOBS[0]
    vs = 30.0

    def func_args(priors=None):
        mapper = vel_fit.ParamMapper(names, dict(zip(names, par)), [],
                                     vel_fit.VSiniMapper(su['cfg']['max_vsini']),
                                     fitVsini=True)
        return dict(specdata=su['sds'][0], paramMapper=mapper, options=dict(npoly=10),
                    config=su['cfg'], priors=priors, min_vel=su['cfg']['min_vel'],
                    max_vel=su['cfg']['max_vel'])
    args = func_args()
    p = np.array([vel, vs] + list(par))
    f, g = vel_fit.chisq_func_grad(p, args)
    ref = vel_fit.chisq_func(p, args)
    assert isinstance(f, float) and g.shape == (2 + ND, )
    assert abs(f - ref) < 1e-11 * max(abs(ref), 1e3), (f, ref)
    _, gp = spec_fit.get_chisq_grad(su['sds'][0], vel, par, (vs, ),
                                    options=args['options'], config=su['cfg'],
                                    vsini_grad=True)
    assert args['paramMapper'].get_fitted_params() == ['vel', 'vsini'] + names
    assert (g == gp[[0, 5, 1, 2, 3, 4]]).all() and g[1] != 0
    f0, g0 = vel_fit.chisq_func0_grad(args['paramMapper'].forward(p), args,
                                      vsini_grad=True)
    assert f0 == f and (g0 == gp).all()
    mu, sig = 5800.0, 150.0
    f1, g1 = vel_fit.chisq_func_grad(p, func_args(priors={'teff': (mu, sig)}))
    it = names.index('teff')
    d = g1 - g
    assert d[2 + it] == pytest.approx(2 * (par[it] - mu) / sig**2, rel=1e-9)
    d[2 + it] = 0
    assert not d.any()
    assert f1 - f == pytest.approx(((par[it] - mu) / sig)**2, rel=1e-9)


def test_mlp_libraries_stay_refused(setup):
    """the scope check still names what it refuses"""
    from rvspecfit_amd import engine

    class NN:
        ndim, kind = 4, 'nn'
    b = setup['batch']
    with pytest.raises(ValueError, match='regular-grid'):
        engine.check_grad_scope(b, {n: NN for n in b.names}, 10)
    engine.check_grad_scope(b, setup['libs'], 10, vsini_grad=True)
