"""rvs_objective_grad (csrc/objective_grad.hip) at every shape it admits,
against the float64 autograd truth (tests/chisq_grad_truth.py, vsini_grad_truth.py) and
against the value kernel (engine.objective_fused).  The cases are those of
tests/objective_grad_shapes.py, whose inputs tests/test_objective_grad_shapes_cpu.py
holds to a conditioning cap of 2.6e-12 on the CPU; the bound here is REL_ERR_BOUND of
tests/test_objective_grad_gpu.py (4.72e-11, ten times what the golden shape measured),
DEFECT (5e-10) the line above which nothing is argued away.  No bound comes from what
the kernel measures at a new shape.

Every in-cell case asserts: status 0; the value within 1e-7 |truth|; the gradient within
the bound, relative to max(|g_k|, 1e-6 |g|_inf); status and value (within
1e-11 max(|chi^2|, 1e3)) those of engine.objective_fused.  Every case prints one line.

Largest relative error of the gradient against the truth per group, measured on an
MI355X (the whole module: 58 tests in 4.2 s):
    chunk geometry      3.78e-11  chunk-cut860 job 0, d/dalpha = 0.109 beside 3.27 and
                                  2.30: the contraction sum_n tbar_n t_n g_dn cancels
                                  576-fold there (the chain on the same job: 2.8e-12);
                                  the other eleven cases: 1.5e-13 ... 3.6e-12
    production sizes    2.3e-11   prod-desi job 0, on d/dvsini at R = 0.7 (the chain:
                                  2.4e-13); ntp 6485: 3.5e-12, lib_sdss1: 3.5e-13
    packing             2.06e-11  pack-cut32-kmax13 job 0, on d/dvsini (the chain:
                                  6.6e-13); 2 npix = ntp, ntp - 1: 2.6e-12, 4.7e-13, 3.3e-12
    every P             8.24e-12  p3-cut263 job 0, d/dalpha (cancels 147-fold); the other
                                  thirteen cases <= 6.2e-13
    dimensions          1.19e-12  nd2-vsini
    linear knots        1.05e-12
    mixed arms          9.06e-13
Beside them: the missing vertex 5.4e-14 on d/dvel, the refused rotational kernel
1.16e-11 against the truth without rotation, the node query within the bound of the
chain.  The three figures above 1e-11 sit where the golden shape's largest one sits (a
component near a zero of its own, formed by a sum over the knots that cancels more than
the chain's sum over the pixels); all are under the bound, none was used to set it.

Three in-bounds mutants of the kernel were run once against this module and against
test_objective_grad_gpu.py: the second cross-wave neighbour of chain3 taken from the
wrong lane (caught by chunk-cut860, -cut873, -fine5826, -fine5827, prod-sdss1 and by the
golden shape), the dw bit order fixed at nd = 4 (caught by all six dimension cases
only), half a step added to the linear pix_pos (caught by linear-cut263 only).
"""
import pytest
import torch

import chisq_grad_truth as truth
import objective_grad_shapes as shapes
from test_objective_grad_gpu import REL_ERR_BOUND, DEFECT

pytestmark = pytest.mark.gpu
GROUP_WORST = {}
_registered = set()
_dev = {}


def _device(c):
    """the case on the device: batch, libraries, job tensors"""
    if c.name in _dev:
        return _dev[c.name]
    from rvspecfit_amd import _lib, spec_fit, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    for n, _ in c.arms:
        if n not in _registered:
            spec_inter.register_library(TemplateLibrary(n, shapes.lib_dict(n)),
                                        shapes.ROOT)
            _registered.add(n)
    batch = SpecBatch.from_specdata(shapes.specdata(c, spec_fit.SpecData))
    assert [a.npix for a in batch.arms] == [npix for _, npix in c.arms]
    libs = spec_inter.get_libs(batch.names, shapes.config())
    f64 = dict(dtype=torch.float64, device=batch.device)
    vs = None
    if any(j[3] is not None for j in c.jobs):
        vs = torch.tensor([j[3] or 0.0 for j in c.jobs], **f64)
    d = dict(batch=batch, libs=libs, vs=vs,
             idx=torch.tensor([j[0] for j in c.jobs], dtype=torch.int32,
                              device=batch.device),
             vel=torch.tensor([j[1] for j in c.jobs], **f64),
             par=torch.tensor([list(j[2]) for j in c.jobs], **f64))
    _dev.clear()          # one case's libraries and batch at a time
    _dev[c.name] = d
    return d


def _fused(c, d, order=None):
    from rvspecfit_amd import engine
    sel = torch.arange(len(c.jobs), device=d['vel'].device) if order is None else \
        torch.tensor(order, device=d['vel'].device)
    return engine.objective_grad_fused(
        d['batch'], d['libs'], d['par'][sel].contiguous(),
        None if d['vs'] is None else d['vs'][sel].contiguous(),
        d['vel'][sel].contiguous(), c.npoly, c.rbf, d['idx'][sel].contiguous(),
        c.vsini_grad)


def _value_kernel(c, d):
    from rvspecfit_amd import engine
    return engine.objective_fused(d['batch'], d['libs'], d['par'], d['vs'], d['vel'],
                                  c.npoly, c.rbf, d['idx'])


def _agrees_with_value_kernel(c, d, chi, st):
    ref, rst = _value_kernel(c, d)
    assert torch.equal(st, rst), (st, rst)
    for j in range(len(c.jobs)):
        a, b = chi[j].item(), ref[j].item()
        assert abs(a - b) <= 1e-11 * max(abs(b), 1e3), (c.name, j, a, b)


def _check(name):
    """the four assertions of an in-cell case; one line per case"""
    c = shapes.case(name)
    d = _device(c)
    chi, grad, st = _fused(c, d)
    K = 1 + c.ndim + (1 if c.vsini_grad else 0)
    assert grad.shape == (len(c.jobs), K)
    grad = grad.cpu().numpy()
    worst, at = 0.0, None
    want = [shapes.truth_job(c, j) for j in range(len(c.jobs))]
    for j, (val, g) in enumerate(want):
        e = shapes.rel_err(grad[j], g)
        if e.max() >= worst:
            worst, at = float(e.max()), j
    j = at
    GROUP_WORST[c.group] = max(GROUP_WORST.get(c.group, 0.0), worst)
    print('%s job %d value %.12g truth %.12g largest relative error %.3g '
          '(group %s so far %.3g, bound %.3g)'
          % (name, j, chi[j].item(), want[j][0], worst, c.group,
             GROUP_WORST[c.group], REL_ERR_BOUND))
    for j, (val, g) in enumerate(want):
        assert int(st[j].item()) == 0, (name, j)
        assert abs(chi[j].item() - val) <= 1e-7 * abs(val), (name, j, chi[j].item(), val)
    assert worst <= DEFECT, 'a defect to find, not a bound to set'
    assert worst <= REL_ERR_BOUND
    _agrees_with_value_kernel(c, d, chi, st)


# ---- 1. the groups of the in-cell cases ---------------------------------------------
@pytest.mark.parametrize('name', shapes.names('chunk'))
def test_chunk_geometry(name):
    """one wave; a last chunk of 13 rows and of 1 row; an exact wave fill; 1, 2 and 3
    chunks into wave 1 (the neighbours chain3 reads through sh.edge); wave 7 empty, then
    with one row -- without rotation and at R = 1.6"""
    _check(name)


@pytest.mark.parametrize('name', shapes.names('production'))
def test_production_sizes(name):
    """the three DESI arms as one three-arm batch, the LDS limit ntp = 6485, lib_sdss1:
    npoly 10, vsini fitted, R 0.7 and 9.3 -- all eight waves"""
    _check(name)


@pytest.mark.parametrize('name', shapes.names('packing'))
def test_packing_of_the_third_buffer(name):
    """2 npix = ntp and ntp - 1 (first[] directly behind mbar, ntp even and odd) at
    R = 9.3; kmax = 13 on 32 knots: taps and tap derivatives in 2 kmax + 2 <= ntp, the
    primitives in 2 (kmax + 3) = ntp"""
    _check(name)


@pytest.mark.parametrize('name', shapes.names('every_p'))
def test_every_npoly(name):
    """all ten objective_grad_kernel<P> instances (wave_halve at every NV = P (P + 3) /
    2), and fewer pixels than one wave: npix = npoly, npix = 2"""
    _check(name)


@pytest.mark.parametrize('name', shapes.names('dims'))
def test_lower_dimensional_grids(name):
    """grids of 1, 2 and 3 dimensions (the dw table d 2^nd + v, K = 2 + nd, the source
    columns of armgrad), with and without the vsini column; the second query lies in the
    last cell of every axis"""
    _check(name)


@pytest.mark.parametrize('name', shapes.names('linear'))
def test_linear_knots(name):
    """log_step False: the lin_inv_step branch of pix_pos"""
    _check(name)


@pytest.mark.parametrize('name', shapes.names('mixed'))
def test_mixed_arms(name):
    """32 and 6485 knots as two arms of one spectrum: the dynamic LDS is sized by the
    largest arm, the buffers are carved per arm; R = 1 on the first arm is 6.6 on the
    second"""
    _check(name)


# ---- 2. not in a cell -------------------------------------------------------------------
def _side_case(name, jobs, vsini_grad=False, arms=None, npoly=5):
    arms = arms or [(shapes.cut(263), 131)]
    return shapes.Case(name, 'side', arms, npoly, vsini_grad=vsini_grad, in_cell=False,
                       jobs=jobs, seed=81)


def test_missing_vertex():
    """chisq_grad_truth.HOLE_PARAM on 263 knots: the nearest-neighbour template -- the
    parameter components are exactly 0, the velocity component and the value (with the
    outside penalty) are the truth's"""
    lib = shapes.olib(shapes.cut(263))
    assert shapes.cell_margin(lib, truth.HOLE_PARAM) < 0
    c = _side_case('hole', None)
    c.jobs = [(0, shapes.VEL, truth.HOLE_PARAM, None),
              (1, shapes.VEL, truth.HOLE_PARAM, c.vsini(1.6))]
    d = _device(c)
    chi, grad, st = _fused(c, d)
    grad = grad.cpu().numpy()
    for j in range(2):
        val, g = shapes.truth_job(c, j)
        e = abs(grad[j, 0] - g[0]) / abs(g[0])
        print('hole job %d value %.12g truth %.12g d/dvel %.12g truth %.12g rel err %.3g'
              % (j, chi[j].item(), val, grad[j, 0], g[0], e))
        assert int(st[j].item()) == 0
        assert not grad[j, 1:].any() and not g[1:].any()
        assert abs(chi[j].item() - val) <= 1e-7 * abs(val)
        assert e <= REL_ERR_BOUND
    _agrees_with_value_kernel(c, d, chi, st)


def test_query_on_a_grid_node():
    """logg and feh exactly on a node: the derivative is one-sided there, so the
    comparison is with spec_fit.chisq_grad_jobs on the chain, which searches the cell
    with the same code, not with the truth"""
    from rvspecfit_amd import spec_fit
    lib = shapes.olib(shapes.cut(263))
    par = (6000.0, float(lib.uvecs[1][1]), float(lib.uvecs[2][2]), 0.1)
    c = _side_case('node', [(0, shapes.VEL, par, None), (1, shapes.VEL, par, None)])
    d = _device(c)
    chi, grad, st = _fused(c, d)
    zero = torch.zeros_like(d['vel'])
    cchi, cgrad, cst = spec_fit.chisq_grad_jobs(
        d['batch'], d['idx'].long(), d['vel'], d['par'], zero, dict(npoly=c.npoly),
        shapes.config())
    assert torch.equal(st, cst) and not st.any()
    grad, cgrad = grad.cpu().numpy(), cgrad.cpu().numpy()
    for j in range(2):
        e = shapes.rel_err(grad[j], cgrad[j])
        print('node job %d value %.12g chain %.12g gradient %s chain %s rel err %.3g'
              % (j, chi[j].item(), cchi[j].item(), grad[j], cgrad[j], e.max()))
        assert grad[j, 2] != 0.0 and grad[j, 3] != 0.0
        assert abs(chi[j].item() - cchi[j].item()) <= 1e-11 * max(abs(cchi[j].item()), 1e3)
        assert e.max() <= REL_ERR_BOUND


# ---- 3. refusal and range ---------------------------------------------------------------
def test_refused_rotational_kernel():
    """R = 12.5 on 32 knots: kmax = 14, 2 (kmax + 3) = 34 > ntp.  Status and value are
    objective_fused's and RVS_ST_NONFINITE is set.  The gradient gets the treatment the
    chain (chisq_grad_jobs: vsini_kernel<true>) gives a rotational kernel it refuses: the
    template goes through UNBROADENED and the vsini row is exactly zero -- so the vsini
    component is exactly 0 and the other components are those of the same job without
    rotation, held to the truth at vsini = None.  (The chain itself refuses only beyond
    its own tap limit, so at kmax = 14 it broadens and is no reference here.)"""
    from rvspecfit_amd import _lib
    name = shapes.cut(32)
    c = shapes.Case('refused-kmax14', 'side', [(name, 16)], 5, Rs=(12.5, ),
                    vsini_grad=True, in_cell=False, seed=shapes.REFUSED_SEED)
    d = _device(c)
    chi, grad, st = _fused(c, d)
    grad = grad.cpu().numpy()
    _agrees_with_value_kernel(c, d, chi, st)
    plain = shapes.case('refused-plain')      # (under the conditioning cap)
    assert plain.seed == c.seed and plain.arms == c.arms
    assert [j[:3] for j in plain.jobs] == [j[:3] for j in c.jobs]
    for j in range(len(c.jobs)):
        val, g = shapes.truth_job(plain, j)
        e = shapes.rel_err(grad[j, :5], g)
        print('refused job %d status %d value %.12g truth without rotation %.12g '
              'rel err %.3g d/dvsini %g' % (j, st[j].item(), chi[j].item(), val, e.max(),
                                            grad[j, 5]))
        assert int(st[j].item()) == _lib.ST_NONFINITE
        assert grad[j, 5] == 0.0
        assert abs(chi[j].item() - val) <= 1e-7 * abs(val)
        assert e.max() <= REL_ERR_BOUND


def test_pixels_beyond_the_last_knot():
    """a velocity that puts the last pixels beyond the last knot: RVS_ST_SPLINE_RANGE,
    status and value those of the chain and of objective_fused"""
    from rvspecfit_amd import _lib, spec_fit
    c = _side_case('range', [(0, -400.0, shapes.Q0, None), (1, shapes.VEL, shapes.Q0, None)])
    sd = shapes.spectra(c)[0][0]
    assert sd[1][-1] * shapes.doppler(-400.0) > shapes.olib(c.arms[0][0]).lam[-1]
    d = _device(c)
    chi, grad, st = _fused(c, d)
    zero = torch.zeros_like(d['vel'])
    cchi, cgrad, cst = spec_fit.chisq_grad_jobs(
        d['batch'], d['idx'].long(), d['vel'], d['par'], zero, dict(npoly=c.npoly),
        shapes.config())
    ref, rst = _value_kernel(c, d)
    print('range: status %s chain %s value %s chain %s objective_fused %s gradient %s'
          % (st.tolist(), cst.tolist(), chi.tolist(), cchi.tolist(), ref.tolist(),
             grad[0].tolist()))
    assert int(st[0].item()) & _lib.ST_SPLINE_RANGE and int(st[1].item()) == 0
    assert torch.equal(st, cst) and torch.equal(st, rst)
    a, b, r = chi[0].item(), cchi[0].item(), ref[0].item()
    assert (a == b or (a != a and b != b)) and (a == r or (a != a and r != r))
    assert abs(chi[1].item() - cchi[1].item()) <= 1e-11 * max(abs(cchi[1].item()), 1e3)


# ---- 4. determinism -------------------------------------------------------------------------
@pytest.mark.parametrize('name', shapes.names('chunk') + shapes.names('mixed'))
def test_determinism(name):
    """every thread occupancy of the sweeps, twice and with the job list permuted: the
    same bits"""
    c = shapes.case(name)
    d = _device(c)
    chi, grad, st = _fused(c, d)
    chi2, grad2, st2 = _fused(c, d)
    assert torch.equal(grad, grad2) and torch.equal(chi, chi2) and torch.equal(st, st2)
    perm = [2, 0, 3, 1]
    assert len(c.jobs) == 4
    chi3, grad3, st3 = _fused(c, d, perm)
    sel = torch.tensor(perm, device=grad.device)
    assert torch.equal(grad3, grad[sel]) and torch.equal(chi3, chi[sel])
    assert torch.equal(st3, st[sel])
