"""The inputs of tests/test_objective_grad_shapes_gpu.py without a GPU: every in-cell
case of tests/objective_grad_shapes.py is well conditioned -- the numpy restatement of
the adjoint method stays within 2.6e-12 of the autograd truth, the bounds
test_objective_grad_cpu.py holds at npoly 10 on the golden arms -- and
rvs_objective_grad_ok admits and refuses where the cases say it does.  The cap is a
condition on the INPUTS: a case that misses it gets another window or seed."""
import numpy as np
import pytest
import torch

import chisq_grad_truth as truth
import objective_grad_shapes as shapes

CAP = 2.6e-12


def test_banded_spline_solve_is_the_dense_one(gold_libs):
    """truth.spline_eval with the banded solve (what the cases of ~6000 knots use)
    against the dense inverse at 977 knots: value and gradient by the template row
    within 1e-13"""
    lam = gold_libs['gold_b'].lam
    rng = np.random.default_rng(3)
    t0 = np.exp(gold_libs['gold_b'].dats[7].astype(np.float64))
    x = torch.as_tensor(np.sort(rng.uniform(lam[0], lam[-1], 401)))
    cw = torch.as_tensor(rng.standard_normal(401))
    out = []
    for above in (None, 100):
        t = torch.tensor(t0, requires_grad=True)
        with truth.banded_spline(above):
            m = truth.spline_eval(lam, t, x)
        (m * cw).sum().backward()
        out.append((m.detach().numpy(), t.grad.numpy()))
    assert truth.BANDED_ABOVE is None
    (m0, g0), (m1, g1) = out
    em = np.abs(m1 - m0).max() / np.abs(m0).max()
    eg = np.abs(g1 - g0).max() / np.abs(g0).max()
    print('banded against dense: value %.3g gradient %.3g' % (em, eg))
    assert em <= 1e-13 and eg <= 1e-13


@pytest.mark.parametrize('name', shapes.names())
def test_conditioning_cap(name):
    c = shapes.case(name)
    assert c.in_cell
    worst_g = worst_v = 0.0
    for j, (s, vel, par, vs) in enumerate(c.jobs):
        for n, _ in c.arms:
            assert shapes.cell_margin(shapes.olib(n), par) >= 0.01, (n, par)
        val, g = shapes.truth_job(c, j)
        rv, rg = shapes.restated_job(c, j)
        assert g.shape == rg.shape == (1 + c.ndim + (1 if c.vsini_grad else 0), )
        worst_g = max(worst_g, float(shapes.rel_err(rg, g).max()))
        worst_v = max(worst_v, abs(rv - val) / max(abs(val), 1e3))
    print('%s restatement against the truth: gradient %.3g value %.3g'
          % (name, worst_g, worst_v))
    assert worst_g <= CAP
    assert worst_v <= CAP


def test_admission_boundaries():
    from rvspecfit_amd import _lib
    ok = _lib.lib().rvs_objective_grad_ok
    for vg in (0, 1):
        assert ok(10, 3242, 6485, 4, vg) == 1      # 3 x 6485 x 8 + 8192 <= 160 KB
        assert ok(10, 3242, 6486, 4, vg) == 0
        assert ok(10, 16, 32, 4, vg) == 1
        assert ok(10, 16, 33, 4, vg) == 1
        assert ok(10, 17, 33, 4, vg) == 0          # 2 npix > ntp
        for npoly in range(1, 11):
            for nd in range(1, 5):
                assert ok(npoly, 131, 263, nd, vg) == 1, (npoly, nd)
    # every case of the GPU module is admitted
    for c in shapes.cases():
        for n, npix in c.arms:
            lib = shapes.olib(n)
            assert ok(c.npoly, npix, len(lib.lam), lib.ndim, int(c.vsini_grad)) == 1, c
