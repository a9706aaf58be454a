"""The yardstick of the analytic gradient, pinned on the CPU before any kernel is held
against it: tests/chisq_grad_truth.py (torch float64, autograd) against the oracle's
get_chisq -- its value on the golden cases, its gradient against a Richardson-
extrapolated central difference of the oracle's value."""
import numpy as np
import pytest

from conftest import gold_specdata
from oracle import rvs_oracle as orc

import chisq_grad_truth as truth

TAGS = ['c0', 'c1', 'c2', 'c3']


@pytest.mark.parametrize('tag', TAGS)
def test_truth_value_is_the_oracles(cases, gold_libs, gold_config, tag):
    """value of the truth == oracle get_chisq on the golden cases (in-cell, on cell
    faces, broadened, outside the grid, non-finite parameters), to the 1e-7 relative
    that test_oracle_golden.py::test_get_chisq holds the oracle itself to"""
    sds = gold_specdata(cases, tag, orc.SpecData)
    for i in range(7):
        k = '%s/chisq/t%d/' % (tag, i)
        vs = float(cases[k + 'vsini'])
        npoly, rbf = int(cases[k + 'npoly']), bool(cases[k + 'rbf'])
        val, _ = truth.chisq_and_grad(sds, gold_libs, float(cases[k + 'vel']),
                                      cases[k + 'param'], None if np.isnan(vs) else vs,
                                      npoly=npoly, rbf=rbf)
        ref = float(cases[k + 'value'])
        assert abs(val - ref) <= 1e-7 * abs(ref), (i, val, ref)


# central-difference steps (h, h/2) per component: km/s, K, dex, dex, dex.  Small
# against the scales on which the objective bends (a pixel is ~50 km/s, a grid cell
# 1000+ K and 0.13-1 dex) and inside every cell of truth.JOBS (>= 1 % of its width
# from a face: >= 12 K, 0.01, 0.0067, 0.0013 dex)
STEPS = np.array([0.2, 4.0, 4e-3, 2e-3, 1e-3])


@pytest.mark.parametrize('job', truth.INSIDE)
def test_truth_gradient_is_the_oracles_central_difference(cases, gold_libs,
                                                          gold_config, job):
    """D(h) = (f(x+h) - f(x-h)) / 2h has error h^2 f'''/6 + O(h^4): the Richardson
    combination (4 D(h/2) - D(h)) / 3 removes the h^2 term.  What is left: O(h^4)
    (in velocity O(h^3), the spline's third derivative jumps at a knot), below 1e-6
    of the component at these steps, and the rounding of the oracle's value -- its
    SVD solve in the raw basis carries ~1e-13 |f| + 1e-10 -- divided by h/2 and
    amplified 5/3 by the combination."""
    npoly = 10
    s, vel, par, vs = truth.JOBS[job]
    sds = truth.spectra(cases, orc.SpecData)[s]
    val, g = truth.truth_jobs(cases, gold_libs, npoly)[job]

    def f(x):
        return orc.get_chisq(sds, float(x[0]), tuple(x[1:]),
                             None if vs is None else (vs, ), options=dict(npoly=npoly),
                             config=gold_config, libs=gold_libs, use_c=True)
    x0 = np.array([vel] + list(par))
    assert abs(f(x0) - val) <= 1e-7 * abs(val)
    for k in range(5):
        d = []
        for h in (STEPS[k], STEPS[k] / 2):
            e = np.zeros(5)
            e[k] = h
            d.append((f(x0 + e) - f(x0 - e)) / (2 * h))
        rich = (4 * d[1] - d[0]) / 3
        noise = (1e-13 * abs(val) + 1e-10) / (STEPS[k] / 2) * 5 / 3
        print('job %d component %d truth %.12g richardson %.12g diff %.3g bound %.3g'
              % (job, k, g[k], rich, g[k] - rich, 1e-6 * abs(g[k]) + noise))
        assert abs(g[k] - rich) <= 1e-6 * abs(g[k]) + noise, (job, k, g[k], rich)
