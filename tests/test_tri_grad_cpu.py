"""The yardstick of the analytic gradient on Delaunay libraries, pinned on the CPU before
any kernel is held against it: tests/tri_grad_truth.py (torch float64, autograd) against
the oracle's get_chisq on the golden Delaunay libraries -- its value, its gradient
against a Richardson-extrapolated central difference of the oracle's value --, the jobs
the GPU tests share, and the declarations of the two new entry points against their
bindings.

Observed on the CPU (npoly 10, the six in-simplex jobs, five components each):
|truth - Richardson| is at most 0.012 of the bound below (job 4, velocity: 6.2e-10 on
0.0505, i.e. 1.2e-8 of the component; every parameter component is below 1e-4 of its
bound); the vsini component of the broadened job differs by 9.5e-10 under a bound of
6.0e-8; the truth's value is within 2.0e-13 relative of the oracle's get_chisq at
npoly 5, 10 and 16."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import rvs_oracle as orc

import tri_grad_truth as ttruth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def tri_libs():
    return ttruth.oracle_libs()


def test_jobs_are_what_the_gpu_tests_assume(tri_libs):
    """the module constant: at least five in-simplex jobs spread over the three spectra,
    one of them broadened, every barycentric coordinate >= MIN_BARY on both arms and
    extraflags 0 there; one job without a simplex; one with a non-finite mapped
    parameter"""
    inside = ttruth.INSIDE
    assert len(inside) >= 5
    assert {ttruth.JOBS[j][0] for j in inside} == {0, 1, 2}
    assert ttruth.BROADENED in inside and ttruth.JOBS[ttruth.BROADENED][3] > 0
    assert sum(1 for j in inside if ttruth.JOBS[j][3]) >= 1
    for j in inside:
        p = np.array(ttruth.JOBS[j][2])
        for n, lib in tri_libs.items():
            mp = lib.map_params(p)
            xid = lib.find_simplex(mp)
            assert xid >= 0, (j, n)
            b = lib._bary(mp, xid)
            print('job %d %s simplex %d smallest coordinate %.4f' % (j, n, xid, b.min()))
            assert b.min() >= ttruth.MIN_BARY, (j, n, b)
            assert lib.outside_flag(p) == 0.0
    rest = [j for j in range(len(ttruth.JOBS)) if j not in inside]
    assert sorted(rest) == sorted([ttruth.NO_SIMPLEX, ttruth.NONFINITE])
    for n, lib in tri_libs.items():
        with np.errstate(all='ignore'):
            mp = lib.map_params(np.array(ttruth.JOBS[ttruth.NO_SIMPLEX][2]))
            assert np.isfinite(mp).all() and lib.find_simplex(mp) == -1
            mp = lib.map_params(np.array(ttruth.JOBS[ttruth.NONFINITE][2]))
            assert not np.isfinite(mp).all() and lib.find_simplex(mp) == -1


def _oracle_value(sds, libs, config, x, vs, npoly):
    with np.errstate(all='ignore'):
        return orc.get_chisq(sds, float(x[0]), tuple(x[1:]),
                             None if vs is None else (vs, ), options=dict(npoly=npoly),
                             config=config, libs=libs, use_c=True)


@pytest.mark.parametrize('npoly', [5, 10, 16])
def test_truth_value_is_the_oracles(cases, tri_libs, gold_config, npoly):
    """value of the truth == oracle get_chisq on every job (the two penalised ones
    included), to the 1e-7 relative that test_chisq_grad_cpu.py asks on the regular
    grid"""
    sp = ttruth.spectra(cases, orc.SpecData)
    want = ttruth.truth_jobs(cases, tri_libs, npoly)
    for j, (s, vel, par, vs) in enumerate(ttruth.JOBS):
        ref = _oracle_value(sp[s], tri_libs, gold_config, [vel] + list(par), vs, npoly)
        val = want[j][0]
        print('npoly %d job %d truth %.12g oracle %.12g rel %.3g'
              % (npoly, j, val, ref, abs(val - ref) / abs(ref)))
        assert abs(val - ref) <= 1e-7 * abs(ref), (j, val, ref)
    for j in (ttruth.NO_SIMPLEX, ttruth.NONFINITE):
        badchi = 10 * sum(len(sd.lam) for sd in sp[ttruth.JOBS[j][0]])
        assert want[j][0] == 2 * 1000.0 * badchi and not want[j][1].any()


# central-difference steps (h, h/2) per component: km/s, K, dex, dex, dex -- those of
# test_chisq_grad_cpu.py, small against a simplex of the golden triangulation (the jobs
# keep 0.0275 or more, in barycentric units, from every face); the test asserts that
# every stepped point stays in the job's simplex.
STEPS = np.array([0.2, 4.0, 4e-3, 2e-3, 1e-3])


@pytest.mark.parametrize('job', ttruth.INSIDE)
def test_truth_gradient_is_the_oracles_central_difference(cases, tri_libs, gold_config,
                                                          job):
    """D(h) = (f(x+h) - f(x-h)) / 2h and the Richardson combination
    (4 D(h/2) - D(h)) / 3 of the oracle's value; the bound of test_vsini_grad_cpu.py and
    test_chisq_grad_cpu.py: 1e-6 of the component + the value's rounding
    (1e-13 |f| + 1e-10) / (h/2) * 5/3"""
    npoly = 10
    s, vel, par, vs = ttruth.JOBS[job]
    sds = ttruth.spectra(cases, orc.SpecData)[s]
    val, g = ttruth.truth_jobs(cases, tri_libs, npoly)[job]
    lib = tri_libs['gold_b']
    x0 = np.array([vel] + list(par))
    sx0 = lib.find_simplex(lib.map_params(x0[1:]))
    f = lambda x: _oracle_value(sds, tri_libs, gold_config, x, vs, npoly)
    assert abs(f(x0) - val) <= 1e-7 * abs(val)
    for k in range(5):
        d = []
        for h in (STEPS[k], STEPS[k] / 2):
            e = np.zeros(5)
            e[k] = h
            for sg in (1, -1):
                assert lib.find_simplex(lib.map_params((x0 + sg * e)[1:])) == sx0
            d.append((f(x0 + e) - f(x0 - e)) / (2 * h))
        rich = (4 * d[1] - d[0]) / 3
        noise = (1e-13 * abs(val) + 1e-10) / (STEPS[k] / 2) * 5 / 3
        bound = 1e-6 * abs(g[k]) + noise
        print('job %d component %d truth %.12g richardson %.12g diff %.3g bound %.3g '
              '(%.3g of it)' % (job, k, g[k], rich, g[k] - rich, bound,
                                abs(g[k] - rich) / bound))
        assert abs(g[k] - rich) <= bound, (job, k, g[k], rich)


def test_truth_vsini_component_is_its_central_difference(cases, tri_libs):
    """the broadened job with vsini as the last parameter: value and first 1 + ndim
    components are those of the call without it; the vsini component against the
    Richardson central difference of the truth's value in vsini (steps 0.2 and
    0.1 km/s), bound as in test_vsini_grad_cpu.py"""
    npoly = 10
    s, vel, par, vs = ttruth.JOBS[ttruth.BROADENED]
    sds = ttruth.spectra(cases, orc.SpecData)[s]
    val, g = ttruth.chisq_and_grad(sds, tri_libs, vel, par, vs, npoly=npoly,
                                   vsini_grad=True)
    val0, g0 = ttruth.truth_jobs(cases, tri_libs, npoly)[ttruth.BROADENED]
    assert g.shape == (6, )
    assert abs(val - val0) <= 1e-12 * abs(val0)
    assert np.abs(g[:5] - g0).max() <= 1e-12 * np.abs(g0).max()
    h0 = 0.2
    d = []
    for h in (h0, h0 / 2):
        f = [ttruth.chisq_and_grad(sds, tri_libs, vel, par, vs + e, npoly=npoly)[0]
             for e in (h, -h)]
        d.append((f[0] - f[1]) / (2 * h))
    rich = (4 * d[1] - d[0]) / 3
    noise = (1e-13 * abs(val) + 1e-10) / (h0 / 2) * 5 / 3
    print('d/dvsini truth %.12g richardson %.12g diff %.3g bound %.3g'
          % (g[5], rich, g[5] - rich, 1e-6 * abs(g[5]) + noise))
    assert abs(g[5] - rich) <= 1e-6 * abs(g[5]) + noise


def numpy_tangent_rows(lib, p):
    """plain-numpy restatement of the sums of the tangent rows: the table
    db_i/dp_k = T[i][k] s_k (last row minus the column sums), g_k = sum_i db_ik L_i in
    vertex order, tangent k = t g_k; returns (t [ntp], rows [ndim, ntp])"""
    nd = lib.ndim
    mp = lib.map_params(np.asarray(p, dtype=np.float64))
    xid = lib.find_simplex(mp)
    T = lib.transform[xid, :nd, :]
    s = np.array([1.0 / (p[k] * np.log(10.0)) if k in lib.log_ids else 1.0
                  for k in range(nd)])
    db = np.empty((nd + 1, nd))
    db[:nd] = T * s[None, :]
    db[nd] = -db[:nd].sum(axis=0)
    L = lib.dats[lib.simplices[xid], :]
    t = lib.eval(np.asarray(p, dtype=np.float64))
    g = np.zeros((nd, L.shape[1]))
    for i in range(nd + 1):
        g += db[i][:, None] * L[i][None, :]
    return t, t[None, :] * g


def test_numpy_restatement_of_the_tangent_rows(tri_libs):
    """the closed form against autograd, absolute, on both arms and the six in-simplex
    jobs: what float64 leaves of the tangent rows.  Observed: largest |difference|
    5.0e-16 (rows of up to 6e-5 per K and 0.39 per dex), and relative to the row's
    largest entry 4.05e-15 (sum_i db_i = 0: the sums cancel the level of the log-flux
    rows).  The device test starts from 10 x the relative figure."""
    worst_abs = worst_rel = 0.0
    for n, lib in tri_libs.items():
        for j in ttruth.INSIDE:
            p = ttruth.JOBS[j][2]
            t, jac = ttruth.template_jacobian(lib, p)
            t2, rows = numpy_tangent_rows(lib, p)
            assert np.abs(t - t2).max() <= 4e-16 * np.abs(t).max()
            for k in range(lib.ndim):
                ea = np.abs(rows[k] - jac[k]).max()
                er = ea / np.abs(jac[k]).max()
                print('%s job %d dt/dp_%d max %.3g abs err %.3g rel %.3g'
                      % (n, j, k, np.abs(jac[k]).max(), ea, er))
                worst_abs, worst_rel = max(worst_abs, ea), max(worst_rel, er)
    print('largest absolute %.3g, relative to the row maximum %.3g'
          % (worst_abs, worst_rel))
    # ndim + 1 = 5 products and their sums, each rounded to ~1.1e-16 of a term that
    # cancellation leaves <~ 10 x the row's largest entry, on both sides of the
    # comparison: 2 * 5 * 1.1e-16 * 10
    assert worst_rel <= 1.1e-14


def test_header_and_binding_agree():
    """rvs_template_tri_grad / rvs_template_tri_buckets_grad are declared in
    include/rvsgpu.h with the arguments of rvs_template_tri / rvs_template_tri_buckets
    and the kinds the ctypes table gives them, are exported, and refuse bad shapes
    before any launch; the ABI number did not move"""
    from rvspecfit_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
    assert _lib.ABI_VERSION == 18
    txt = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    decl = {}
    for name in ('rvs_template_tri', 'rvs_template_tri_grad',
                 'rvs_template_tri_buckets', 'rvs_template_tri_buckets_grad'):
        m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, txt, flags=re.S)
        assert m, name + ' is not declared'
        decl[name] = [' '.join(a.split()) for a in m.group(1).split(',')]
    for name in ('rvs_template_tri', 'rvs_template_tri_buckets'):
        assert decl[name + '_grad'] == decl[name]
        kinds = []
        for a in decl[name + '_grad']:
            kinds.append(ctypes.c_void_p if '*' in a else
                         {'int': ctypes.c_int, 'uint32_t': ctypes.c_uint32}[a.split()[0]])
        res, args = _lib.SIGNATURES[name + '_grad']
        assert res is ctypes.c_int and args == kinds
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES[name + '_grad']
    L = _lib.lib()
    assert L.rvs_abi_version() == 18
    a = ctypes.c_void_p(64)     # never dereferenced
    f = L.rvs_template_tri_grad
    assert f(a, 10, a, a, a, 5, 7, 0, 1, a, 1, a, a, a, None, None) == -1   # ndim > 6
    assert f(a, 10, a, a, a, 5, 0, 0, 1, a, 1, a, a, a, None, None) == -1   # ndim < 1
    assert f(a, 10, a, a, a, 5, 4, 0, 1, a, 0, a, a, a, None, None) == -1   # B < 1
    assert f(a, 0, a, a, a, 5, 4, 0, 1, a, 1, a, a, a, None, None) == -1    # ntp < 1
    assert f(a, 10, a, a, a, 5, 4, 0, 1, a, 1, a, a, None, None, None) == -1  # simplex
    f = L.rvs_template_tri_buckets_grad
    assert f(a, 10, a, a, a, 5, 4, 0, 1, None, a, 1, a, a, a, None, None) == -1
    bk = _lib.TriBuckets()      # no lists
    assert f(a, 10, a, a, a, 5, 4, 0, 1, ctypes.addressof(bk), a, 1, a, a, a, None,
             None) == -1


def test_scope_check_names_the_library_kind(cases):
    """engine.check_grad_scope takes regular-grid and Delaunay libraries; the kinds
    still refused are refused in the words the regular-grid test pins"""
    from rvspecfit_amd import engine

    class Arm:
        name, G, resol = 'gold_b', 1, None

    class Batch:
        arms = [Arm]

    class Lib:
        ndim = 4

    for kind in ('regulargrid', 'triangulation'):
        Lib.kind = kind
        engine.check_grad_scope(Batch, {'gold_b': Lib}, 10)
        engine.check_grad_scope(Batch, {'gold_b': Lib}, 10, vsini_grad=True)
    Lib.kind = 'nn'
    with pytest.raises(ValueError, match='regular-grid'):
        engine.check_grad_scope(Batch, {'gold_b': Lib}, 10)
    Lib.kind, Lib.ndim = 'triangulation', 6
    with pytest.raises(ValueError, match=r'vsini.*ndim = 6'):
        engine.check_grad_scope(Batch, {'gold_b': Lib}, 10, vsini_grad=True)
