"""Levenberg-Marquardt on (value, gradient, Gauss-Newton matrix) rows, no GPU: the Python
restatement (tests/refmachines/lm_restated.py) against truth, the C++ machine
(csrc/lm_machine.h, through rvs_lm_begin ... rvs_lm_end) against the restatement, the
prototypes of the new entry points, the host driver under sanitizers, and the numpy
statement of rvs_proc_finish_fisher's mapping against a brute-force construction.

Agreement of the C++ machine with the restatement: BIT EQUALITY was reached, on every
case -- x, fun, grad, hess and mu to the bit, nit / nfev / status / rounds equal.  Why it
can be: the restatement is scalar arithmetic on Python floats with explicit loops, the
C++ follows it statement by statement, both sum in index order, sqrt and the division
are correctly rounded on both sides, and the host object is built with
-ffp-contract=off (lm_machine.h also switches contraction off for clang), so a * b + c
rounds twice in both.  The ceiling the issue allowed (equal counters, |dx| < 5e-3, fun
to 1e-9) was not needed.

Objectives return (f, g, H).  Least-squares problems give g = 2 J^T r, H = 2 J^T J."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.optimize as so

from refmachines import bfgs_jac_scipy_restated as bfgs_ref
from refmachines import lm_restated as ref
import lm_truth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- objectives: fgh(i, x) -> (f, g, H) of run i -----------------------------------
def _lsq(r, J):
    return float(r @ r), 2.0 * J.T @ r, 2.0 * J.T @ J


def rosen_res(x):
    """the chained Rosenbrock function as residuals: 10 (x_{i+1} - x_i^2), 1 - x_i"""
    n = len(x)
    r = np.empty(2 * (n - 1))
    J = np.zeros((2 * (n - 1), n))
    for i in range(n - 1):
        r[2 * i] = 10.0 * (x[i + 1] - x[i]**2)
        J[2 * i, i + 1] = 10.0
        J[2 * i, i] = -20.0 * x[i]
        r[2 * i + 1] = 1.0 - x[i]
        J[2 * i + 1, i] = -1.0
    return r, J


def rosen(i, x):
    return _lsq(*rosen_res(x))


_rng = np.random.RandomState(17)
_Q6 = np.linalg.qr(_rng.normal(size=(6, 6)))[0]
_D6 = np.logspace(-3, 3, 6)                       # K beside dex
_A6 = (_Q6 * np.logspace(0, 2, 6)) @ _Q6.T        # cond Lambda = 1e2
_A6 = 0.5 * (_A6 + _A6.T)
_A6 = _D6[:, None] * _A6 * _D6[None, :]
_C6 = 0.1 * np.arange(1, 7)


def illquad(i, x):
    d = x - _C6
    return 0.5 * d @ _A6 @ d, _A6 @ d, _A6


def barrier(i, x):
    """test_bfgs_jac_cpu.barrier: 0.5 |x + 2|^2 - sum log(1 - x), +inf outside x < 1.
    With its exact Hessian 1 + 1 / (1 - x)^2 Newton's step on this convex function never
    leaves the domain, so the matrix handed over is 0.1 of it -- a curvature that
    underestimates, as a Gauss-Newton matrix can: from x0 <= -3 the first trial lands
    beyond x = 1 and is rejected."""
    if (x >= 1).any():
        return np.inf, np.zeros_like(x), np.zeros((len(x), len(x)))
    return (0.5 * np.sum((x + 2)**2) - np.sum(np.log(1 - x)), (x + 2) + 1 / (1 - x),
            0.1 * np.diag(1 + 1 / (1 - x)**2))


BARRIER_MIN = -0.5 * (1 + np.sqrt(13.0))      # (x + 2) (1 - x) = -1, x < 1

_Q4 = np.linalg.qr(np.random.RandomState(5).normal(size=(4, 4)))[0]
_A4 = (_Q4 * np.logspace(0, 2, 4)) @ _Q4.T
_A4 = 0.5 * (_A4 + _A4.T)


def quad_smallH(i, x):
    """H deliberately 0.01 of the true matrix: steps overshoot a hundredfold"""
    d = x - 0.2 * (i + 1)
    return 0.5 * d @ _A4 @ d, _A4 @ d, 0.01 * _A4


def quartic_badgrad(i, x):
    """test_bfgs_jac_cpu.quartic_badgrad: the gradient is the one at x + 1e-3, so it
    vanishes 1e-3 beside the minimum of f; H is the true Hessian.  A run whose Newton
    step lands within gtol of the gradient's zero while f still falls ends with status
    0; one that comes to rest between the two zeros finds no decrease: status 2."""
    w = np.arange(1, len(x) + 1)
    d = x - 0.3
    f = 0.5 * np.sum(d**2 * w) + 0.1 * np.sum(d**4)
    H = np.diag(w + 1.2 * d**2)
    d = d + 1e-3
    return f, d * w + 0.4 * d**3, H


def dead_column(i, x):
    """column 2 has g = 0 and a zero row and column of H: vsini at the clamp"""
    d = x[:2] - np.array([0.5, -1.5])
    A = np.array([[3.0, 1.0], [1.0, 2.0]])
    g, H = np.zeros(3), np.zeros((3, 3))
    g[:2] = A @ d + 0.4 * d**3
    H[:2, :2] = A + np.diag(1.2 * d**2)
    return 0.5 * d @ A @ d + 0.1 * np.sum(d**4), g, H


def quartic1(i, x):
    d = x - 0.7
    return (float(d[0]**2 + 0.1 * d[0]**4 + np.cos(d[0])),
            2 * d + 0.4 * d**3 - np.sin(d), (2 + 1.2 * d**2 - np.cos(d)).reshape(1, 1))


def bad_row(i, x):
    return 1e30, np.zeros_like(x), np.zeros((len(x), len(x)))


def _rows(fgh, trace=None):
    def f(idx, X):
        out = np.empty((len(idx), ref.npack(X.shape[1])))
        for r, (i, x) in enumerate(zip(idx, X)):
            v, g, H = fgh(int(i), x)
            out[r] = np.concatenate([[v], g, H[np.tril_indices(len(x))]])
            if trace is not None:
                trace.append((int(i), float(v)))
        return out
    return f


def _x0(seed, S, n, scale=2.0, shift=0.0):
    # spread on purpose: the S runs of a case end in different rounds
    rng = np.random.RandomState(seed)
    return rng.normal(size=(S, n)) * scale * np.linspace(0.2, 1.5, S)[:, None] + shift


S = 6
CASES = {
    # name: (fgh, x0 [S, n], options)
    # (gtol: the run ends where max |g_i| <= gtol, so |x - 1| <= sqrt(n) gtol / lmin(H);
    # lmin(2 J^T J) at the minimum is 0.4 for n = 2 and 0.5 for the chain, and 1e-8
    # puts the end 1e-7 and better inside the 1e-6 asked of it -- the default 1e-5
    # would allow 3.5e-5)
    'rosen2': (rosen, _x0(1, S, 2), dict(gtol=1e-8)),
    'rosen6': (rosen, _x0(2, S, 6, scale=1.0), dict(gtol=1e-8)),
    'illquad': (illquad, _C6 + _x0(3, S, 6) / _D6, {}),
    'barrier': (barrier, np.full((S, 3), -3.0) - 0.1 * np.arange(S)[:, None], {}),
    'smallH': (quad_smallH, _x0(4, S, 4), {}),
    'badgrad': (quartic_badgrad, _x0(5, 8, 4), {}),
    'dead_column': (dead_column, _x0(6, S, 3), {}),
    'n1': (quartic1, _x0(7, S, 1), {}),
    'bad_first_row': (bad_row, _x0(8, 4, 3), {}),
    'maxiter2': (rosen, _x0(1, S, 2), dict(gtol=1e-8, maxiter=2)),
}


@pytest.fixture(scope='module')
def restated():
    """the restatement's result of every case, computed once; with the trace of
    (run, value) of every row it asked for"""
    out = {}
    with np.errstate(all='ignore'):
        for k, (fgh, x0, opt) in CASES.items():
            trace = []
            out[k] = ref.minimize_lockstep(_rows(fgh, trace), x0, max_rows=3, **opt)
            out[k]['trace'] = trace
    return out


def _start_values(fgh, x0):
    return np.array([fgh(i, x)[0] for i, x in enumerate(x0)])


@pytest.mark.parametrize('name', list(CASES))
def test_every_run_ends_at_or_below_its_start(name, restated):
    fgh, x0, _ = CASES[name]
    r = restated[name]
    assert (r['fun'] <= _start_values(fgh, x0)).all()
    assert (r['nfev'] >= 1).all() and (r['nfev'] >= r['nit'] + 1).all()


@pytest.mark.parametrize('name', ['rosen2', 'rosen6'])
def test_rosenbrock(name, restated):
    fgh, x0, _ = CASES[name]
    r = restated[name]
    print(name, 'nit', r['nit'], 'nfev', r['nfev'], 'status', r['status'])
    assert (r['status'] == 0).all()
    assert np.abs(r['x'] - 1.0).max() < 1e-6
    for i in range(len(x0)):
        q = so.least_squares(lambda x: rosen_res(x)[0], x0[i],
                             jac=lambda x: rosen_res(x)[1], method='lm')
        assert np.abs(q.x - r['x'][i]).max() < 1e-6
    assert len(set(r['nfev'])) > 1          # the runs end in different rounds


def test_ill_scaled_quadratic(restated):
    fgh, x0, _ = CASES['illquad']
    r = restated['illquad']
    with np.errstate(all='ignore'):
        b = bfgs_ref.minimize_lockstep_jac(
            lambda idx, X: _rows(fgh)(idx, X)[:, :7], x0, hess_inv0=None, max_rows=3)
    print('illquad LM rows', r['nfev'], 'BFGS rows', b['nfev'], 'LM fun', r['fun'],
          'BFGS fun', b['fun'], 'BFGS status', b['status'])
    assert (r['status'] == 0).all()
    # at the minimum: |g| <= gtol gives f - 0 <= g^T A^-1 g / 2 <= n gtol^2 / (2 lmin),
    # lmin(A) >= lmin(Lambda) min(D)^2 = 1e-6
    assert (r['fun'] <= 6 * 1e-5**2 / (2 * 1e-6)).all()
    assert np.abs(r['grad']).max() <= 1e-5
    assert r['nfev'].sum() < b['nfev'].sum()


def test_barrier(restated):
    fgh, x0, _ = CASES['barrier']
    r = restated['barrier']
    for i in range(len(x0)):
        vals = [v for s, v in r['trace'] if s == i]
        assert np.isfinite(vals[0]) and vals[1] == np.inf    # the first trial: outside
    assert (r['nrej'] >= 1).all()
    assert (r['mu'] > ref.TAU).all()
    assert (r['status'] == 0).all()
    assert (r['x'] < 1).all()
    # |g| <= gtol with f'' >= 1: within gtol of the analytic minimum
    assert np.abs(r['x'] - BARRIER_MIN).max() <= 1e-5


def test_small_H_rejections(restated):
    r = restated['smallH']
    print('smallH nrej', r['nrej'], 'nit', r['nit'], 'mu', r['mu'])
    assert (r['nrej'] >= 1).all()
    assert (r['status'] == 0).all()
    x_min = 0.2 * (np.arange(len(r['x'])) + 1)[:, None]
    assert np.abs(r['x'] - x_min).max() <= 1e-5      # lmin(A) = 1: |d| <= |g|


def test_bad_gradient_both_exits(restated):
    r = restated['badgrad']
    print('badgrad status', r['status'], 'nit', r['nit'], 'nfev', r['nfev'])
    assert set(r['status']) == {0, 2}
    assert np.abs(r['x'] - 0.3).max() < 2e-3


def test_dead_column(restated):
    fgh, x0, _ = CASES['dead_column']
    r = restated['dead_column']
    assert np.array_equal(r['x'][:, 2], x0[:, 2])         # never moves, to the bit
    assert (r['status'] == 0).all()
    assert np.abs(r['x'][:, :2] - np.array([0.5, -1.5])).max() < 1e-5


def test_n1(restated):
    r = restated['n1']
    assert (r['status'] == 0).all()
    q = so.minimize_scalar(lambda t: quartic1(0, np.array([t]))[0], bracket=(0, 1),
                           tol=1e-12)
    assert np.abs(r['x'][:, 0] - q.x).max() < 1e-5


def test_bad_first_row(restated):
    fgh, x0, _ = CASES['bad_first_row']
    r = restated['bad_first_row']
    assert (r['status'] == 2).all() and (r['nfev'] == 1).all() and (r['nit'] == 0).all()
    assert np.array_equal(r['x'], x0)
    assert r['rounds'] == 1


def test_maxiter(restated):
    r = restated['maxiter2']
    assert (r['status'] == 1).all() and (r['nit'] == 2).all()


# ---- the C++ machine against the restatement ---------------------------------------
@pytest.mark.parametrize('name', list(CASES))
def test_native_equals_restatement(name, restated):
    from rvspecfit_amd import lm
    fgh, x0, opt = CASES[name]
    a = restated[name]
    with np.errstate(all='ignore'):
        b = lm.minimize_lockstep_native(_rows(fgh), x0, max_rows=3, **opt)
    print(name, 'nit', a['nit'], b['nit'], 'nfev', a['nfev'], b['nfev'], 'status',
          a['status'], b['status'], 'max|dx|', np.abs(a['x'] - b['x']).max(),
          'max|dfun|', np.abs(a['fun'] - b['fun']).max())
    for k in ('nit', 'nfev', 'status'):
        assert np.array_equal(a[k], b[k]), k
    assert a['rounds'] == b['rounds']
    for k in ('x', 'fun', 'grad', 'hess', 'mu'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_native_arguments():
    from rvspecfit_amd import lm
    with pytest.raises(ValueError):
        lm.minimize_lockstep_native(_rows(rosen), np.zeros((2, 9)))
    with pytest.raises(ValueError):   # a (f, g) objective
        lm.minimize_lockstep_native(lambda idx, X: np.zeros((len(idx), 4)),
                                    np.ones((2, 3)))


def test_unpack_rows():
    from rvspecfit_amd import lm
    f, g, H = rosen(0, np.array([0.3, -0.2, 1.1]))
    F = lm.pack_row(f, g, H)[None]
    f2, g2, H2 = lm.unpack_rows(F, 3)
    assert f2[0] == f and np.array_equal(g2[0], g) and np.array_equal(H2[0], H)
    assert F.shape[1] == lm.npack(3) == ref.npack(3) == 10


# ---- prototypes --------------------------------------------------------------------
E_ARG = -1     # RVS_E_ARG of include/rvsgpu.h
NEW = ('rvs_proc_finish_fisher', 'rvs_fisher_chain_work_size', 'rvs_lm_begin',
       'rvs_lm_pending', 'rvs_lm_feed', 'rvs_lm_result', 'rvs_lm_end',
       'rvs_lm_run_bytes', 'rvs_lm_run')


def _header_prototypes():
    txt = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    txt = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    out = {}
    for m in re.finditer(r'\b(void \*|int|int64_t|void)\s*(rvs_\w+)\s*\(([^;{]*?)\)\s*;',
                         txt, flags=re.S):
        args = [a.strip() for a in m.group(3).split(',')]
        out[m.group(2)] = (m.group(1).strip(), [] if args == ['void'] else args)
    return out


def test_new_prototypes_match_ctypes_table():
    import ctypes
    from rvspecfit_amd import _lib
    protos = _header_prototypes()
    kind = {ctypes.c_void_p: 'ptr', ctypes.c_int: 'int', ctypes.c_int64: 'int64_t',
            ctypes.c_double: 'double', ctypes.c_uint32: 'uint32_t', None: 'void'}
    L = _lib.lib()
    for name in NEW:
        assert name in protos, name
        assert hasattr(L, name), name
        ret, args = protos[name]
        res, argtypes = _lib.SIGNATURES[name]
        assert kind[res] == ('ptr' if '*' in ret else ret), name
        want = ['ptr' if '*' in a else a.split()[-2] for a in args]
        assert [kind[t] for t in argtypes] == want, name
    assert _lib.ABI_VERSION == 18 and L.rvs_abi_version() == 18
    assert L.rvs_lm_run_bytes() < 1024          # a run's state: well under 1 KB


def test_new_struct_layouts_match_the_header(tmp_path):
    import ctypes
    from rvspecfit_amd import _lib
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    pairs = [('rvs_fisher_chain', _lib.FisherChain), ('rvs_lm_state', _lib.LmState),
             ('rvs_grad_chain', _lib.GradChain)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rvsgpu.h"',
             'int main(void) {']
    for cname, cls in pairs:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f in cls._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));'
                         % (cname, f[0], cname, f[0]))
    lines += ['return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = str(tmp_path / 'layout')
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-I',
                           os.path.join(REPO, 'include'), str(src), '-o', exe])
    got = dict(ln.split() for ln in
               subprocess.check_output([exe]).decode().splitlines())
    for cname, cls in pairs:
        assert int(got[cname]) == ctypes.sizeof(cls), cname
        for f in cls._fields_:
            assert int(got['%s.%s' % (cname, f[0])]) == getattr(cls, f[0]).offset, \
                (cname, f[0])


def test_new_entry_points_refuse_bad_arguments():
    """no GPU here: a device call that got as far as a launch would fail differently"""
    import ctypes
    from rvspecfit_amd import _lib
    L = _lib.lib()
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    x0 = np.zeros((2, 3))
    for S_, n_, x_ in [(0, 3, p(x0)), (2, 0, p(x0)), (2, 9, p(x0)), (2, 3, None)]:
        assert not L.rvs_lm_begin(S_, n_, x_, 1e-5, 0., 0., 0., 0)
    F = np.zeros((2, ref.npack(3)))
    assert L.rvs_lm_feed(None, p(F), 2) == E_ARG
    h = ctypes.c_void_p(L.rvs_lm_begin(2, 3, p(x0), 1e-5, 0., 0., 0., 0))
    assert h
    x, g, fun, mu = np.zeros((2, 3)), np.zeros((2, 3)), np.zeros(2), np.zeros(2)
    i32 = [np.zeros(2, dtype=np.int32) for _ in range(3)]
    res = lambda h_, x_=x: L.rvs_lm_result(  # noqa: E731
        h_, p(x_), p(fun), p(g), None, p(mu), p(i32[0]), p(i32[1]), p(i32[2]), None)
    try:
        idx, X = np.zeros(2, dtype=np.int64), np.zeros((2, 3))
        assert L.rvs_lm_pending(h, p(idx), p(X), 1) == -2
        assert L.rvs_lm_pending(h, None, p(X), 2) == -1
        assert L.rvs_lm_pending(h, p(idx), p(X), 2) == 2
        assert L.rvs_lm_feed(h, None, 2) == E_ARG
        assert L.rvs_lm_feed(h, p(F), 1) == E_ARG
        assert res(h) == E_ARG                     # unfinished runs
        assert L.rvs_lm_feed(h, p(F), 2) == 0      # f = 0, g = 0: converged
        assert L.rvs_lm_pending(h, p(idx), p(X), 2) == 0
        assert res(h, None) == E_ARG and res(None) == E_ARG
        assert res(h) == 0
        assert list(i32[1]) == [1, 1] and list(i32[2]) == [0, 0]
    finally:
        L.rvs_lm_end(h)
    a = np.zeros(256)
    i = np.zeros(64, dtype=np.int32)
    src = (ctypes.c_int32 * 4)(2, 3, 4, 5)

    def fin(J=2, n=6, ndim=4, ntan=5, src=src, vcol=1, chi=a, F=a, fisher=a):
        return L.rvs_proc_finish_fisher(J, n, ndim, ntan, None, 0, p(chi), p(a),
                                        p(fisher), p(a), p(a), p(a), p(i), p(i), p(i),
                                        src, vcol, None, None, 500.0, p(F), p(i), None)
    assert fin(J=0) == E_ARG and fin(n=9) == E_ARG and fin(ndim=7) == E_ARG
    assert fin(ntan=4) == E_ARG and fin(chi=None) == E_ARG and fin(F=None) == E_ARG
    assert fin(src=None) == E_ARG and fin(vcol=6) == E_ARG and fin(fisher=None) == E_ARG
    assert fin(src=(ctypes.c_int32 * 4)(0, 3, 4, 5)) == E_ARG
    assert fin(src=(ctypes.c_int32 * 4)(1, 3, 4, 5)) == E_ARG
    assert fin(src=(ctypes.c_int32 * 4)(2, 3, 4, -1)) == E_ARG
    ntp = (ctypes.c_int32 * 2)(977, 781)
    assert L.rvs_fisher_chain_work_size(0, 2, 5, ntp, 2) == 0
    assert L.rvs_fisher_chain_work_size(4, 2, 7, ntp, 2) == 0
    assert L.rvs_fisher_chain_work_size(4, 2, 5, None, 2) == 0
    extra = L.rvs_fisher_chain_work_size(4, 2, 5, ntp, 2) - \
        L.rvs_grad_chain_work_size(4, 2, 5, ntp, 2)
    assert extra == L.rvs_chisq_point_fisher_work_size(4, 2, 5) + 4 * 36 * 8
    b, o, g, fc = _lib.LmState(), _lib.NmObjective(), _lib.GradChain(), \
        _lib.FisherChain()
    ad = ctypes.addressof
    assert L.rvs_lm_run(None, ad(o), ad(g), ad(fc), 4, None, None) == E_ARG
    assert L.rvs_lm_run(ad(b), None, ad(g), ad(fc), 4, None, None) == E_ARG
    assert L.rvs_lm_run(ad(b), ad(o), None, ad(fc), 4, None, None) == E_ARG
    assert L.rvs_lm_run(ad(b), ad(o), ad(g), None, 4, None, None) == E_ARG
    assert L.rvs_lm_run(ad(b), ad(o), ad(g), ad(fc), 4, None, None) == E_ARG
    b.S, b.n, o.n = 2, 6, 6
    assert L.rvs_lm_run(ad(b), ad(o), ad(g), ad(fc), 0, None, None) == E_ARG


def test_native_under_sanitizers(tmp_path):
    """csrc/lm_host.cpp built for the host with -fsanitize=address,undefined and driven
    through rvs_lm_begin ... rvs_lm_end by a stand-alone program on the Rosenbrock
    residuals and the log barrier: no report, the runs end where they should"""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'lm_san')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
           '-fno-omit-frame-pointer', '-ffp-contract=off',
           '-I' + os.path.join(REPO, 'include'), '-o', exe,
           os.path.join(REPO, 'tests', 'lm_sanitizer_main.cpp'),
           os.path.join(REPO, 'rvspecfit_amd', 'csrc', 'lm_host.cpp')]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    assert 'rosenbrock' in out.stdout and 'barrier' in out.stdout
    assert 'ERROR' not in out.stderr and 'runtime error' not in out.stderr


# ---- the mapping Fisher matrix -> H ------------------------------------------------
MAPPINGS = {
    # name: (n, src, vsini_col)
    'n6': (6, [2, 3, 4, 5], 1),
    'n3_two_fixed': (3, [-1, 1, -1, 2], -1),
    'n1': (1, [-1, -1, -1, -1], -1),
    'n4_vsini_last': (4, [1, -1, 2, -1], 3),
}


@pytest.mark.parametrize('name', list(MAPPINGS))
def test_mapping_statement_equals_brute_force(name):
    n, src, vcol = MAPPINGS[name]
    fisher, X, isig = lm_truth.seeded_rows(23, 37, n, src, vcol)
    a = lm_truth.hess_from_fisher(fisher, X, src, vcol, isig, 500.0)
    b = lm_truth.hess_brute(fisher, X, src, vcol, isig, 500.0)
    np.testing.assert_array_equal(a, b)
    assert np.array_equal(a, a.transpose(0, 2, 1))
    if vcol >= 0:
        x = X[:, vcol]
        clamped = ~((0 < x) & (x < 500.0))
        assert clamped.any() and (~clamped).any()
        off = np.delete(a[:, vcol, :], vcol, axis=1)
        assert (off[clamped] == 0).all() and (off[~clamped] != 0).all()
        assert (a[(x < 0) | (x > 500.0), vcol, vcol] == 2.0).all()
        assert (a[(x == 0) | (x == 500.0), vcol, vcol] == 0.0).all()
    # without priors and inside the clamp: a plain selection of 2 F
    c = lm_truth.hess_from_fisher(fisher, np.full_like(X, 1.0), src, vcol, None, 500.0)
    keep = lm_truth.tangents(n, src, vcol, fisher.shape[1] - 1)
    np.testing.assert_array_equal(c, 2.0 * fisher[:, keep][:, :, keep])
