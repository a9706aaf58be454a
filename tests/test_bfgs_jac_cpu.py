"""BFGS on an objective that returns its gradient (jac=True), no GPU: scipy against the
Python restatement (tests/refmachines/bfgs_jac_scipy_restated.py), the restatement
against the C++ machine (csrc/bfgs_machine.h: advance_jac, through rvs_bfgs_*_jac),
the prototypes of the new entry points, and the host driver under sanitizers.

Agreement.  Restatement against scipy: the same statements on the same values, so
x, fun, hess_inv to the bit and nit / nfev / njev / status equal -- what
tests/test_tools_cpu.py::test_lockstep_bfgs_equals_scipy asks of the differenced form.
C++ against the restatement: the C++ dot products are sums in index order, numpy's go
through BLAS, so the two follow each other to rounding, not to the bit; the bounds are
those of test_tools_cpu.py::test_native_bfgs_follows_scipy_restatement (same argument
about the dot products): on smooth objectives equal nit / nfev / status, |dx| < 5e-3,
fun to 1e-9 (relative and absolute); on the long Rosenbrock valley and at the
precision-loss exit, whose end depends on the last bits, the same minimum and exit
with effort within 10 % / 25 %; and every run of those cases whose counters and
status DO equal the restatement's is held to the smooth bounds on x and fun.  njev is
held to what nfev is held to.  hess_inv (which that test does not compare) on the
smooth cases: 1e-6 of its largest entry -- it is a rational function of the same s_k,
y_k; with exact gradients the 1 / 1.5e-8 amplification of the differenced form is absent
and rounding (1e-16) through <= 20 rank-two updates on Hessians of condition <= 1e4
stays below 1e-6.  That argument does not carry to the long cases -- 60 updates along
the Rosenbrock valley, where y_k.s_k nearly cancels, amplify the last bit of x
(|dx| ~ 1e-7) into the inverse Hessian -- so there hess_inv is printed, not bounded."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest
import scipy.optimize as so

from refmachines import bfgs_jac_scipy_restated as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- objectives: fg(i, x) -> (f, g) of run i ---------------------------------
def rosen(i, x):
    return so.rosen(x), so.rosen_der(x)


_Q8 = np.random.RandomState(11).normal(size=(8, 8))
_Q8 = np.linalg.qr(_Q8)[0]
_A8 = _Q8 @ np.diag(np.logspace(0, 4, 8)) @ _Q8.T     # condition 1e4
_A8 = 0.5 * (_A8 + _A8.T)


def quad8(i, x):
    d = x - 0.1 * (i + 1)
    return 0.5 * d @ _A8 @ d, _A8 @ d


def barrier(i, x):
    """0.5 |x + 2|^2 - sum log(1 - x): +inf outside x < 1.  From x0 = -3 the first
    trial step lands outside, dcstep's cubic is nan there and dcsrch's bisection
    safeguard brings the search back inside."""
    if (x >= 1).any():
        return np.inf, np.zeros_like(x)
    return 0.5 * np.sum((x + 2)**2) - np.sum(np.log(1 - x)), (x + 2) + 1 / (1 - x)


def kink(i, x):
    """0.5 |x|^2 + 3 |x_0 + 1|: the slope jumps by 6 at x_0 = -1, where the minimum
    is, so no point near it passes the curvature test.  line_search_wolfe1 shrinks
    its bracket onto the kink and gives up (xtol); the search is then repeated by
    line_search_wolfe2, whose _zoom runs its cubic / quadratic / bisection steps.
    (No function was found on which the fall-back succeeds where dcsrch fails: both
    test the same strong Wolfe conditions.  The fall-back's own exits are covered
    statement by statement all the same -- the runs end through it.)"""
    f = 0.5 * np.sum(x**2) + 3 * abs(x[0] + 1)
    g = x.copy()
    g[0] += 3 * np.sign(x[0] + 1)
    return f, g


def quartic_badgrad(i, x):
    """a gradient with a deliberate error of 1e-3 of the problem's scale (it is the
    gradient at x + 1e-3, so it vanishes 1e-3 beside the minimum of f): close to the
    minimum the slope it promises is not there, the line searches find no decrease
    -- scipy's 'precision loss' (status 2).  The runs that come in along the error
    reach |g| <= gtol first and end with status 0: both exits in one case."""
    w = np.arange(1, len(x) + 1)
    d = x - 0.3
    f = 0.5 * np.sum(d**2 * w) + 0.1 * np.sum(d**4)
    d = d + 1e-3
    return f, d * w + 0.4 * d**3


def quartic1(i, x):
    d = x - 0.7
    return float(d[0]**2 + 0.1 * d[0]**4 + np.cos(d[0])), \
        2 * d + 0.4 * d**3 - np.sin(d)


def _rows(fg):
    def f(idx, X):
        out = np.empty((len(idx), X.shape[1] + 1))
        for r, (i, x) in enumerate(zip(idx, X)):
            v, g = fg(int(i), x)
            out[r, 0] = v
            out[r, 1:] = g
        return out
    return f


def _x0(seed, S, n, scale=2.0, shift=0.0):
    # spread on purpose: the S runs of a case end in different rounds
    rng = np.random.RandomState(seed)
    return rng.normal(size=(S, n)) * scale * np.linspace(0.2, 1.5, S)[:, None] + shift


def _h0(seed, n):
    return np.diag(np.random.RandomState(seed).uniform(0.5, 2, n))


S = 5
CASES = {
    # name: (fg, x0 [S, n], hess_inv0, tier, want)
    'rosen2': (rosen, _x0(1, S, 2), _h0(1, 2), 'long', dict(status=0)),
    'rosen5': (rosen, _x0(2, S, 5), _h0(2, 5), 'long', dict(status=0)),
    'quad8': (quad8, _x0(3, S, 8), _h0(3, 8), 'smooth', dict(status=0)),
    'barrier': (barrier, np.full((S, 3), -3.0) - 0.1 * np.arange(S)[:, None],
                None, 'smooth', dict(status=0)),
    'kink': (kink, np.array([-3.0, 0.5]) - 0.3 * np.arange(S)[:, None],
             10 * np.eye(2), 'long', dict(status=2, wolfe2=True)),
    'precision_loss': (quartic_badgrad, _x0(5, S, 4), _h0(5, 4), 'long',
                       dict(status=(0, 2))),
    'n1': (quartic1, _x0(6, S, 1), _h0(6, 1), 'smooth', dict(status=0)),
}


@pytest.fixture(scope='module')
def restated():
    """the restatement's result of every case, computed once"""
    with np.errstate(all='ignore'):
        return {k: ref.minimize_lockstep_jac(_rows(c[0]), c[1], hess_inv0=c[2],
                                             max_rows=3)
                for k, c in CASES.items()}


@pytest.mark.parametrize('name', list(CASES))
def test_restatement_equals_scipy(name, restated):
    fg, x0, H0, _, want = CASES[name]
    r = restated[name]
    with warnings.catch_warnings(), np.errstate(all='ignore'):
        warnings.simplefilter('ignore')
        for i in range(S):
            opt = {} if H0 is None else dict(hess_inv0=H0)
            q = so.minimize(lambda x: fg(i, x), x0[i], method='BFGS', jac=True,
                            options=opt)
            assert (q.nit, q.nfev, q.njev, q.status) == \
                (r['nit'][i], r['nfev'][i], r['njev'][i], r['status'][i]), i
            np.testing.assert_array_equal(q.x, r['x'][i])
            assert q.fun == r['fun'][i]
            np.testing.assert_array_equal(q.hess_inv, r['hess_inv'][i])
    assert set(r['status']) == set(np.atleast_1d(want['status']))
    if want.get('wolfe2'):
        # line_search_wolfe1 asks for value and slope of every point; only the
        # fall-back's phi() takes a value alone
        assert (r['nfev'] > r['njev']).all()
    assert len(set(r['njev'])) > 1          # the runs end in different rounds


@pytest.mark.parametrize('name', list(CASES))
def test_native_jac_follows_restatement(name, restated):
    from rvspecfit_amd import bfgs
    fg, x0, H0, tier, want = CASES[name]
    a = restated[name]
    with np.errstate(all='ignore'):
        b = bfgs.minimize_lockstep_native(_rows(fg), x0, hess_inv0=H0, max_rows=3,
                                          jac=True)
    print(name, 'nit', a['nit'], b['nit'], 'nfev', a['nfev'], b['nfev'], 'njev',
          a['njev'], b['njev'], 'status', a['status'], b['status'], 'max|dx|',
          np.abs(a['x'] - b['x']).max(), 'max|dfun|',
          np.abs(a['fun'] - b['fun']).max(), 'max|dH|/max|H|',
          [float(np.abs(Ha - Hb).max() / np.abs(Ha).max())
           for Ha, Hb in zip(a['hess_inv'], b['hess_inv'])])
    if tier == 'smooth':
        assert np.array_equal(a['status'], b['status'])
        assert np.array_equal(a['nit'], b['nit'])
        assert np.array_equal(a['nfev'], b['nfev'])
        assert np.array_equal(a['njev'], b['njev'])
        assert np.abs(a['x'] - b['x']).max() < 5e-3
        assert np.allclose(a['fun'], b['fun'], rtol=1e-9, atol=1e-9)
        for Ha, Hb in zip(a['hess_inv'], b['hess_inv']):
            assert np.abs(Ha - Hb).max() <= 1e-6 * np.abs(Ha).max()
        assert a['rounds'] == b['rounds']
    else:
        ok = {2} if want['status'] == 2 else {0, 2}
        assert set(a['status']) <= ok and set(b['status']) <= ok
        if want['status'] == 0:
            assert np.allclose(a['fun'], b['fun'], atol=1e-6)
            assert np.abs(a['x'] - b['x']).max() < 5e-3
            tol = 0.1
        else:
            assert (b['status'] == 2).mean() >= 0.8 * (a['status'] == 2).mean() > 0
            assert abs(a['fun'].mean() - b['fun'].mean()) < 0.02
            tol = 0.25
        for k in ('nfev', 'njev'):
            assert abs(a[k].mean() - b[k].mean()) <= tol * a[k].mean()
        # the runs that took the restatement's path, run by run
        same = np.ones(S, dtype=bool)
        for k in ('nit', 'nfev', 'njev', 'status'):
            same &= a[k] == b[k]
        assert np.abs(a['x'] - b['x'])[same].max(initial=0) < 5e-3
        assert np.allclose(a['fun'][same], b['fun'][same], rtol=1e-9, atol=1e-9)


def test_native_jac_arguments():
    from rvspecfit_amd import bfgs
    with pytest.raises(ValueError):
        bfgs.minimize_lockstep_native(_rows(quad8), np.zeros((2, 17)), jac=True)
    with pytest.raises(ValueError):   # a value-only objective under jac=True
        bfgs.minimize_lockstep_native(lambda idx, X: np.zeros(len(idx)),
                                      np.zeros((2, 3)), jac=True)


# ---- prototypes ----------------------------------------------------------------
E_ARG = -1     # RVS_E_ARG of include/rvsgpu.h
NEW = ('rvs_bfgs_begin_jac', 'rvs_bfgs_feed_jac', 'rvs_bfgs_result_jac',
       'rvs_proc_finish_grad', 'rvs_grad_chain_work_size', 'rvs_bfgs_run_grad')


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


def test_new_entry_points_refuse_bad_arguments():
    import ctypes
    from rvspecfit_amd import _lib
    L = _lib.lib()
    x0 = np.zeros((2, 3))
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)   # noqa: E731
    bad = [(0, 3, p(x0)), (2, 0, p(x0)), (2, 17, p(x0)), (2, 3, None)]
    for S_, n_, x_ in bad:
        assert not L.rvs_bfgs_begin_jac(S_, n_, x_, None, 1e-5, 1e-4, 0.9, 0., 0)
    F = np.zeros((2, 4))
    assert L.rvs_bfgs_feed_jac(None, p(F), 2) == E_ARG
    i32 = [np.zeros(2, dtype=np.int32) for _ in range(4)]
    x, fun = np.zeros((2, 3)), np.zeros(2)
    assert L.rvs_bfgs_result_jac(None, p(x), p(fun), p(i32[0]), p(i32[1]), p(i32[2]),
                                 p(i32[3]), None, None) == E_ARG
    h = ctypes.c_void_p(L.rvs_bfgs_begin_jac(2, 3, p(x0), None, 1e-5, 1e-4, 0.9, 0.,
                                             0))
    assert h
    try:
        idx, X = np.zeros(2, dtype=np.int64), np.zeros((2, 3))
        assert L.rvs_bfgs_pending(h, p(idx), p(X), 1) == -2     # too small a list
        assert L.rvs_bfgs_pending(h, p(idx), p(X), 2) == 2
        assert L.rvs_bfgs_feed(h, p(F), 2) == E_ARG        # the differenced feed
        assert L.rvs_bfgs_feed_jac(h, None, 2) == E_ARG
        assert L.rvs_bfgs_feed_jac(h, p(F), 1) == E_ARG    # [rows, 1 + n], rows = 2
        # unfinished runs, a missing njev
        assert L.rvs_bfgs_result_jac(h, p(x), p(fun), p(i32[0]), p(i32[1]), p(i32[2]),
                                     p(i32[3]), None, None) == E_ARG
        assert L.rvs_bfgs_feed_jac(h, p(F), 2) == 0             # f = 0, g = 0: done
        assert L.rvs_bfgs_pending(h, p(idx), p(X), 2) == 0
        assert L.rvs_bfgs_result_jac(h, p(x), p(fun), p(i32[0]), p(i32[1]), None,
                                     p(i32[3]), None, None) == E_ARG
        assert L.rvs_bfgs_result_jac(h, p(x), p(fun), p(i32[0]), p(i32[1]), p(i32[2]),
                                     p(i32[3]), None, None) == 0
        assert list(i32[1]) == [1, 1] and list(i32[2]) == [1, 1]
    finally:
        L.rvs_bfgs_end(h)
    # a handle of rvs_bfgs_begin does not take (f, g) rows
    h = ctypes.c_void_p(L.rvs_bfgs_begin(2, 3, p(x0), None, 1e-5, 1e-4, 0.9, 0., 0))
    try:
        assert L.rvs_bfgs_feed_jac(h, p(F), 2) == E_ARG
    finally:
        L.rvs_bfgs_end(h)


def test_device_entry_points_refuse_bad_arguments_before_any_launch():
    """no GPU here: a call that got as far as a launch would fail differently"""
    import ctypes
    from rvspecfit_amd import _lib
    L = _lib.lib()
    a = np.zeros(64)
    i = np.zeros(64, dtype=np.int32)
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    src = (ctypes.c_int32 * 4)(2, 3, 4, 5)

    def fin(J=2, n=6, ndim=4, ntan=5, src=src, vcol=1, chi=a, F=a):
        return L.rvs_proc_finish_grad(J, n, ndim, ntan, None, 0, p(chi), p(a), p(a),
                                      p(a), p(a), p(i), p(i), p(i), src, vcol, None,
                                      None, 500.0, p(F), p(i), None)
    assert fin(J=0) == E_ARG and fin(n=9) == E_ARG and fin(ndim=7) == E_ARG
    assert fin(ntan=4) == E_ARG and fin(chi=None) == E_ARG and fin(F=None) == E_ARG
    assert fin(src=None) == E_ARG and fin(vcol=6) == E_ARG
    assert fin(src=(ctypes.c_int32 * 4)(0, 3, 4, 5)) == E_ARG   # the velocity's column
    assert fin(src=(ctypes.c_int32 * 4)(1, 3, 4, 5)) == E_ARG   # the vsini column
    assert fin(src=(ctypes.c_int32 * 4)(2, 3, 4, -1)) == E_ARG  # a column with no source
    ntp = (ctypes.c_int32 * 2)(977, 781)
    assert L.rvs_grad_chain_work_size(0, 2, 5, ntp, 2) == 0
    assert L.rvs_grad_chain_work_size(4, 5, 5, ntp, 2) == 0
    assert L.rvs_grad_chain_work_size(4, 2, 7, ntp, 2) == 0
    assert L.rvs_grad_chain_work_size(4, 2, 5, None, 2) == 0
    assert L.rvs_grad_chain_work_size(4, 2, 5, ntp, 3) == 0
    # templ + templ2 + coef: 48 bytes per template pixel and row
    assert L.rvs_grad_chain_work_size(4, 2, 5, ntp, 2) > 4 * 6 * (977 + 781) * 48
    assert L.rvs_grad_chain_work_size(4, 2, 5, ntp, 0) < \
        L.rvs_grad_chain_work_size(4, 2, 5, ntp, 2)
    b, o, g = _lib.BfgsState(), _lib.NmObjective(), _lib.GradChain()
    ad = ctypes.addressof
    assert L.rvs_bfgs_run_grad(None, ad(o), ad(g), 4, None, None) == E_ARG
    assert L.rvs_bfgs_run_grad(ad(b), None, ad(g), 4, None, None) == E_ARG
    assert L.rvs_bfgs_run_grad(ad(b), ad(o), None, 4, None, None) == E_ARG
    assert L.rvs_bfgs_run_grad(ad(b), ad(o), ad(g), 4, None, None) == E_ARG  # all NULL
    b.S, b.n, o.n = 2, 6, 6
    assert L.rvs_bfgs_run_grad(ad(b), ad(o), ad(g), 0, None, None) == E_ARG


def test_new_struct_layouts_match_the_header(tmp_path):
    """rvs_grad_arm / rvs_grad_chain: the ctypes mirrors have the size and the field
    offsets a C compiler gives the header's structs; the pinned ones keep theirs
    (tests/test_abi.py) and RVS_ABI_VERSION stays 18"""
    import ctypes
    from rvspecfit_amd import _lib
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    pairs = [('rvs_grad_arm', _lib.GradArm), ('rvs_grad_chain', _lib.GradChain)]
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
    assert _lib.ABI_VERSION == 18 and _lib.lib().rvs_abi_version() == 18


def test_native_jac_under_sanitizers(tmp_path):
    """csrc/bfgs_host.cpp built for the host with -fsanitize=address,undefined and
    driven through rvs_bfgs_begin_jac ... rvs_bfgs_end on 200 quadratics by a
    stand-alone program: no report, all runs end"""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'bfgs_jac_san')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
           '-fno-omit-frame-pointer', '-I' + os.path.join(REPO, 'include'), '-o',
           exe, os.path.join(REPO, 'tests', 'bfgs_jac_sanitizer_main.cpp'),
           os.path.join(REPO, 'rvspecfit_amd', 'csrc', 'bfgs_host.cpp')]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    assert 'rounds' in out.stdout and 'ERROR' not in out.stderr
    assert 'runtime error' not in out.stderr
