"""The joint fit of a star's epochs, the parts that need no GPU: the arrow
Levenberg-Marquardt machine (tests/refmachines/lm_arrow_restated.py, the statement;
csrc/alm_machine.h through csrc/alm_host.cpp, the product) and the numpy statement of
rvs_epoch_map / rvs_epoch_finish (tests/epochs_truth.py).

1. one step of the restatement against numpy.linalg.solve on the dense d H d + mu I
2. the restated machine on a zero-residual least-squares problem with arrow structure
3. alm_host.cpp against the restatement, bit for bit
4. alm_host.cpp under the sanitizers, as a stand-alone program
5. epochs_truth: a star of one epoch is lm_truth's mapping, rearranged
6. prototypes, exports and the ABI version
"""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import epochs_truth as etruth
import lm_truth
from refmachines import lm_arrow_restated as ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps
SHAPES = [(m, E) for m in (1, 3, 7) for E in (1, 2, 7, 70)]


def _id(s):
    return 'm%d_E%d' % s


# ---- a least-squares problem with arrow structure ------------------------------------
class Bilinear:
    """r_ek = a_ek . theta + b_ek v_e + nl (a_ek . theta) v_e - y_ek, k < m + 3, for N
    stars of E epochs each; y from the truth, so the minimum is 0"""

    def __init__(self, seed, N, m, E, nl=0.1):
        self.nl = nl
        rng = np.random.RandomState(seed)
        self.N, self.m, self.E = N, m, E
        self.a = rng.normal(size=(N, E, m + 3, m))
        self.b = rng.normal(size=(N, E, m + 3)) + 2.0
        self.theta = rng.normal(size=(N, m))
        self.v = rng.normal(size=(N, E))
        self.y = np.stack([self.resid(s, np.concatenate([self.theta[s], self.v[s]]),
                                      0.0)[0] for s in range(N)])
        self.eoff = np.arange(N + 1) * E

    def resid(self, s, z, y):
        m = self.m
        at = self.a[s] @ z[:m]                              # [E, K]
        v = z[m:, None]
        r = at + self.b[s] * v + self.nl * at * v - y
        Jt = self.a[s] * (1 + self.nl * v)[:, :, None]          # [E, K, m]
        Jv = self.b[s] + self.nl * at                           # [E, K]
        return r, Jt, Jv

    def row(self, s, z):
        m, E = self.m, self.E
        r, Jt, Jv = self.resid(s, np.asarray(z, dtype=np.float64), self.y[s])
        out = np.zeros(ref.row_size(m, E))
        out[0] = (r * r).sum()
        out[1:1 + m] = 2 * np.einsum('eki,ek->i', Jt, r)
        H = 2 * np.einsum('eki,ekj->ij', Jt, Jt)
        out[1 + m:1 + m + m * (m + 1) // 2] = H[np.tril_indices(m)]
        rec = out[1 + m + m * (m + 1) // 2:].reshape(E, 2 + m)
        rec[:, 0] = 2 * (Jv * r).sum(axis=1)
        rec[:, 1] = 2 * (Jv * Jv).sum(axis=1)
        rec[:, 2:] = 2 * np.einsum('eki,ek->ei', Jt, Jv)
        return out

    def start(self, seed, scale=0.3):
        rng = np.random.RandomState(seed)
        return np.concatenate([np.concatenate([self.theta[s], self.v[s]]) +
                               scale * rng.normal(size=self.m + self.E)
                               for s in range(self.N)])


def _dense(row, m, E):
    from rvspecfit_amd import alm
    return alm.dense(row, m, E)


# ---- 1. one step against a dense solve --------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_arrow_step_against_dense_solve(shape):
    m, E = shape
    worst = 0.0
    for seed, mu in ((1, 1e-3), (2, 0.7), (3, 1e-9)):
        P = Bilinear(seed, 1, m, E)
        row = P.row(0, P.start(seed + 10))
        g, H = _dense(row, m, E)
        # (positive semi-definite: 2 J^T J)
        assert np.linalg.eigvalsh(H).min() >= -1e-9 * np.abs(H).max()
        ok, d, y = ref.arrow_step(list(row), m, E, mu)
        assert ok
        d, y = np.array(d), np.array(y)
        dh = np.diag(H)
        np.testing.assert_array_equal(d, np.where(dh > 0, 1 / np.sqrt(dh), 1.0))
        A = d[:, None] * H * d[None, :] + mu * np.eye(m + E)
        cond = np.linalg.cond(A)
        yd = np.linalg.solve(A, -d * g)
        err = np.linalg.norm(y - yd) / np.linalg.norm(yd)
        bound = 100 * EPS * cond
        print(_id(shape), 'mu', mu, 'cond', cond, 'step error', err, 'bound', bound)
        assert err <= bound
        worst = max(worst, err / bound)
        # the machine's own trial point and prediction: x0 = 0, so xt is delta
        run = ref.Run(m, np.zeros(m + E), gtol=0.0, tau=mu)
        run.advance()
        run.advance(row)
        assert run.pending
        delta = d * yd
        terms = delta * (mu * delta / d ** 2 - g)
        np.testing.assert_array_equal(np.array(run.xt), d * y)
        assert np.linalg.norm((np.array(run.xt) - delta) / d) <= \
            bound * np.linalg.norm(yd)
        assert abs(run.pred - 0.5 * terms.sum()) <= bound * 0.5 * np.abs(terms).sum()
    print(_id(shape), 'worst error / bound', worst)


# ---- 2. the restated machine on a zero-residual problem -----------------------------------
class Line:
    """y(t) = 1 - d exp(-(t - v_e)^2 / (2 w^2)) at 13 points, theta = (d, w), the truth
    (0.6, 1.2, vt): zero residual at the minimum"""
    T = -3.0 + 0.5 * np.arange(13)

    def __init__(self, vt):
        self.vt = np.asarray(vt, dtype=np.float64)
        self.E = len(vt)

    def row(self, z):
        z = np.asarray(z, dtype=np.float64)
        E, m = self.E, 2
        d, w, v = z[0], z[1], z[2:]
        u = self.T[None, :] - v[:, None]
        ut = self.T[None, :] - self.vt[:, None]
        G = np.exp(-u * u / (2 * w * w))
        r = (1 - d * G) - (1 - 0.6 * np.exp(-ut * ut / (2 * 1.2 * 1.2)))
        Jt = np.stack([-G, -d * G * u * u / w ** 3], axis=2)
        Jv = -d * G * u / w ** 2
        out = np.zeros(ref.row_size(m, E))
        out[0] = (r * r).sum()
        out[1:3] = 2 * np.einsum('eki,ek->i', Jt, r)
        out[3:6] = (2 * np.einsum('eki,ekj->ij', Jt, Jt))[np.tril_indices(2)]
        rec = out[6:].reshape(E, 4)
        rec[:, 0] = 2 * (Jv * r).sum(axis=1)
        rec[:, 1] = 2 * (Jv * Jv).sum(axis=1)
        rec[:, 2:] = 2 * np.einsum('eki,ek->ei', Jt, Jv)
        return out


@pytest.mark.parametrize('E', [1, 5])
def test_restated_machine_on_zero_residual_problem(E):
    rng = np.random.RandomState(5 + E)
    N, gtol = 6, 1e-8
    probs = [Line(rng.uniform(-1, 1, size=E)) for _ in range(N)]
    x0 = np.concatenate([np.concatenate([[0.6, 1.2], p.vt]) *
                         (1 + 0.1 * rng.uniform(-1, 1, size=2 + E)) for p in probs])
    eoff = np.arange(N + 1) * E
    r = ref.minimize_lockstep(lambda idx, Z: [probs[s].row(z) for s, z in zip(idx, Z)],
                              2, eoff, x0, gtol=gtol)
    print('E', E, 'nit', r['nit'], 'nfev', r['nfev'], 'status', r['status'], 'fun',
          r['fun'])
    assert (r['status'] == 0).all()
    xo, _ = ref.offsets(2, eoff)
    for s in range(N):
        z = r['x'][xo[s]:xo[s + 1]]
        g, _ = _dense(probs[s].row(z), 2, E)
        assert np.abs(g).max() <= gtol
        assert np.abs(z - np.concatenate([[0.6, 1.2], probs[s].vt])).max() < 1e-6


# ---- 3. the C++ machine against the restatement -----------------------------------------
def _cases():
    """name -> (m, eoff, func(idx, Z) -> rows or a factory of one with state, x0,
    options)"""
    out = {}
    for m, E in SHAPES:
        N = 3 if E < 70 else 2
        P = Bilinear(100 + 10 * m + E, N, m, E)

        def rows(idx, Z, P=P):
            return [P.row(s, z) for s, z in zip(idx, Z)]
        out['plain_' + _id((m, E))] = (m, P.eoff, rows, P.start(7), {})
    # ragged: stars of 1, 2, 5 and 70 epochs in one call, m = 3
    Ps = [Bilinear(200 + E, 1, 3, E) for E in (1, 2, 5, 70)]
    eoff = np.concatenate([[0], np.cumsum([p.E for p in Ps])])
    x0 = np.concatenate([p.start(9) for p in Ps])

    def ragged(idx, Z):
        return [Ps[s].row(0, z) for s, z in zip(idx, Z)]
    out['ragged'] = (3, eoff, ragged, x0, {})
    out['maxiter2'] = (3, eoff, ragged, x0, dict(maxiter=2))

    def neg_pivot(idx, Z):      # Htt_00 < 0: the Schur pivot is not positive
        rows = ragged(idx, Z)
        for r in rows:
            r[1 + 3] = -5.0
        return rows
    out['neg_pivot'] = (3, eoff, neg_pivot, x0, dict(maxiter=30))

    def neg_h(idx, Z):          # h_0 < 0: a_0 <= 0 until mu exceeds it
        rows = ragged(idx, Z)
        for r in rows:
            r[1 + 3 + 6 + 1] = -0.25
        return rows
    out['neg_epoch_curvature'] = (3, eoff, neg_h, x0, dict(maxiter=30))

    def bad_first(idx, Z):
        rows = ragged(idx, Z)
        for s, r in zip(idx, rows):
            if s == 1:
                r[:] = 0.0
                r[0] = 1e30
            if s == 2:
                r[4] = np.nan
        return rows
    out['bad_first_row'] = (3, eoff, bad_first, x0, {})

    def wall():                 # every star's first trial row is not finite
        seen = {}

        def func(idx, Z):
            rows = ragged(idx, Z)
            for s, r in zip(idx, rows):
                seen[s] = seen.get(s, 0) + 1
                if seen[s] == 2:
                    r[:] = np.inf
            return rows
        return func
    out['nonfinite_trial'] = (3, eoff, wall, x0, {})

    # a strongly non-linear problem from a far start with next to no damping: trials
    # that increase the value
    Pn = Bilinear(300, 4, 3, 5, nl=1.5)
    out['rejected'] = (3, Pn.eoff, lambda idx, Z: [Pn.row(s, z) for s, z in zip(idx, Z)],
                       Pn.start(11, 2.0), dict(tau=1e-9, maxiter=40))

    def flat(idx, Z):           # the value never falls: mu runs beyond mu_max
        rows = ragged(idx, Z)
        for r in rows:
            r[0] = 3.0
        return rows
    out['mu_max'] = (3, eoff, flat, x0, dict(mu_max=1e6))
    return out


CASES = _cases()
STATEFUL = ('nonfinite_trial', )


def _func(name, func):
    return func() if name in STATEFUL else func


@pytest.fixture(scope='module')
def restated():
    out = {}
    with np.errstate(all='ignore'):
        for name, (m, eoff, func, x0, opt) in CASES.items():
            out[name] = ref.minimize_lockstep(_func(name, func), m, eoff, x0,
                                              max_stars=2, **opt)
    return out


def test_cases_take_the_paths_they_are_named_for(restated):
    for name, r in restated.items():
        print(name, 'status', r['status'], 'nit', r['nit'], 'nfev', r['nfev'], 'nrej',
              r['nrej'])
    assert all((restated[k]['status'] == 0).all() for k in restated if
               k.startswith('plain_'))
    assert restated['rejected']['nrej'].sum() >= 1
    assert (restated['ragged']['status'] == 0).all()
    assert (restated['maxiter2']['status'] == 1).all()
    assert (restated['maxiter2']['nit'] == 2).all()
    assert (restated['neg_pivot']['nrej'] >= 1).all()
    assert (restated['neg_epoch_curvature']['nrej'] >= 1).all()
    b = restated['bad_first_row']
    assert list(b['status'][1:3]) == [2, 2] and list(b['nfev'][1:3]) == [1, 1]
    assert b['status'][0] == 0 and b['status'][3] == 0
    assert (restated['nonfinite_trial']['nrej'] >= 1).all()
    assert (restated['nonfinite_trial']['status'] == 0).all()
    assert (restated['mu_max']['status'] == 2).all()
    assert (restated['mu_max']['mu'] > 1e6).all() and (restated['mu_max']['nit'] == 0).all()


@pytest.mark.parametrize('name', list(CASES))
def test_native_equals_restatement(name, restated):
    from rvspecfit_amd import alm
    m, eoff, func, x0, opt = CASES[name]
    a = restated[name]
    func = _func(name, func)

    def rows(idx, X, xoff):
        return np.concatenate(func(idx, [X[xoff[q]:xoff[q + 1]]
                                         for q in range(len(idx))]))
    with np.errstate(all='ignore'):
        b = alm.minimize_lockstep_native(rows, m, eoff, x0, max_stars=2, **opt)
    print(name, 'nit', a['nit'], b['nit'], 'nfev', a['nfev'], b['nfev'], 'status',
          a['status'], b['status'])
    for k in ('nit', 'nfev', 'status'):
        assert np.array_equal(a[k], b[k]), k
    assert a['rounds'] == b['rounds']
    for k in ('x', 'fun', 'grad', 'row', 'mu'):
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def test_native_arguments():
    from rvspecfit_amd import alm
    f = lambda idx, X, xoff: np.zeros(1)  # noqa: E731
    with pytest.raises(ValueError, match='m <= 7'):
        alm.minimize_lockstep_native(f, 8, [0, 1], np.zeros(9))
    with pytest.raises(ValueError, match='at least one epoch'):
        alm.minimize_lockstep_native(f, 2, [0, 1, 1], np.zeros(5))
    with pytest.raises(ValueError, match='entries'):
        alm.minimize_lockstep_native(f, 2, [0, 1, 3], np.zeros(6))
    with pytest.raises(ValueError, match='values'):
        alm.minimize_lockstep_native(f, 2, [0, 1, 3], np.ones(7))
    assert alm.row_size(3, 5) == ref.row_size(3, 5) == etruth.row_size(3, 5) == 35


# ---- 4. under the sanitizers --------------------------------------------------------
def test_native_under_sanitizers(tmp_path):
    """csrc/alm_host.cpp built for the host with -fsanitize=address,undefined inside a
    stand-alone program (tests/epochs_sanitizer_main.cpp includes it) that drives 200
    seeded runs through rvs_alm_begin ... rvs_alm_end: no report, the runs end where
    they should"""
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = str(tmp_path / 'epochs_san')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
           '-fno-omit-frame-pointer', '-ffp-contract=off',
           '-I' + os.path.join(REPO, 'include'), '-o', exe,
           os.path.join(REPO, 'tests', 'epochs_sanitizer_main.cpp')]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.returncode, out.stdout[-500:], out.stderr[-2000:])
    assert out.stdout.count('converged') == 5 and 'nan_first_row' in out.stdout
    assert 'ERROR' not in out.stderr and 'runtime error' not in out.stderr


# ---- 5. the numpy statement of the kernels ----------------------------------------------
FINISH = {
    # name: (m, src [ndim = 4] in theta's columns, vsini_col, priors)
    'm5': (5, [1, 2, 3, 4], 0, True),
    'm2_two_fixed_one_prior': (2, [-1, 0, -1, 1], -1, True),
    'm4_vsini_last': (4, [0, -1, 1, 2], 3, True),
    'm3_no_prior': (3, [0, 1, 2], -1, False),
}


def finish_inputs(name, eoff, seed=41):
    """seeded inputs of rvs_epoch_finish for stars of the given epochs: lm_truth's rows
    (its vsini kinds and prior pattern) as the epochs, the theta of a star from the
    first of them"""
    m, src, vcol, prior = FINISH[name]
    ndim = len(src)
    eoff = np.asarray(eoff)
    N, S = len(eoff) - 1, int(eoff[-1])
    srcX = [c + 1 if c >= 0 else -1 for c in src]
    fisher, X, isig = lm_truth.seeded_rows(seed, S, m + 1, srcX,
                                           vcol + 1 if vcol >= 0 else -1, prior=prior)
    K = fisher.shape[1]
    rng = np.random.RandomState(seed + 1)
    d = dict(chi=rng.normal(size=S) * 1e3, grad=rng.normal(size=(S, K)) * 10,
             fisher=fisher, theta=np.ascontiguousarray(X[eoff[:-1], 1:]),
             params=rng.normal(size=(N, ndim)), extra=np.abs(rng.normal(size=N)),
             bad=np.zeros(N, dtype=np.int32),
             star_id=rng.permutation(N).astype(np.int32),
             job_status=np.zeros(S, dtype=np.int32), X=X, srcX=srcX)
    if prior:
        d['prior_isig'] = np.ascontiguousarray(isig[:N])
        d['prior_mean'] = rng.normal(size=(N, ndim))
    else:
        d['prior_isig'] = d['prior_mean'] = None
    return d


@pytest.mark.parametrize('name', list(FINISH))
def test_one_epoch_is_the_single_spectrum_mapping(name):
    m, src, vcol, prior = FINISH[name]
    N = 37
    eoff = np.arange(N + 1)
    d = finish_inputs(name, eoff)
    F = etruth.epoch_finish(d['chi'], d['grad'], d['fisher'], d['theta'], d['params'],
                            d['extra'], d['bad'], d['star_id'], eoff, src, vcol,
                            d['prior_mean'], d['prior_isig'], 500.0)
    w = etruth.row_size(m, 1)
    assert F.shape == (N * w, )
    isig_rows = None if not prior else d['prior_isig'][d['star_id']]
    H = lm_truth.hess_from_fisher(d['fisher'], d['X'], d['srcX'],
                                  vcol + 1 if vcol >= 0 else -1, isig_rows, 500.0)
    from rvspecfit_amd import alm
    for n in range(N):
        f, gt, Htt, gv, h, c = alm.unpack_row(F[n * w:(n + 1) * w], m, 1)
        assert f == d['chi'][n] + d['extra'][n]
        np.testing.assert_array_equal(Htt, H[n, 1:, 1:])
        assert h[0] == H[n, 0, 0] and gv[0] == d['grad'][n, 0]
        np.testing.assert_array_equal(c[0], H[n, 1:, 0])
    if vcol >= 0:
        x = d['theta'][:, vcol]
        for kind in (x < 0, x == 0, (0 < x) & (x < 500), x > 500):
            assert kind.any()


def test_truth_sums_in_epoch_order_and_counts_the_prior_once():
    name = 'm5'
    m, src, vcol, prior = FINISH[name]
    eoff = np.array([0, 1, 3, 8, 78])
    d = finish_inputs(name, eoff)
    d['bad'][1] = 1
    F = etruth.epoch_finish(d['chi'], d['grad'], d['fisher'], d['theta'], d['params'],
                            d['extra'], d['bad'], d['star_id'], eoff, src, vcol,
                            d['prior_mean'], d['prior_isig'], 500.0)
    ro = etruth.row_offsets(m, eoff)
    assert F.shape == (ro[-1], ) and ro[-1] == sum(etruth.row_size(m, e)
                                                  for e in (1, 2, 5, 70))
    bad = F[ro[1]:ro[2]]
    assert bad[0] == 1e30 and not bad[1:].any()
    s = d['chi'][8]
    for e in range(9, 78):
        s = s + d['chi'][e]
    assert F[ro[3]] == s + d['extra'][3]
    # the prior's curvature appears once on the diagonal of Htt, whatever E is
    tan = etruth.tangents(m, src, vcol, 5)
    r = d['star_id'][3]
    a = 1                                   # a column with a prior (library parameter 0
    sF = d['fisher'][8].copy()              # has isig = 0 in lm_truth.seeded_rows)
    for e in range(9, 78):
        sF = sF + d['fisher'][e]
    a = [i for i in range(m) if i != vcol and d['prior_isig'][r, tan[i] - 1] != 0][0]
    want = 2.0 * sF[tan[a], tan[a]] + 2.0 * d['prior_isig'][r, tan[a] - 1] ** 2
    assert F[ro[3] + 1 + m + a * (a + 1) // 2 + a] == want


def test_map_truth_counts_penalties_once_per_star():
    rng = np.random.RandomState(3)
    N, m, ndim = 3, 3, 3
    eoff = np.array([0, 5, 6, 9])
    theta = rng.normal(size=(N, m))
    theta[:, 0] = [-4.0, 20.0, 510.0]
    vel = rng.normal(size=9) * 100
    vel[7] = 2000.0
    mean, isig = rng.normal(size=(N, ndim)), np.abs(rng.normal(size=(N, ndim)))
    out = etruth.epoch_map(theta, vel, eoff, [0, 1, 2], [-1, 1, 2], 0,
                           np.full((N, ndim), 0.5), None, np.full((N, ndim), 7.0), mean,
                           isig, -1000.0, 1000.0, 500.0)
    p0 = np.array([0.5, theta[0, 1], theta[0, 2]])
    want = 0.0 + (0.0 - -4.0) * (0.0 - -4.0)
    for i in range(ndim):
        dd = (mean[0, i] - p0[i]) * isig[0, i]
        want = want + dd * dd
    assert out['extra'][0] == want and out['vsini'][0] == 0.0
    assert list(out['bad']) == [0, 0, 1]
    assert (out['vel'][6:] == 0).all() and (out['params'][2] == 7.0).all()
    np.testing.assert_array_equal(out['vel'][:6], vel[:6])
    assert list(out['job_templ']) == [0] * 5 + [1] + [2] * 3


# ---- 6. prototypes ----------------------------------------------------------------------
E_ARG = -1
NEW = ('rvs_epoch_map', 'rvs_epoch_finish', 'rvs_alm_row_size', 'rvs_alm_begin',
       'rvs_alm_pending', 'rvs_alm_feed', 'rvs_alm_result', 'rvs_alm_end',
       'rvs_alm_run_bytes', 'rvs_alm_run')


def _header_prototypes():
    txt = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    txt = re.sub(r'/\*.*?\*/', ' ', txt, flags=re.S)
    out = {}
    for mm in re.finditer(r'\b(void \*|int|int64_t|void)\s*(rvs_\w+)\s*\(([^;{]*?)\)\s*;',
                          txt, flags=re.S):
        args = [a.strip() for a in mm.group(3).split(',')]
        out[mm.group(2)] = (mm.group(1).strip(), [] if args == ['void'] else args)
    return out


def test_new_prototypes_match_ctypes_table():
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
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
    assert _lib.ABI_VERSION == 18 and L.rvs_abi_version() == 18
    assert L.rvs_alm_row_size(3, 5) == 35 and L.rvs_alm_row_size(7, 70) == 666
    assert L.rvs_alm_row_size(8, 1) == 0 and L.rvs_alm_row_size(0, 1) == 0
    assert L.rvs_alm_row_size(3, 0) == 0


def test_new_entry_points_refuse_bad_arguments():
    """no GPU here: a device call that got as far as a launch would fail differently"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    eoff = np.array([0, 2, 3], dtype=np.int32)
    x0 = np.zeros(2 * 3 + 3)
    assert not L.rvs_alm_begin(0, 3, p(eoff), p(x0), 1e-5, 0., 0., 0., 0)
    assert not L.rvs_alm_begin(2, 8, p(eoff), p(x0), 1e-5, 0., 0., 0., 0)
    assert not L.rvs_alm_begin(2, 3, None, p(x0), 1e-5, 0., 0., 0., 0)
    assert not L.rvs_alm_begin(2, 3, p(eoff), None, 1e-5, 0., 0., 0., 0)
    empty = np.array([0, 2, 2], dtype=np.int32)
    assert not L.rvs_alm_begin(2, 3, p(empty), p(x0), 1e-5, 0., 0., 0., 0)
    assert L.rvs_alm_feed(None, p(x0), 2) == E_ARG
    h = ctypes.c_void_p(L.rvs_alm_begin(2, 3, p(eoff), p(x0), 1e-5, 0., 0., 0., 0))
    assert h
    try:
        idx, X = np.zeros(2, dtype=np.int64), np.zeros(9)
        assert L.rvs_alm_pending(h, p(idx), p(X), 8) == -2
        assert L.rvs_alm_pending(h, None, p(X), 9) == -1
        assert L.rvs_alm_pending(h, p(idx), p(X), 9) == 2
        F = np.zeros(ref.row_size(3, 2) + ref.row_size(3, 1))
        assert L.rvs_alm_feed(h, None, 2) == E_ARG and L.rvs_alm_feed(h, p(F), 1) == E_ARG
        x, g, fun, mu = np.zeros(9), np.zeros(9), np.zeros(2), np.zeros(2)
        i32 = [np.zeros(2, dtype=np.int32) for _ in range(3)]
        res = lambda h_, x_=x: L.rvs_alm_result(  # noqa: E731
            h_, p(x_), p(fun), p(g), None, p(mu), p(i32[0]), p(i32[1]), p(i32[2]), None)
        assert res(h) == E_ARG                     # unfinished runs
        assert L.rvs_alm_feed(h, p(F), 2) == 0     # f = 0, g = 0: converged
        assert L.rvs_alm_pending(h, p(idx), p(X), 9) == 0
        assert res(h, None) == E_ARG and res(None) == E_ARG
        assert res(h) == 0
        assert list(i32[1]) == [1, 1] and list(i32[2]) == [0, 0]
    finally:
        L.rvs_alm_end(h)
    a = np.zeros(512)
    i = np.zeros(64, dtype=np.int32)
    i64 = np.zeros(8, dtype=np.int64)
    src = (ctypes.c_int32 * 4)(1, 2, 3, 4)

    def fin(N=2, m=5, ndim=4, ntan=5, src=src, vcol=0, chi=a, F=a, fisher=a, rowoff=i64):
        return L.rvs_epoch_finish(N, m, ndim, ntan, None, 0, p(i), p(rowoff), p(chi),
                                  p(a), p(fisher), p(a), p(a), p(a), p(i), p(i), p(i),
                                  src, vcol, None, None, 500.0, p(F), p(i), None)
    assert fin(N=0) == E_ARG and fin(m=8) == E_ARG and fin(ndim=7) == E_ARG
    assert fin(ntan=4) == E_ARG and fin(chi=None) == E_ARG and fin(F=None) == E_ARG
    assert fin(src=None) == E_ARG and fin(vcol=5) == E_ARG and fin(fisher=None) == E_ARG
    assert fin(rowoff=None) == E_ARG
    assert fin(src=(ctypes.c_int32 * 4)(0, 2, 3, 4)) == E_ARG      # vsini's column
    assert fin(src=(ctypes.c_int32 * 4)(1, 1, 3, 4)) == E_ARG      # one column twice
    assert fin(src=(ctypes.c_int32 * 4)(1, 2, 3, -1)) == E_ARG     # a column without source
    src6 = (ctypes.c_int32 * 6)(1, 2, 3, 4, 5, 6)
    assert fin(m=7, ndim=6, ntan=7, src=src6) == E_ARG             # K = 8: ntan <= 6

    def mp(N=2, S=3, m=5, ndim=4, src=src, vcol=0, theta=a, vsini=a):
        return L.rvs_epoch_map(N, S, m, ndim, p(theta), p(a), p(i), p(i), src, vcol, p(a),
                               None, p(a), None, None, -1000., 1000., 500., p(i), p(i),
                               p(a), p(vsini), p(a), p(a), p(i), None)
    assert mp(N=0) == E_ARG and mp(S=1) == E_ARG and mp(m=8) == E_ARG
    assert mp(theta=None) == E_ARG and mp(src=None) == E_ARG and mp(vcol=5) == E_ARG
    assert mp(vsini=None) == E_ARG      # vsini fitted, but no rotation


def test_new_struct_layouts_match_the_header(tmp_path):
    from rvspecfit_amd import _lib
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    pairs = [('rvs_epoch_chain', _lib.EpochChain), ('rvs_alm_state', _lib.AlmState)]
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


def test_alm_run_refuses_bad_arguments():
    """no GPU here: a call that got as far as a launch would fail differently"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    b, c = _lib.AlmState(), _lib.EpochChain()
    ad = ctypes.addressof
    assert L.rvs_alm_run(None, ad(c), None, None) == E_ARG
    assert L.rvs_alm_run(ad(b), None, None, None) == E_ARG
    assert L.rvs_alm_run(ad(b), ad(c), None, None) == E_ARG
    b.N, b.m, c.m = 2, 7, 7                      # the device chain takes m <= 6
    assert L.rvs_alm_run(ad(b), ad(c), None, None) == E_ARG
    assert 0 < L.rvs_alm_run_bytes() < 256       # a run: pointers and scalars
