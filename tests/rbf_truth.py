"""Independent CPU statement of what rvs_rbf_factor / _solve / _eval compute, and the
inputs of the regularize_grid tests.

The truth: the bordered system of the multiquadric interpolant,

    [ K + diag(s)  1 ] [ c   ]   [ d ]        K[i,j] = -sqrt(eps^2 |y_i - y_j|^2 + 1)
    [ 1^T          0 ] [ lam ] = [ 0 ]

assembled in long double, solved by LAPACK's pivoted LU (float64) and refined with
long-double residuals until the correction stops shrinking; the evaluation
out[m] = sum_j -sqrt(eps^2 |x_m - y_j|^2 + 1) c[j] + lam in long double.  No shifted
matrix, no Cholesky: nothing of the device's route.
"""
import numpy as np
import scipy.linalg

LD = np.longdouble


def _kernel(a, b, eps):
    a, b = np.asarray(a, dtype=LD) * LD(eps), np.asarray(b, dtype=LD) * LD(eps)
    r2 = np.zeros((a.shape[0], b.shape[0]), dtype=LD)
    for k in range(a.shape[1]):
        t = a[:, k][:, None] - b[:, k][None, :]
        r2 += t * t
    return -np.sqrt(r2 + LD(1))


def solve(y, d, smoothing=0.0, eps=1.0, max_steps=8):
    """(c [N, S], lam [S]) in long double, and the sizes of the refinement steps"""
    y = np.asarray(y, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64)
    d = d.reshape(len(y), -1)
    n = len(y)
    A = np.zeros((n + 1, n + 1), dtype=LD)
    A[:n, :n] = _kernel(y, y, eps)
    A[np.arange(n), np.arange(n)] += np.broadcast_to(np.asarray(smoothing, dtype=LD), n)
    A[:n, n] = 1
    A[n, :n] = 1
    rhs = np.zeros((n + 1, d.shape[1]), dtype=LD)
    rhs[:n] = d
    lu = scipy.linalg.lu_factor(A.astype(np.float64))
    sol = scipy.linalg.lu_solve(lu, rhs.astype(np.float64)).astype(LD)
    steps = []
    last = np.inf
    for _ in range(max_steps):
        res = rhs - A @ sol
        cor = scipy.linalg.lu_solve(lu, res.astype(np.float64)).astype(LD)
        size = float(np.abs(cor).max())
        if not size < last:
            break
        sol = sol + cor
        steps.append(size)
        last = size
        if size == 0:
            break
    return sol[:n], sol[n], steps


def evaluate(x, y, c, lam, eps=1.0, chunk=256):
    """out [M, S] in long double"""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((len(x), c.shape[1]), dtype=LD)
    for a in range(0, len(x), chunk):
        out[a:a + chunk] = _kernel(x[a:a + chunk], y, eps) @ c + lam[None, :]
    return out


def interpolate(y, d, x, smoothing=0.0, eps=1.0):
    c, lam, _ = solve(y, d, smoothing, eps)
    return evaluate(x, y, c, lam, eps)


# ---------------------------------------------------------------------------
# The grids of tests/golden/regularize_cases.npz.  Only the reference's outputs are
# stored there; the inputs are made here from the recipe, by rvspecfit_amd.synth.
# ---------------------------------------------------------------------------
CASES = {
    # 16 teff values (4 windows), unevenly spaced; smooth = 0
    'windows': dict(
        axes=([3500., 3600., 3700., 3800., 3900., 4000., 4250., 4500., 4750., 5000.,
               5500., 6000., 6500., 7000., 8000., 10000.],
              [1., 2., 3., 4., 5.], [-2., -1.5, -1., -0.5, 0., 0.5], [0., 0.2, 0.4]),
        seed=11, hole_fraction=0.05, corner=1, smooth=0.,
        options=dict(min_feh=-2., max_feh=0.5, step_feh=.25, min_alpha=-.2,
                     max_alpha=.6, step_alpha=.2)),
    # 8 teff values: one window; smooth > 0
    'single': dict(
        axes=([4000., 4500., 5000., 5500., 6000., 6500., 7000., 8000.],
              [2., 3., 4., 5.], [-2., -1., -0.5, 0.], [0., 0.2, 0.4]),
        seed=12, hole_fraction=0.05, corner=1, smooth=0.01,
        options=dict(min_feh=-2., max_feh=0., step_feh=.5, min_alpha=0.,
                     max_alpha=.4, step_alpha=.2)),
}
LAM = (4500., 4530., 16)        # np.linspace: the pixels of the rows


def holey_vec(axes, seed, hole_fraction, corner):
    """vec [4, T] of a grid with the holes of a real one: alpha != 0 is missing at both
    ends of the feh axis, a random share of single models is missing, and `corner`
    (teff, logg) nodes are cut from the hot, low-gravity corner of the footprint"""
    from rvspecfit_amd import synth
    u, vec = synth.regular_grid(axes=axes)
    teff, logg, feh, alpha = vec
    keep = ~((alpha != 0) & ((feh == u[2][0]) | (feh == u[2][-1])))
    keep &= np.random.default_rng(seed).random(vec.shape[1]) >= hole_fraction
    for k in range(corner):
        keep &= ~((teff == u[0][-1 - k]) & (logg == u[1][0]))
    return vec[:, keep]


def case_inputs(name):
    """(specs_dict as make_interpol.build_specs returns it, with float64 numpy rows;
    the options of regularize) of a golden case"""
    from rvspecfit_amd import synth
    rec = CASES[name]
    vec = holey_vec(rec['axes'], rec['seed'], rec['hole_fraction'], rec['corner'])
    lam = np.linspace(*LAM)
    specs = np.array([np.log(synth.spectrum(lam, *v)) for v in vec.T])
    D = dict(specs=specs, vec=vec, lam=lam,
             parnames=('teff', 'logg', 'feh', 'alpha'),
             mapper_module='rvspecfit.read_grid', mapper_class_name='LogParamMapper',
             mapper_args=((0, ), ), lognorms=np.zeros(vec.shape[1]), log_step=False,
             log_spec=True)
    return D, dict(rec['options'], smooth=rec['smooth'])
