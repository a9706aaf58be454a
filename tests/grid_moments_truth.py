"""An exact statement of the tail of the reference's find_best (spec_fit.py:1072-1092
with _quadratic_interp_min, :992-1015), what rvs_grid_moments computes, and the case
list that tests/test_grid_moments_truth_cpu.py and tests/test_grid_moments_gpu.py share.

truth() takes the float64 inputs of ONE group as exact and evaluates everything in
mpmath at DPS digits.  Beside every value a float64 evaluation is held to it returns an
A-PRIORI bound on the error of such an evaluation, derived from the terms themselves
and not from any implementation's results.  With u = 2^-53 (unit roundoff), a_i =
-(c_i - c_min)/2, e_i = exp(a_i), psum = sum e_i, p_i = e_i / psum, d_i = v_i - bv and
t_i = p_i d_i^k:

  e_i     (|a_i| + K_EXP) u e_i + K_TINY 2^-1074
            fl(c_i - c_min) has relative error u, the halving is exact, and exp turns
            an absolute error |a_i| u of its argument into that relative error; K_EXP =
            4: an exp good to two ulps (one ulp is 2 u); K_TINY = 2: a result below
            2^-1022 is rounded to a multiple of 2^-1074, twice where the scaling by
            2^k is a step of its own
  psum    sum of the above + n u psum
            recursive summation of n terms, any order: n u sum|e_i|
  p_i     p_i (err(e_i)/e_i + err(psum)/psum + 2 u) + (K_TINY + 1) 2^-1074
            the quotient's two relative errors, the division's own rounding (u, stated
            as 2 u), and one more subnormal rounding of the quotient; psum >= 1
            because the minimum is a term of it, so err(e_i) is not amplified
  vertex  d1 = (yb - ya)/(xb - xa) and d2 likewise: 3 u each (two differences, one
            division); a2 = (d2 - d1)/(xc - xa): (err d1 + err d2)/(xc - xa) + 3 u |a2|;
            b1 = d1 + a2 (xb - xa): err d1 + err a2 (xb - xa) + 2 u |a2| (xb - xa) +
            u |b1|; q = b1/(2 a2): err b1/|2 a2| + |q| err a2/|a2| + u |q|; bv = xb - q:
            err q + u |bv|
  m_k     sum_i [ err(p_i) |d_i|^k + (2 k + 2) u |t_i| + k p_i |d_i|^(k-1) err(bv) ]
          + n u sum|t_i|
            d_i carries one rounding, k times; k multiplications; 2 u more for a pow()
            good to one ulp in place of the repeated product; the derivative of d^k
            with respect to bv; then the summation.  Relative to sum|t_i|, NOT to the
            result: the third moment of a symmetric posterior cancels to nothing and
            is still checkable
  vel_err   err(m_2)/(2 vel_err) + u vel_err           (square root)
  kurtosis  err(m_4)/vel_err^4 + kurtosis (4 err(vel_err)/vel_err + 4 u)
  skewness  err(m_3)/vel_err^3 + |skewness| (3 err(vel_err)/vel_err + 3 u)
            three, two multiplications of vel_err and the division

all to first order.  `about=` evaluates the moments about a given float64 best_vel
taken as exact (err(bv) = 0): what an implementation that found its best_vel another
way (np.polyfit) is held to.

Measured, and asserted nowhere: how far inside these bounds the float64 numpy
restatement oracle.rvs_oracle.grid_summary lies, as the worst |error| / bound over
every group of launches() (tests/test_grid_moments_truth_cpu.py prints them):

  best_chi 0 (exact)   probs 0.87   vel_err 0.14   kurtosis 0.11   skewness 0.079

(the worst probability is one of 3e-224, 1027 above the minimum: nearly all of its
bound is the rounding of c_i - c_min, which any float64 evaluation shares).  Its
best_vel is np.polyfit's and is not held to the vertex bound: the worst |error| /
bound is 9.3e4, and 1.8e3 against u x (condition number of the scaled Vandermonde
matrix polyfit solves) x (width of the bracket): a least-squares solve on uncentred
velocities of a few hundred km/s with steps down to 0.01 and values near 100, where
the divided differences about the centre point lose nothing.
"""
import functools

import mpmath
import numpy as np

DPS = 60
U = 2.0**-53
TINY = 2.0**-1074
K_EXP = 4.0
K_TINY = 2.0
SWITCH = 1e-10      # spec_fit.py:1081

_ctx = mpmath.MPContext()
_ctx.dps = DPS
mpf = _ctx.mpf
NAN = _ctx.nan


def _f(x):
    """an mpf as the nearest float (bounds, and values for printing)"""
    return float(x)


def _vertex(x, y):
    """exact vertex of the parabola through three points, its float64 bound, and
    whether the reference's assert (spec_fit.py:1014) holds.  (None, 0, False) where
    it is undefined."""
    if not (np.all(np.isfinite(y)) and np.all(np.isfinite(x))):
        return None, 0.0, False
    xa, xb, xc = (mpf(float(_)) for _ in x)
    ya, yb, yc = (mpf(float(_)) for _ in y)
    if xb == xa or xc == xb or xc == xa:
        return None, 0.0, False
    d1, d2 = (yb - ya) / (xb - xa), (yc - yb) / (xc - xb)
    a2 = (d2 - d1) / (xc - xa)
    if a2 == 0:
        return None, 0.0, False
    h = abs(xb - xa)
    b1 = d1 + a2 * (xb - xa)
    q = b1 / (2 * a2)
    bv = xb - q
    e_d1, e_d2 = 3 * U * abs(d1), 3 * U * abs(d2)
    e_a2 = (e_d1 + e_d2) / abs(xc - xa) + 3 * U * abs(a2)
    e_b1 = e_d1 + e_a2 * h + 2 * U * abs(a2) * h + U * abs(b1)
    e_q = e_b1 / abs(2 * a2) + abs(q) * e_a2 / abs(a2) + U * abs(q)
    e_bv = e_q + U * abs(bv)
    return bv, _f(e_bv), bool(xa < bv < xc)


def empty():
    """what rvs_grid_moments defines for a group with nvel < 1"""
    return dict(i1=-1, i2=-1, best_chi=float('inf'), best_vel=NAN, vel_err=NAN,
                kurtosis=NAN, skewness=NAN, psum=mpf(0), probs=[], asserts=False,
                switch_ambiguous=False, empty=True,
                bound=dict(best_vel=0.0, vel_err=0.0, kurtosis=0.0, skewness=0.0,
                           psum=0.0, probs=np.zeros(0), m2=0.0, m3=0.0, m4=0.0))


def truth(vels, chisq, quadratic=True, about=None):
    """vels [nv], chisq [Np, nv] (float64, taken as exact) -> dict of i1, i2, best_chi
    (float64), best_vel, vel_err, kurtosis, skewness, psum, m2, m3, m4, abs3 (= sum
    |t_i| of the third moment) (mpf), probs (list of mpf), asserts (the reference
    would have raised in _quadratic_interp_min), switch_ambiguous (vel_err within its
    bound of 1e-10) and bound (dict of floats; probs an array)."""
    vels = np.ascontiguousarray(vels, dtype=np.float64)
    chisq = np.ascontiguousarray(chisq, dtype=np.float64)
    Np, nv = chisq.shape
    assert vels.shape == (nv, )
    if nv == 0:
        return empty()
    # the reference's own two lines, on its own [nv, Np] layout
    ref = np.ascontiguousarray(chisq.T)
    i1, i2 = (int(_) for _ in np.unravel_index(np.argmin(ref), ref.shape))
    col = chisq[i2]
    cmin = col[i1]
    out = dict(i1=i1, i2=i2, best_chi=float(cmin), asserts=False, empty=False,
               switch_ambiguous=False)
    bound = dict(best_vel=0.0)
    out['bound'] = bound
    # best_vel
    if about is not None:
        bv, e_bv = mpf(float(about)), 0.0
    elif quadratic and 0 < i1 < nv - 1:
        bv, e_bv, inside = _vertex(vels[i1 - 1:i1 + 2], col[i1 - 1:i1 + 2])
        out['asserts'] = not inside
        if bv is None:
            bv = NAN
    else:
        bv, e_bv = mpf(float(vels[i1])), 0.0
    out['best_vel'], bound['best_vel'] = bv, e_bv
    # probs; inf - inf and NaN make every term NaN, as in float64
    if not np.isfinite(cmin):
        out.update(psum=NAN, probs=[NAN] * nv, vel_err=NAN, kurtosis=NAN, skewness=NAN,
                   m2=NAN, m3=NAN, m4=NAN, abs3=NAN)
        bound.update(psum=0.0, probs=np.zeros(nv), vel_err=0.0, kurtosis=0.0,
                     skewness=0.0, m2=0.0, m3=0.0, m4=0.0)
        return out
    cm = mpf(float(cmin))
    e, e_e = [], []
    for c in col:
        if c == np.inf:             # fl(inf - c_min) = inf and exp(-inf) = 0, exactly
            e.append(mpf(0))
            e_e.append(mpf(0))
            continue
        a = -(mpf(float(c)) - cm) / 2
        ei = _ctx.exp(a)
        e.append(ei)
        e_e.append((abs(a) + K_EXP) * U * ei + K_TINY * TINY)
    psum = _ctx.fsum(e)
    e_psum = _ctx.fsum(e_e) + nv * U * psum
    r_psum = e_psum / psum
    p = [ei / psum for ei in e]
    e_p = [pi * (r_psum + 2 * U) + eei / psum + (TINY if eei else 0)
           for pi, eei in zip(p, e_e)]
    out['psum'], out['probs'] = psum, p
    bound['psum'] = _f(e_psum)
    bound['probs'] = np.array([_f(_) for _ in e_p])
    if _ctx.isnan(bv):
        out.update(vel_err=NAN, kurtosis=NAN, skewness=NAN, m2=NAN, m3=NAN, m4=NAN,
                   abs3=NAN)
        bound.update(vel_err=0.0, kurtosis=0.0, skewness=0.0, m2=0.0, m3=0.0, m4=0.0)
        return out
    # moments about bv
    d = [mpf(float(v)) - bv for v in vels]
    ad = {1: [abs(_) for _ in d]}
    for k in (2, 3, 4):
        ad[k] = [x * y for x, y in zip(ad[k - 1], ad[1])]
    # sum |t_i| of every order; orders 2 and 4 have no negative term
    sabs = {k: _ctx.fsum(pi * x for pi, x in zip(p, ad[k])) for k in (1, 2, 3, 4)}
    m = {2: sabs[2], 4: sabs[4],
         3: _ctx.fsum(pi * x if di > 0 else -(pi * x)
                      for pi, x, di in zip(p, ad[3], d))}
    e_m = {}
    for k in (2, 3, 4):
        e_m[k] = _ctx.fsum(epi * x for epi, x in zip(e_p, ad[k])) \
            + k * e_bv * sabs[k - 1] + ((2 * k + 2) * U + nv * U) * sabs[k]
        out['m%d' % k], bound['m%d' % k] = m[k], _f(e_m[k])
    out['abs3'] = sabs[3]
    err = _ctx.sqrt(m[2])
    e_err = (e_m[2] / (2 * err) + U * err) if err > 0 else _ctx.sqrt(e_m[2])
    out['vel_err'], bound['vel_err'] = err, _f(e_err)
    out['switch_ambiguous'] = bool(abs(err - mpf(SWITCH)) <= e_err)
    if err < mpf(SWITCH):
        out['kurtosis'] = out['skewness'] = mpf(0)
        bound['kurtosis'] = bound['skewness'] = 0.0
    else:
        kur, skw = m[4] / err**4, m[3] / err**3
        out['kurtosis'], out['skewness'] = kur, skw
        bound['kurtosis'] = _f(e_m[4] / err**4 + kur * (4 * e_err / err + 4 * U))
        bound['skewness'] = _f(e_m[3] / err**3 + abs(skw) * (3 * e_err / err + 3 * U))
    return out


def ratio(got, want, bound):
    """|got - want| / bound in exact arithmetic on the float64 `got`; 0 where both
    are NaN or equal, inf where only one is NaN or they differ with bound 0"""
    got = float(got)
    wn = _ctx.isnan(want) if isinstance(want, _ctx.mpf) else want != want
    if wn or got != got:
        return 0.0 if (wn and got != got) else float('inf')
    diff = abs(mpf(got) - want)
    if diff == 0:
        return 0.0
    return _f(diff / bound) if bound > 0 else float('inf')


# ---------------------------------------------------------------------------
# the case list: launches of rvs_grid_moments, many groups each
# ---------------------------------------------------------------------------
NVS = [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1000, 4097]
NPS = [1, 2, 3, 7, 76]
# every Nv with one and with three templates, every Np at the lengths around the
# wave and the block, and the corners of the table
PLAIN_SHAPES = sorted(set([(nv, 1) for nv in NVS] + [(nv, 3) for nv in NVS[:-1]] +
                          [(nv, np_) for nv in (2, 3, 65, 257) for np_ in NPS] +
                          [(1, 76), (1000, 7), (4097, 76)]))


def grid(rng, nv, uniform, step=None, lo=None):
    step = float(rng.choice([0.01, 0.5, 5.0])) if step is None else step
    lo = float(rng.uniform(-500, 300)) if lo is None else lo
    if uniform:
        return lo + step * np.arange(nv)
    return lo + np.concatenate([[0.], np.cumsum(rng.uniform(0.5, 1.5, nv - 1) * step)])


def curve(rng, vels, Np, v0, width, best=None, noise=1e-3):
    """chisq [Np, nv] = 100 + offset_p + ((v - v0) / width)^2 + noise: a Gaussian
    posterior of sigma `width` centred on v0 in template `best`"""
    off = rng.uniform(1., 20., Np)
    best = int(rng.randint(Np)) if best is None else best
    off[best] = 0.
    c = 100. + off[:, None] + ((vels[None, :] - v0) / width)**2
    return c + noise * rng.standard_normal(c.shape)


def interior_curve(rng, vels, Np, wsteps):
    """minimum at an interior velocity where there is one"""
    nv = len(vels)
    if nv < 3:
        return curve(rng, vels, Np, vels[0] + 0.3 * (vels[-1] - vels[0]), 1.0)
    k = int(rng.randint(1, nv - 1))
    hl, hr = vels[k] - vels[k - 1], vels[k + 1] - vels[k]
    v0 = vels[k] + float(rng.uniform(-0.3, 0.3)) * min(hl, hr)
    c = curve(rng, vels, Np, v0, wsteps * min(hl, hr),
              noise=1e-3 if wsteps < 2 else 1e-6)
    return c


def _launch(name, family, chisq, vels, quadratic=1, nvel=None, **kw):
    chisq = np.ascontiguousarray(chisq, dtype=np.float64)
    G, Np, Nv = chisq.shape
    vels = np.ascontiguousarray(vels, dtype=np.float64)
    assert vels.shape in ((Nv, ), (G, Nv))
    if nvel is not None:
        nvel = np.ascontiguousarray(nvel, dtype=np.int32)
        assert nvel.shape == (G, ) and nvel.min() >= 0 and nvel.max() <= Nv
    d = dict(name=name, family=family, chisq=chisq, vels=vels, quadratic=int(quadratic),
             nvel=nvel, G=G, Np=Np, Nv=Nv)
    d.update(kw)
    return d


def group_inputs(L, g):
    """(vels [nv], chisq [Np, nv]) of group g: what the kernel may read"""
    nv = L['Nv'] if L['nvel'] is None else int(L['nvel'][g])
    v = L['vels'] if L['vels'].ndim == 1 else L['vels'][g]
    return v[:nv], L['chisq'][g][:, :nv]


_truths = {}


def group_truth(L, g):
    v, c = group_inputs(L, g)
    key = (v.tobytes(), c.tobytes(), c.shape, L['quadratic'])
    if key not in _truths:
        _truths[key] = truth(v, c, L['quadratic'])
    return _truths[key]


def _plain():
    out = []
    for nv, np_ in PLAIN_SHAPES:
        rng = np.random.RandomState(1000 * np_ + nv)
        G = 4 if nv < 255 else 2 if nv < 1000 else 1
        # per-group grids (vel_stride = Nv): uniform and non-uniform alternate
        vels = np.stack([grid(rng, nv, g % 2 == 0) for g in range(G)])
        ws = [3.0, max(0.7, nv / 8.), 0.7, 1.5]
        c = np.stack([interior_curve(rng, vels[g], np_, ws[g]) for g in range(G)])
        out.append(_launch('plain-%dx%d-pergroup-q1' % (nv, np_), 'plain', c, vels, 1))
        # one shared grid (vel_stride = 0), non-uniform, without the parabola
        v1 = grid(rng, nv, False)
        c = np.stack([interior_curve(rng, v1, np_, ws[g]) for g in range(G)])
        out.append(_launch('plain-%dx%d-shared-q0' % (nv, np_), 'plain', c, v1, 0))
    # the two remaining combinations at one shape past the block
    rng = np.random.RandomState(77)
    v1 = grid(rng, 257, True)
    c = np.stack([interior_curve(rng, v1, 3, w) for w in (0.7, 3.0, 30.)])
    out.append(_launch('plain-257x3-shared-q1', 'plain', c, v1, 1))
    vels = np.stack([grid(rng, 257, g == 1) for g in range(3)])
    c = np.stack([interior_curve(rng, vels[g], 3, w) for g, w in enumerate((0.7, 3., 30.))])
    out.append(_launch('plain-257x3-pergroup-q0', 'plain', c, vels, 0))
    return out


def _ends():
    out = []
    for Nv, np_ in ((2, 1), (3, 2), (65, 1), (65, 3), (300, 7)):
        rng = np.random.RandomState(2000 + 10 * Nv + np_)
        vels = np.stack([grid(rng, Nv, g % 2 == 0, step=1.0) for g in range(3)])
        nvel = np.array([Nv, Nv, max(Nv - 2, 1)], dtype=np.int32)
        c = np.empty((3, np_, Nv))
        # minimum at index 0: the curve rises over the whole grid
        c[0] = curve(rng, vels[0], np_, vels[0, 0] - 2.3, 4.0)
        # minimum at nv - 1 = Nv - 1: the curve falls over the whole grid
        c[1] = curve(rng, vels[1], np_, vels[1, -1] + 2.3, 4.0)
        # minimum at nv - 1 < Nv - 1: it goes on falling into the padding
        c[2] = curve(rng, vels[2], np_, vels[2, -1] + 2.3, 4.0)
        want = [0, Nv - 1, int(nvel[2]) - 1]
        out.append(_launch('ends-%dx%d' % (Nv, np_), 'ends', c, vels, 1, nvel,
                           want_i1=want))
    return out


PADS = ('nan', 'low', 'last')


def _nvel():
    out = []
    for Nv, np_ in ((4, 1), (70, 1), (70, 3), (300, 2)):
        rng = np.random.RandomState(3000 + 10 * Nv + np_)
        lens = sorted(set(n for n in (1, 2, 3, 64, 65, 257, Nv - 1, Nv) if n <= Nv))
        G = len(lens)
        vels = np.stack([grid(rng, Nv, g % 2 == 0) for g in range(G)])
        c = np.zeros((G, np_, Nv))
        for g, n in enumerate(lens):
            c[g, :, :n] = interior_curve(rng, vels[g, :n], np_, 2.0)
        for pad in PADS:
            cc, vv = c.copy(), vels.copy()
            for g, n in enumerate(lens):
                if pad == 'nan':
                    cc[g, :, n:], vv[g, n:] = np.nan, np.nan
                elif pad == 'low':
                    cc[g, :, n:], vv[g, n:] = -1e300, vv[g, n - 1]
                else:
                    cc[g, :, n:], vv[g, n:] = cc[g, :, n - 1:n], vv[g, n - 1]
            out.append(_launch('nvel-%dx%d-pad-%s' % (Nv, np_, pad), 'nvel', cc, vv, 1,
                               np.array(lens), pad=pad,
                               same_as='nvel-%dx%d-pad-%s' % (Nv, np_, PADS[0])))
    return out


def _ties():
    """equal minima; with 256 threads, element e = p * nv + i belongs to thread
    e % 256, wave (e % 256) // 64"""
    out = []
    for Nv, np_, pairs in (
            # ((p, i), (p, i)) tied; the expected winner is numpy's
            (600, 3, [((0, 100), (2, 100)), ((1, 100), (2, 100)),       # same velocity
                      ((1, 100), (1, 101)), ((1, 100), (1, 164)),       # same template:
                      ((1, 100), (1, 356)), ((1, 100), (1, 102)),       #  thread/wave/stride
                      ((2, 100), (0, 101)), ((2, 100), (0, 164)),       # later template at
                      ((2, 100), (0, 276)), ((2, 7), (0, 599))]),       #  the earlier velocity
            (4, 3, [((0, 1), (2, 1)), ((1, 1), (1, 2)), ((2, 1), (0, 2)),
                    ((1, 0), (0, 3))]),
            (257, 1, [((0, 3), (0, 4)), ((0, 3), (0, 67)), ((0, 0), (0, 256)),
                      ((0, 128), (0, 255))])):
        rng = np.random.RandomState(4000 + Nv)
        v1 = grid(rng, Nv, True, step=1.0)
        G = len(pairs)
        c = np.stack([curve(rng, v1, np_, v1[Nv // 2] + 0.2, Nv / 6.) for g in range(G)])
        want = []
        for g, (a, b) in enumerate(pairs):
            low = c[g].min() - 0.75
            c[g, a[0], a[1]] = c[g, b[0], b[1]] = low
            want.append(min((a[1], a[0]), (b[1], b[0])))
        out.append(_launch('ties-%dx%d' % (Nv, np_), 'ties', c, v1, 1, want_i=want))
    return out


def _parabola():
    out = []
    for Nv, np_ in ((5, 1), (66, 3), (300, 2)):
        rng = np.random.RandomState(5000 + Nv)
        v1 = grid(rng, Nv, False, step=0.5)
        k = Nv // 2
        names = ['plain', 'plateau2', 'flat3', 'inf_left', 'inf_right', 'inf_both',
                 'plain']
        G = len(names)
        c = np.stack([curve(rng, v1, np_, v1[k] + 0.1, 1.2, best=np_ - 1)
                      for g in range(G)])
        p = np_ - 1
        for g, n in enumerate(names):
            low = c[g].min() - 0.5
            if n == 'plateau2':
                c[g, p, k] = c[g, p, k + 1] = low
            elif n == 'flat3':
                c[g, p, k - 1] = c[g, p, k] = c[g, p, k + 1] = low
            elif n.startswith('inf'):
                c[g, p, k] = low
                if n in ('inf_left', 'inf_both'):
                    c[g, p, k - 1] = np.inf
                if n in ('inf_right', 'inf_both'):
                    c[g, p, k + 1] = np.inf
        out.append(_launch('parabola-%dx%d' % (Nv, np_), 'parabola', c, v1, 1,
                           kinds=names))
    return out


def _moments():
    out = []
    for Nv, np_ in ((65, 1), (257, 2), (1000, 1)):
        rng = np.random.RandomState(6000 + Nv)
        v1 = (np.arange(Nv) - Nv // 2).astype(np.float64)     # exactly symmetric
        x = np.abs(v1)
        half = float(Nv // 2)
        kinds = ['symmetric', 'symmetric_q0', 'sharp', 'span1e3', 'span1.5e3',
                 'span1e6', 'constant', 'inf_away']
        c = np.empty((len(kinds), np_, Nv))
        for g, n in enumerate(kinds):
            c[g] = 50. + rng.uniform(2000., 3000., (np_, 1)) + x[None, :]
            row = c[g, np_ - 1]
            if n.startswith('symmetric'):
                row[:] = 50. + (x / 3.)**2 - 0.25 * np.cos(x)
            elif n == 'sharp':
                row[:] = 50. + 1000. * x**2           # integers: the vertex is exact
            elif n.startswith('span'):
                span = float(n[4:])
                row[:] = 50. + span * (x / half)**2
                if n == 'span1.5e3':
                    # e^-720 is subnormal, e^-750 rounds to 0
                    row[0], row[-1], row[1] = 50. + 1440., 50. + 1500., 50. + 1480.
            elif n == 'constant':
                c[g, :, :] = 50.
            elif n == 'inf_away':
                row[:] = 50. + (x / 4.)**2
                row[[0, 1, Nv // 4, Nv - 1]] = np.inf
        out.append(_launch('moments-%dx%d-q1' % (Nv, np_), 'moments', c, v1, 1,
                           kinds=kinds))
    # the same launch without the parabola: best_vel on the grid point
    L = out[0]
    out.append(_launch('moments-65x1-q0', 'moments', L['chisq'], L['vels'], 0,
                       kinds=L['kinds']))
    return out


def _nan():
    out = []
    for Nv, np_ in ((5, 2), (300, 3), (257, 1)):
        rng = np.random.RandomState(7000 + Nv)
        v1 = grid(rng, Nv, True)
        spots = [[], [(np_ - 1, Nv // 2)], [],
                 [(np_ - 1, Nv - 1), (0, Nv - 2), (np_ - 1, 1)],   # several: waves,
                 [(0, 0)], [(np_ - 1, Nv - 1)], []]                # templates, ends
        if Nv >= 257:
            spots[3] = [(np_ - 1, 200), (0, 70), (np_ - 1, 3 + 64), (0, 3 + 128 + 64)]
        c = np.stack([interior_curve(rng, v1, np_, 2.0) for g in range(len(spots))])
        for g, s in enumerate(spots):
            for (p, i) in s:
                c[g, p, i] = np.nan
        out.append(_launch('nan-%dx%d' % (Nv, np_), 'nan', c, v1, 1,
                           clean=[g for g, s in enumerate(spots) if not s]))
    return out


def _empty():
    out = []
    for Nv, np_ in ((5, 1), (5, 3), (257, 3), (70, 1)):
        rng = np.random.RandomState(8000 + 10 * Nv + np_)
        nvel = np.array([Nv, 0, 3, 0, 0, Nv - 1, 1], dtype=np.int32)
        G = len(nvel)
        vels = np.stack([grid(rng, Nv, True) for g in range(G)])
        c = np.stack([interior_curve(rng, vels[g], np_, 2.0) for g in range(G)])
        for g, n in enumerate(nvel):
            if 3 <= n < Nv:
                c[g, :, :n] = interior_curve(rng, vels[g, :n], np_, 2.0)
        out.append(_launch('empty-%dx%d' % (Nv, np_), 'empty', c, vels, 1, nvel))
    return out


@functools.lru_cache(maxsize=None)
def launches():
    """every launch of every family, in a fixed order"""
    out = []
    for fam in (_plain, _ends, _nvel, _ties, _parabola, _moments, _nan, _empty):
        out.extend(fam())
    names = [L['name'] for L in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_family(family):
    return [L for L in launches() if L['family'] == family]


def by_name(name):
    return [L for L in launches() if L['name'] == name][0]
