"""rvs_epoch_map and rvs_epoch_finish (csrc/epochs.hip) stated in numpy, scalar by scalar
in the kernels' order, so that the kernels (built without FMA contraction) give the same
bits.

  theta [N, m]       the stars' shared parameters, columns [vsini,] free stellar parameters
  vel [S]            one velocity per epoch; star n owns the epochs eoff[n] .. eoff[n+1]-1
  src [ndim]         column of THETA of library parameter i, or -1 where it is fixed
  vsini_col          column of theta of vsini, or -1
  chi [S], grad [S, K], fisher [S, K, K]   K = 1 + ntan, ordered (vel, library parameters,
                     vsini last), in the 0.5 chi^2 convention
  tables             fixed, safe, prior_mean, prior_isig [., ndim], vsini_fixed [.]: rows
                     list[n]
A star's row: f, g_theta [m], Htt packed lower triangle, then per epoch (g_e, h_e, c_e).
"""
import numpy as np


def row_size(m, E):
    return 1 + m + m * (m + 1) // 2 + E * (2 + m)


def row_offsets(m, eoff):
    eoff = np.asarray(eoff, dtype=np.int64)
    k = np.arange(len(eoff), dtype=np.int64)
    return k * (1 + m + m * (m + 1) // 2) + eoff * (2 + m)


def tangents(m, src, vsini_col, ntan):
    """column of theta -> row of the gradient / Fisher matrix"""
    tan = [0] * m
    for i, c in enumerate(src):
        if c >= 0:
            tan[c] = 1 + i
    if vsini_col >= 0:
        tan[vsini_col] = ntan
    return tan


def epoch_map(theta, vel, eoff, lst, src, vsini_col, fixed, vsini_fixed, safe,
              prior_mean, prior_isig, min_vel, max_vel, max_vsini, has_vsini=True):
    theta = np.asarray(theta, dtype=np.float64)
    N, ndim = theta.shape[0], len(src)
    S = len(vel)
    out = dict(star_id=np.zeros(N, dtype=np.int32), job_templ=np.zeros(S, dtype=np.int32),
               vel=np.zeros(S), vsini=np.zeros(N) if has_vsini else None,
               params=np.zeros((N, ndim)), extra=np.zeros(N),
               bad=np.zeros(N, dtype=np.int32))
    with np.errstate(all='ignore'):
        for n in range(N):
            r = lst[n]
            pen = 0.0
            if has_vsini:
                if vsini_col >= 0:
                    v0 = theta[n, vsini_col]
                    vs = min(max(v0, 0.0), max_vsini) if v0 == v0 else v0
                    if v0 < 0 or v0 > max_vsini:
                        pen = pen + (vs - v0) * (vs - v0)
                else:
                    vs = vsini_fixed[r]
                out['vsini'][n] = vs
            isbad = False
            for e in range(eoff[n], eoff[n + 1]):
                if vel[e] > max_vel or vel[e] < min_vel:
                    isbad = True
            p = np.zeros(ndim)
            for i in range(ndim):
                p[i] = theta[n, src[i]] if src[i] >= 0 else fixed[r, i]
                if not abs(p[i]) <= 1.79e308:
                    isbad = True
            if isbad:
                p[:] = safe[r]
            if prior_mean is not None:
                for i in range(ndim):
                    d = (prior_mean[r, i] - p[i]) * prior_isig[r, i]
                    pen = pen + d * d
            out['star_id'][n] = r
            out['params'][n] = p
            out['extra'][n] = pen
            out['bad'][n] = 1 if isbad else 0
            for e in range(eoff[n], eoff[n + 1]):
                out['vel'][e] = 0.0 if isbad else vel[e]
                out['job_templ'][e] = n
    return out


def epoch_finish(chi, grad, fisher, theta, params, extra, bad, star_id, eoff, src,
                 vsini_col, prior_mean, prior_isig, max_vsini):
    """the ragged rows of all stars, one behind the other"""
    fisher = np.asarray(fisher, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    N, m = theta.shape
    K = fisher.shape[1]
    tan = tangents(m, src, vsini_col, K - 1)
    ro = row_offsets(m, eoff)
    F = np.zeros(ro[-1])
    head = 1 + m + m * (m + 1) // 2
    for n in range(N):
        e0, e1 = eoff[n], eoff[n + 1]
        f = F[ro[n]:ro[n + 1]]
        if bad[n]:
            f[0] = 1e30
            continue
        r = star_id[n]
        # the sums: the first epoch's value, then additions in epoch order
        sF = fisher[e0].copy()
        sg = np.array(grad[e0], dtype=np.float64)
        sc = np.float64(chi[e0])
        for e in range(e0 + 1, e1):
            sF = sF + fisher[e]
            sg = sg + grad[e]
            sc = sc + chi[e]
        inside, beyond = True, False
        if vsini_col >= 0:
            x = theta[n, vsini_col]
            cl = min(max(x, 0.0), max_vsini)
            inside = 0 < x < max_vsini
            beyond = x < 0 or x > max_vsini
        f[0] = sc + extra[n]
        for i in range(m):
            v = sg[tan[i]]
            if i == vsini_col:
                v = (v if inside else 0.0) + 2.0 * (x - cl)
            elif prior_mean is not None:
                s = prior_isig[r, tan[i] - 1]
                if s != 0:
                    v = v + 2.0 * (params[n, tan[i] - 1] - prior_mean[r, tan[i] - 1]) \
                        * s * s
            f[1 + i] = v
        for a in range(m):
            for b in range(a + 1):
                v = 2.0 * sF[tan[a], tan[b]]
                if (a == vsini_col or b == vsini_col) and not inside:
                    v = 0.0
                if a == b:
                    if a == vsini_col:
                        if beyond:
                            v = v + 2.0
                    elif prior_mean is not None:
                        s = prior_isig[r, tan[a] - 1]
                        if s != 0:
                            v = v + 2.0 * (s * s)
                f[1 + m + a * (a + 1) // 2 + b] = v
        for e in range(e0, e1):
            rec = f[head + (e - e0) * (2 + m):head + (e - e0 + 1) * (2 + m)]
            rec[0] = grad[e][0]
            rec[1] = 2.0 * fisher[e, 0, 0]
            for i in range(m):
                v = 2.0 * fisher[e, tan[i], 0]
                if i == vsini_col and not inside:
                    v = 0.0
                rec[2 + i] = v
    return F
