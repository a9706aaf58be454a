"""The mapping of rvs_proc_finish_fisher, Fisher matrix -> Gauss-Newton Hessian of
chisq_func in the optimiser's columns, stated in numpy twice: entry by entry as the
kernel forms it (hess_from_fisher), and by brute force -- build the full K x K matrix
over (vel, every library parameter, vsini), add the prior and clamp terms there, then
select the optimiser's columns (hess_brute).  tests/test_lm_cpu.py holds the two against
each other on seeded rows; tests/test_lm_gpu.py holds the kernel against the first.

  fisher [J, K, K]   K = 1 + ntan, ordered (vel, library parameters, vsini last), in
                     the 0.5 chi^2 convention
  X [J, n]           the optimiser's rows; column 0 is the velocity
  src [ndim]         column of X of library parameter i, or -1 where it is fixed
  vsini_col          column of X of vsini, or -1
  isig [J, ndim]     1 / sigma of a parameter's prior (0: none), or None
"""
import numpy as np


def tangents(n, src, vsini_col, ntan):
    """column of X -> row of the Fisher matrix"""
    tan = [0] * n
    for i, c in enumerate(src):
        if c >= 0:
            tan[c] = 1 + i
    if vsini_col >= 0:
        tan[vsini_col] = ntan
    return tan


def hess_from_fisher(fisher, X, src, vsini_col, isig, max_vsini):
    fisher = np.asarray(fisher, dtype=np.float64)
    J, K = fisher.shape[:2]
    n = X.shape[1]
    tan = tangents(n, src, vsini_col, K - 1)
    H = np.zeros((J, n, n))
    for j in range(J):
        inside = beyond = False
        if vsini_col >= 0:
            x = X[j, vsini_col]
            inside = 0 < x < max_vsini
            beyond = x < 0 or x > max_vsini
        for a in range(n):
            for b in range(a + 1):
                v = 2.0 * fisher[j, tan[a], tan[b]]
                if (a == vsini_col or b == vsini_col) and not inside:
                    v = 0.0
                if a == b:
                    if a == vsini_col:
                        if beyond:
                            v += 2.0
                    elif tan[a] >= 1 and isig is not None:
                        s = isig[j, tan[a] - 1]
                        if s != 0:
                            v += 2.0 * (s * s)
                H[j, a, b] = H[j, b, a] = v
    return H


def hess_brute(fisher, X, src, vsini_col, isig, max_vsini):
    fisher = np.asarray(fisher, dtype=np.float64)
    J, K = fisher.shape[:2]
    n = X.shape[1]
    ndim = len(src)
    out = np.zeros((J, n, n))
    for j in range(J):
        full = 2.0 * fisher[j]
        if vsini_col >= 0:
            x = X[j, vsini_col]
            if not (0 < x < max_vsini):
                full[K - 1, :] = 0.0
                full[:, K - 1] = 0.0
            if x < 0 or x > max_vsini:
                full[K - 1, K - 1] += 2.0
        if isig is not None:
            full[1:1 + ndim, 1:1 + ndim] += np.diag(2.0 * isig[j] * isig[j])
        keep = np.array(tangents(n, src, vsini_col, K - 1))
        out[j] = full[np.ix_(keep, keep)]
    return out


def seeded_rows(seed, J, n, src, vsini_col, max_vsini=500.0, prior=True):
    """seeded rows for one configuration: fisher [J, K, K] (symmetric PSD), X [J, n],
    isig [J, ndim].  The vsini column runs through x < 0, x = 0 exactly, inside,
    x = max exactly, x > max; one prior has isig = 0."""
    rng = np.random.RandomState(seed)
    ndim = len(src)
    K = 1 + ndim + (1 if vsini_col >= 0 else 0)
    B = rng.normal(size=(J, K, K + 2)) * np.logspace(-2, 3, K)[None, :, None]
    fisher = B @ B.transpose(0, 2, 1)
    fisher = 0.5 * (fisher + fisher.transpose(0, 2, 1))
    X = rng.normal(size=(J, n)) * 3
    if vsini_col >= 0:
        kinds = np.array([-7.5, 0.0, 13.25, max_vsini, max_vsini + 40.0, 1e-3])
        X[:, vsini_col] = kinds[np.arange(J) % len(kinds)]
    isig = None
    if prior:
        isig = np.abs(rng.normal(size=(J, ndim))) * np.logspace(-2, 1, ndim)
        isig[:, 0] = 0.0
        isig[::3, ndim - 1] = 0.0
    return fisher, X, isig


def pack(f, g, H):
    """rows [J, 1 + n + n (n + 1) / 2] of (f [J], g [J, n], H [J, n, n])"""
    n = g.shape[1]
    il = np.tril_indices(n)
    return np.concatenate([f[:, None], g, H[:, il[0], il[1]]], axis=1)
