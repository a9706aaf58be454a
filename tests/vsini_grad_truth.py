"""Float64 CPU statement of the rotational-broadening taps w(R) and of their derivative
dw/dR, and the truth of tests/chisq_grad_truth.py with vsini as one more, last,
parameter.  Written from the formulas, not from the device code:

  profile    K(x) = c1 sqrt(1 - x^2) + c2 (1 - x^2) on [-1, 1], c1 = 2 (1 - eps) / n,
             c2 = (pi / 2) eps / n, n = pi (1 - eps / 3)           (integral 1)
  taps       W_k(R) = int Lambda(k - R x) K(x) dx, Lambda the unit hat: on the left
             leg x in [k/R, (k+1)/R] Lambda = 1 + k - R x, on the right leg
             x in [(k-1)/R, k/R] Lambda = 1 - k + R x; both clipped to [-1, 1]
  derivative Lambda is continuous and vanishes at its ends, K(+-1) = 0: the boundary
             terms of Leibniz's rule cancel and
             dW_k/dR = -int_left x K dx + int_right x K dx
  normalised w = W / S, S = W_0 + 2 sum_{k >= 1} W_k, dw/dR = (W' - w S') / S

The primitives: P0 of K, P1 of x K,
  P0(x) = c1 (x sqrt(1 - x^2) + asin x) / 2 + c2 (x - x^3 / 3)
  P1(x) = -c1 (1 - x^2)^(3/2) / 3 + c2 (x^2 / 2 - x^4 / 4)
"""
import numpy as np
import torch

import chisq_grad_truth as truth

C_KMS = truth.C_KMS


def _primitives(x, eps):
    n = np.pi * (1 - eps / 3.0)
    c1, c2 = 2 * (1 - eps) / n, (np.pi / 2.0) * eps / n
    u = 1 - x * x
    s = np.sqrt(u)
    return (c1 * (x * s + np.arcsin(x)) / 2 + c2 * (x - x**3 / 3),
            -c1 * u * s / 3 + c2 * (x * x / 2 - x**4 / 4))


def taps(R, eps=0.6):
    """(w [2 kmax + 1], dw/dR [2 kmax + 1]) of the normalised symmetric kernel,
    kmax = ceil(R + 1) as the reference sizes it (the outer taps are zero)"""
    assert R > 0
    kmax = int(np.ceil(R + 1))
    k = np.arange(kmax + 1, dtype=np.float64)
    W = np.zeros(kmax + 1)
    dW = np.zeros(kmax + 1)
    for lo, hi, sign in ((k / R, (k + 1) / R, -1.0), ((k - 1) / R, k / R, 1.0)):
        lo, hi = np.clip(lo, -1, 1), np.clip(hi, -1, 1)
        a0, a1 = _primitives(lo, eps)
        b0, b1 = _primitives(hi, eps)
        i0, i1 = b0 - a0, b1 - a1       # int K, int x K over the clipped leg
        m = hi > lo
        # Lambda = 1 -+ k +- R x on the leg
        W[m] += ((1 - sign * k) * i0 + sign * R * i1)[m]
        dW[m] += (sign * i1)[m]
    S = W[0] + 2 * W[1:].sum()
    dS = dW[0] + 2 * dW[1:].sum()
    w = W / S
    dw = (dW - w * dS) / S
    return np.concatenate([w[:0:-1], w]), np.concatenate([dw[:0:-1], dw])


def lnstep(lib):
    return float(np.log(lib.lam[1] / lib.lam[0]))


def broadened(lib, t, vs):
    """t [ntp] (torch) 'same'-convolved with the taps at the torch scalar vs, entering
    as w(R0) + dw/dR(R0) (R - R0): value and first derivative at R0 are the function's,
    and no derivative is asked of sqrt(1 - x^2) at a clipped endpoint (0 * inf)"""
    v0 = float(vs.detach())
    if not v0 > 0:
        return t
    ls = lnstep(lib)
    R0 = (v0 / C_KMS) / ls
    if R0 < 1e-9:
        return t
    w, dw = taps(R0)
    ker = torch.as_tensor(w) + torch.as_tensor(dw) * ((vs / C_KMS) / ls - R0)
    k = (len(w) - 1) // 2
    return torch.nn.functional.conv1d(t[None, None, :], ker[None, None, :],
                                      padding=k)[0, 0]


def chisq_and_grad_vsini(sds, libs, vel, params, vsini, npoly=5, rbf=True,
                         outside_penalty=True):
    """truth.chisq_and_grad with theta = (vel, *params, vsini): (float,
    ndarray [2 + ndim]), the vsini component per km/s.  vsini <= 0 is the unbroadened
    template (the clamp): that component is then 0."""
    theta = torch.tensor([float(vel)] + [float(_) for _ in params] + [float(vsini)],
                         dtype=torch.float64, requires_grad=True)
    badchi = 10 * sum(len(sd.lam) for sd in sds)
    tot = 0.0 * theta.sum()
    pen = 0.0
    for sd in sds:
        lib = libs[sd.name]
        t, outside = truth.template(lib, theta[1:-1])
        if not np.isfinite(outside):
            pen += 1000.0 * badchi
            continue
        if outside_penalty:
            pen += outside * badchi
        t = broadened(lib, t, theta[-1])
        beta = theta[0] / C_KMS
        x = torch.as_tensor(sd.lam) * torch.sqrt((1 - beta) / (1 + beta))
        m = truth.spline_eval(lib.lam, t, x)
        Q, const = truth.ortho_basis(sd.lam, npoly, rbf)
        tot = tot + truth.marginal_chisq(m, Q, const, torch.as_tensor(sd.spec),
                                         torch.as_tensor(sd.espec))
    tot.backward()
    return float(tot.item()) + pen, theta.grad.numpy().copy()


def vsini_for(lib, R):
    """the vsini (km/s) that gives R taps' widths on `lib`'s grid"""
    return R * C_KMS * lnstep(lib)
