"""CPU statements, in torch, of an MLP template library (nn Mapper + Linear / SiLU stack
+ float64 exp(clip)) and of its derivative by the physical parameters, for the tests of
rvs_template_nn_grad.  Written from the formulas, not from the device code:

  input      x_d = (f32(q_d) - M_d) / S_d rounded to float32, q_d = log10(p_d) for a
             parameter of log_ids, else p_d  (Mapper.forward)
  hidden     a+ = z sigma(z), z = W a + b          (SiLU behind every layer but the last)
  output     t = exp(clip(y, -300, 300)), y = W a + b, in float64
  derivative dt/dp_k = (dt/dx_k at the rounded x) * s_k / S_k, s_k = 1 / (p_k ln 10)
             for a log parameter and 1 otherwise, at the float64 p_k: the float32
             casts of the Mapper are taken as the identity

jacobian64: the network in float64 (the float32 weights widened exactly), dt/dx from
torch.autograd -- the truth.
forward32: the same network in float32 arithmetic with forward-mode tangents (one-hot
tangents at x, the SiLU derivative sigma (1 + z (1 - sigma)) layer by layer), exp and
the factors s_k / S_k in float64 -- what float32 arithmetic alone loses against the
truth, in whatever order the host's matrix product sums.

chain_truth: the continuum-marginalised chi^2 of tests/chisq_grad_truth.py, its
gradient and the Fisher matrix of tests/chisq_fisher_truth.py as functions of GIVEN
template rows [1 + ndim, ntp] (value and tangents): the template enters as
rows[0] + sum_k u_k rows[1 + k] at u = 0, so d/du_k is the derivative by parameter k
for whoever made the rows.
"""
import os

import numpy as np
import torch

import chisq_grad_truth as truth
import vsini_grad_truth as vtruth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
C_KMS = truth.C_KMS
LOG_IDS = (0, )
NDIM = 4


def network(path=None):
    """dict(W, b: lists of float32 arrays, M, S, dims, params, pts) of nn_case.npz"""
    d = np.load(path or os.path.join(GOLD, 'nn_case.npz'))
    nl = len(d['dims']) - 1
    return dict(W=[d['W%d' % i] for i in range(nl)], b=[d['b%d' % i] for i in range(nl)],
                M=d['M'], S=d['S'], dims=d['dims'], params=d['params'], pts=d['pts'])


def lib_dict(net, lam, hull=True):
    """the dictionary TemplateLibrary reads for the network `net` on the grid `lam`"""
    dd = dict(lam=lam, log_step=np.array(True), log_ids=np.array(LOG_IDS),
              parnames=np.array(['teff', 'logg', 'feh', 'alpha'][:len(net['M'])] +
                                ['p%d' % i for i in range(4, len(net['M']))]),
              nn_dims=np.asarray(net['dims'], dtype=np.int32), nn_M=net['M'],
              nn_S=net['S'])
    if hull and net.get('pts') is not None:
        dd['nn_pts'] = net['pts']
    for i, (W, b) in enumerate(zip(net['W'], net['b'])):
        dd['nn_W%d' % i] = W
        dd['nn_b%d' % i] = b
    return dd


def points(net, B, seed=0, shrink=0.01):
    """B parameter vectors inside the training hull: the golden points whose outside
    flag is 0 (the first 22), cycled, each mapped coordinate moved by up to `shrink`
    of itself towards the origin of the mapped space (the mean of the training
    points, inside both convex hulls)"""
    rng = np.random.default_rng(seed)
    base = net['params'][:22]
    p = base[np.arange(B) % len(base)].copy()
    x = mapped(net, p)                       # float64 copy of the mapped point
    x = x * (1.0 - shrink * rng.uniform(0.0, 1.0, size=x.shape))
    q = x * net['S'][None, :] + net['M'][None, :]
    for d in LOG_IDS:
        q[:, d] = 10.0**q[:, d]
    return q


def mapped(net, p):
    """Mapper.forward: float32 input, log10, (q - M) / S in float64, rounded to float32;
    returned as float64 [B, ndim]"""
    q = np.asarray(p, dtype=np.float64).astype(np.float32)
    with np.errstate(all='ignore'):
        for d in LOG_IDS:
            q[:, d] = np.log10(q[:, d].astype(np.float64)).astype(np.float32)
    x = ((q.astype(np.float64) - net['M'][None, :]) / net['S'][None, :])
    return x.astype(np.float32).astype(np.float64)


def input_scale(net, p):
    """s_k / S_k [B, ndim] at the float64 parameters"""
    p = np.asarray(p, dtype=np.float64)
    s = np.ones_like(p)
    for d in LOG_IDS:
        s[:, d] = 1.0 / (p[:, d] * np.log(10.0))
    return s / net['S'][None, :]


def log_template64(net, x):
    """y [B, ntp] of the float64 network at the torch float64 points x [B, ndim]"""
    a = x
    nl = len(net['W'])
    for l in range(nl):
        z = a @ torch.as_tensor(net['W'][l].astype(np.float64)).T + \
            torch.as_tensor(net['b'][l].astype(np.float64))
        a = z * torch.sigmoid(z) if l < nl - 1 else z
    return a


def template64(net, x):
    return torch.exp(torch.clamp(log_template64(net, x), -300.0, 300.0))


def jacobian64(net, p):
    """(t [B, ntp], dt/dp [B, ndim, ntp]) of the float64 network, the Jacobian from
    autograd at x = Mapper.forward(p) (float32-rounded), times the analytic s_k / S_k"""
    x0 = torch.as_tensor(mapped(net, p))
    B, nd = x0.shape
    t = template64(net, x0).numpy()
    jac = np.zeros((B, nd, t.shape[1]))
    for k in range(nd):
        e = torch.zeros_like(x0)
        e[:, k] = 1.0
        # (rows are independent: one jvp gives column k of every job's Jacobian)
        jac[:, k, :] = torch.autograd.functional.jvp(
            lambda x: template64(net, x), x0, e)[1].numpy()
    return t, jac * input_scale(net, p)[:, :, None]


def forward32(net, p):
    """(t [B, ntp], dt/dp [B, ndim, ntp]) of the float32 network with forward-mode
    float32 tangents; exp(clip) and s_k / S_k in float64"""
    x = torch.as_tensor(mapped(net, p).astype(np.float32))
    B, nd = x.shape
    nl = len(net['W'])
    a = x                                                  # [B, K]
    da = torch.eye(nd, dtype=torch.float32)[None].repeat(B, 1, 1)   # [B, nd, K]
    for l in range(nl):
        W = torch.as_tensor(net['W'][l])
        z = a @ W.T + torch.as_tensor(net['b'][l])
        dz = da @ W.T
        if l < nl - 1:
            sg = 1.0 / (1.0 + torch.exp(-z))
            a = z * sg
            da = (sg * (1.0 + z * (1.0 - sg)))[:, None, :] * dz
        else:
            a, da = z, dz
    y = a.numpy().astype(np.float64)
    t = np.exp(np.clip(y, -300.0, 300.0))
    flat = np.abs(y) > 300.0
    jac = t[:, None, :] * da.numpy().astype(np.float64) * input_scale(net, p)[:, :, None]
    jac[np.broadcast_to(flat[:, None, :], jac.shape)] = 0.0
    return t, jac


def tangent_metric(got, want):
    """per (job, k): max_pix |got - want| / max_pix |want|, [B, ndim]"""
    return np.abs(got - want).max(axis=2) / np.abs(want).max(axis=2)


# ---- the chain behind the rows --------------------------------------------------------
class _Lam:
    def __init__(self, lam):
        self.lam = lam


def _model_row(sd_lam, lam, rows, theta, vsini_var, vs_fixed):
    nd = rows.shape[0] - 1
    t = rows[0] + theta[1:1 + nd] @ rows[1:]
    if vsini_var:
        t = vtruth.broadened(_Lam(lam), t, theta[1 + nd])
    elif vs_fixed is not None and vs_fixed > 0:
        t = vtruth.broadened(_Lam(lam), t, torch.tensor(float(vs_fixed),
                                                        dtype=torch.float64))
    beta = theta[0] / C_KMS
    x = torch.as_tensor(sd_lam) * torch.sqrt((1 - beta) / (1 + beta))
    return truth.spline_eval(lam, t, x)


def chain_truth(arms, vel, vsini, npoly, vsini_grad, rbf=True):
    """arms: [(lam_pix, spec, espec, lam_templ, rows [1 + ndim, ntp] numpy)].
    theta = (vel, u [ndim][, vsini]) at u = 0.  Returns dict(chi, grad [K], F, G [K, K],
    cond): chi^2 as chisq_grad_truth.marginal_chisq states it (no penalty) with
    autograd's gradient; F, G and cond(A) as chisq_fisher_truth.arm_fisher builds them
    from the Jacobian of the model row."""
    nd = arms[0][4].shape[0] - 1
    th = [float(vel)] + [0.0] * nd + ([float(vsini)] if vsini_grad else [])
    K = len(th)
    theta = torch.tensor(th, dtype=torch.float64, requires_grad=True)
    tot = 0.0 * theta.sum()
    F, G, cond = np.zeros((K, K)), np.zeros((K, K)), 0.0
    for lam_pix, spec, espec, lam, rows in arms:
        rows_t = torch.as_tensor(rows)
        f = lambda q: _model_row(lam_pix, lam, rows_t, q, vsini_grad, vsini)  # noqa: E731
        Q, const = truth.ortho_basis(lam_pix, npoly, rbf)
        tot = tot + truth.marginal_chisq(f(theta), Q, const, torch.as_tensor(spec),
                                         torch.as_tensor(espec))
        th0 = theta.detach().clone()
        m = f(th0).numpy()
        Jm = torch.autograd.functional.jacobian(f, th0).numpy()
        Qn = Q.numpy()
        e = np.asarray(espec, dtype=np.float64)
        STt = (Qn * (m / e)[None, :]).T
        U, R = np.linalg.qr(STt)
        c = np.linalg.solve(R, U.T @ (np.asarray(spec, dtype=np.float64) / e))
        s = c @ Qn
        Jw = Jm * (s / e)[:, None]
        Jp = Jw - U @ (U.T @ Jw)
        sv = np.linalg.svd(STt, compute_uv=False)
        F += Jp.T @ Jp
        G += Jw.T @ Jw
        cond = max(cond, float((sv[0] / sv[-1])**2))
    tot.backward()
    return dict(chi=float(tot.item()), grad=theta.grad.numpy().copy(), F=F, G=G,
                cond=cond)
