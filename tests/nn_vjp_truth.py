"""CPU statements for the tests of the reverse pass through an MLP template library
(rvs_template_nn_vjp) and of the adjoint row it starts from
(rvs_objective_grad_from_template), written from the formulas of DESIGN 4.25 and of
tests/nn_grad_truth.py, not from the device code:

  vjp64      gparams_k = sum_n tbar_n jacobian64[k, n]: the float64 truth, with the
             scale sum_n |tbar_n jacobian64[k, n]| a float32 sum over the pixels works at
  reverse32  the reverse pass in float32 torch:
               ybar_n = tbar_n t_n in float64, exactly 0 where t_n is exp(+-300);
               each row divided by 2^e, e the exponent of max |ybar|, cast to float32;
               abar = ybar W_L; back through the hidden layers with the forward pass's z,
               delta_l = abar_l sigma (1 + z (1 - sigma)), abar_{l-1} = delta_l W_l;
               xbar 2^e s_k / S_k in float64
  template_adjoint_truth
             d chi^2 / d t by float64 autograd through nn_grad_truth._model_row and
             chisq_grad_truth.marginal_chisq with the template row t as the leaf
"""
import numpy as np
import torch

import chisq_grad_truth as truth
import nn_grad_truth as nt


def vjp64(net, p, tbar):
    """(gparams [B, ndim], scale [B, ndim]) from the float64 Jacobian"""
    _, jac = nt.jacobian64(net, p)
    prod = jac * np.asarray(tbar, dtype=np.float64)[:, None, :]
    return prod.sum(axis=2), np.abs(prod).sum(axis=2)


def row_exponents(ybar):
    """e [B] with max |ybar| = f 2^e, f in [0.5, 1); 0 for a zero or non-finite row"""
    mx = np.abs(ybar).max(axis=1)
    e = np.zeros(len(mx), dtype=np.int64)
    ok = (mx > 0) & np.isfinite(mx)
    e[ok] = np.frexp(mx[ok])[1]
    return e


def reverse32(net, p, t, tbar):
    """gparams [B, ndim] of the float32 reverse pass; t: the value rows [B, ntp]
    (float64) the adjoint rows tbar belong to"""
    t = np.asarray(t, dtype=np.float64)
    ybar = np.asarray(tbar, dtype=np.float64) * t
    ybar[(t >= np.exp(300.0)) | (t <= np.exp(-300.0))] = 0.0
    e = row_exponents(ybar)
    y32 = torch.as_tensor(np.ldexp(ybar, -e[:, None]).astype(np.float32))
    x = torch.as_tensor(nt.mapped(net, p).astype(np.float32))
    nl = len(net['W'])
    a, zs = x, []
    for l in range(nl - 1):
        z = a @ torch.as_tensor(net['W'][l]).T + torch.as_tensor(net['b'][l])
        zs.append(z)
        a = z / (1.0 + torch.exp(-z))
    abar = y32 @ torch.as_tensor(net['W'][nl - 1])
    for l in range(nl - 2, -1, -1):
        z = zs[l]
        sg = 1.0 / (1.0 + torch.exp(-z))
        delta = abar * (sg * (1.0 + z * (1.0 - sg)))
        abar = delta @ torch.as_tensor(net['W'][l])
    xbar = np.ldexp(abar.numpy().astype(np.float64), e[:, None])
    return xbar * nt.input_scale(net, p)


def vjp_metric(got, want, scale):
    """|got - want| / sum_n |tbar_n jac64[k, n]| per (job, k)"""
    return np.abs(got - want) / scale


def template_adjoint_truth(sd_lam, spec, espec, lam, t, vel, vsini=None, npoly=5,
                           rbf=True):
    """(chi^2 without penalties, d chi^2 / d vel, tbar [ntp], cond(A)) of one arm at the
    template row t (float64 [ntp]); vsini: a fixed broadening, or None; cond(A): the
    conditioning of the normal equations, as nn_grad_truth.chain_truth states it"""
    leaf = torch.tensor(np.asarray(t, dtype=np.float64), requires_grad=True)
    theta = torch.tensor([float(vel)], dtype=torch.float64, requires_grad=True)
    m = nt._model_row(sd_lam, lam, leaf[None, :], theta, False, vsini)
    Q, const = truth.ortho_basis(sd_lam, npoly, rbf)
    chi = truth.marginal_chisq(m, Q, const, torch.as_tensor(spec), torch.as_tensor(espec))
    chi.backward()
    e = np.asarray(espec, dtype=np.float64)
    sv = np.linalg.svd((Q.numpy() * (m.detach().numpy() / e)[None, :]).T, compute_uv=False)
    return (float(chi.item()), float(theta.grad[0].item()), leaf.grad.numpy().copy(),
            float((sv[0] / sv[-1])**2))
