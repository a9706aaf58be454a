"""Float64 autograd statement of the adjoint row under a resolution matrix, with the
template row as the leaf: tests/nn_vjp_truth.template_adjoint_truth with the dense matrix R
between the resampling and the pixels.  Independent of the adjoint method: nothing here
transposes anything by hand.

  m      = R @ spline_eval(broadened(t), lam * sqrt((1 - b) / (1 + b)))
  tbar   = d marginal_chisq(m) / d t                       (torch.autograd)
  terms  = sum_k |mbar_k  d m_k / d t_n|,  mbar = d chi^2 / d m: the absolute sum behind
           tbar_n, the scale an error of tbar_n is measured against
"""
import numpy as np
import torch

import chisq_grad_truth as truth
import nn_grad_truth as nt


def adjoint_row(sd, lam, t, R, vel, vsini=None, npoly=5, rbf=True):
    """(chi^2 without penalties, d chi^2 / d vel, tbar [ntp], terms [ntp], cond(A)) of one
    arm `sd` (lam, spec, espec) at the template row t on the knots `lam` under the dense
    float64 matrix R (None: no matrix)"""
    sd_lam = np.asarray(sd.lam, dtype=np.float64)
    Rd = None if R is None else torch.as_tensor(np.asarray(R, dtype=np.float64))

    def model(leaf, theta):
        m = nt._model_row(sd_lam, lam, leaf[None, :], theta, False, vsini)
        return m if Rd is None else Rd @ m

    leaf = torch.tensor(np.asarray(t, dtype=np.float64), requires_grad=True)
    theta = torch.tensor([float(vel)], dtype=torch.float64, requires_grad=True)
    m = model(leaf, theta)
    Q, const = truth.ortho_basis(sd_lam, npoly, rbf)
    spec, espec = torch.as_tensor(sd.spec), torch.as_tensor(sd.espec)
    chi = truth.marginal_chisq(m, Q, const, spec, espec)
    chi.backward()
    # the absolute sum behind every entry: mbar with the model row as the leaf, times the
    # Jacobian of the (linear) map t -> m
    mleaf = m.detach().clone().requires_grad_(True)
    truth.marginal_chisq(mleaf, Q, const, spec, espec).backward()
    th0 = theta.detach()
    Jm = torch.autograd.functional.jacobian(lambda q: model(q, th0), leaf.detach())
    terms = (mleaf.grad.abs()[:, None] * Jm.abs()).sum(0).numpy()
    e = np.asarray(sd.espec, dtype=np.float64)
    sv = np.linalg.svd((Q.numpy() * (m.detach().numpy() / e)[None, :]).T, compute_uv=False)
    return (float(chi.item()), float(theta.grad[0].item()), leaf.grad.numpy().copy(), terms,
            float((sv[0] / sv[-1])**2))


def row_error(tb, want, terms):
    """the largest error of the row tb against the truth's, relative to the absolute sum
    behind the entry (at least 1e-6 of the largest such sum: the project's floor)"""
    return float((np.abs(tb - want) / np.maximum(terms, 1e-6 * terms.max())).max())
