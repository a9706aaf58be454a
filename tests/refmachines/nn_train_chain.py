"""One training step of the MLP template interpolator in float32, restated in plain
numpy in the summation order the header of csrc/nn_train.hip states (and not from its
code): every product is one float32 accumulator per output, updated in ascending k with
one rounding per term, as the f32-input MFMA chains do; the bias gradient is a float32
column sum in ascending rows; dA of the output layer is the float32 sum, in chunk order,
of the chains over chunks of 128 pixels.

It is NOT a bit reference: the fused multiply-add is float32(float64(acc) + float64(a) *
float64(b)) (the product of two float32 is exact in float64; the sum is rounded twice,
which differs from one rounding in rare ties), and exp is numpy's.  It sets the scale of
a tolerance: how far a correct float32 evaluation IN THIS ORDER lies from float64, which
at 1024 rows is several times what torch's blocked sums leave
(tests/nn_train_shapes.py).
"""
import numpy as np
import torch

SPLIT = 128      # pixels per chunk of the output layer's dA


def chain(A, B):
    """C[m, n] = sum_k A[m, k] B[n, k]: A [M, K], B [N, K] float32 -> [M, N] float32"""
    A = np.asarray(A, dtype=np.float32)
    B = np.asarray(B, dtype=np.float32)
    At = np.ascontiguousarray(A.T, dtype=np.float64)
    Bt = np.ascontiguousarray(B.T, dtype=np.float64)
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    tmp = np.empty(acc.shape, dtype=np.float64)
    for k in range(A.shape[1]):
        np.multiply.outer(At[k], Bt[k], out=tmp)
        tmp += acc
        acc[...] = tmp
    return acc


def _sigmoid(z):
    one = np.float32(1)
    return one / (one + np.exp(-z))


def _silu(z):
    return z * _sigmoid(z)


def _dsilu(z):
    one = np.float32(1)
    s = _sigmoid(z)
    return s * (one + z * (one - s))


def _colsum(g):
    s = np.zeros(g.shape[1], dtype=np.float32)
    for row in g:
        s = s + row
    return s


def _np32(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.ascontiguousarray(t, dtype=np.float32)


def loss_and_grads(W, b, x, dat, D0, SD0, spread0, sign=None):
    """As nn_train_torch.loss_and_grads: -> loss (0-d float64 tensor), residual R - dat,
    [dW...], [db...] (float32 tensors).  sign: drive the backward pass with this sign
    pattern instead of sign(residual)"""
    W, b = [_np32(w) for w in W], [_np32(v) for v in b]
    x, dat, D0, SD0 = _np32(x), _np32(dat), _np32(D0), _np32(SD0)
    L = len(W)
    rows, npix = dat.shape
    a, z = [x], [None]
    for l in range(L - 1):
        z.append(chain(a[l], W[l]) + b[l])
        a.append(_silu(z[-1]))
    v = chain(a[L - 1], W[L - 1]) + b[L - 1]
    R = (v.astype(np.float64) * SD0.astype(np.float64) + D0.astype(np.float64)).astype(
        np.float32)
    r = R - dat
    count = float(rows) * npix
    loss = np.abs(r).astype(np.float64).sum() / (count * float(spread0))
    s = np.sign(r) if sign is None else _np32(sign)
    g = (s * SD0) * np.float32(1.0 / (count * float(spread0)))
    dW, db = [None] * L, [None] * L
    dW[L - 1] = chain(g.T, a[L - 1].T)
    db[L - 1] = _colsum(g)
    dA = np.zeros((rows, W[L - 1].shape[1]), dtype=np.float32)
    for c in range(0, npix, SPLIT):
        dA = dA + chain(g[:, c:c + SPLIT], W[L - 1][c:c + SPLIT].T)
    g = dA * _dsilu(z[L - 1])
    for l in range(L - 2, -1, -1):
        dW[l] = chain(g.T, a[l].T)
        db[l] = _colsum(g)
        if l:
            g = chain(g, W[l].T) * _dsilu(z[l])
    return (torch.tensor(loss, dtype=torch.float64), torch.from_numpy(r),
            [torch.from_numpy(w) for w in dW], [torch.from_numpy(v) for v in db])
