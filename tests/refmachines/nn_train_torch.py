"""The training loop of the MLP template interpolator, restated in plain torch.

What the reference does per batch (nn/train_interpolator.py:284-322) with
NNInterpolator(withbn=False, SiLU) (nn/NNInterpolator.py:14-91), written from the
formulas and not from that code: Linear + SiLU for every layer but the last,
R = net(x) * SD_0 + D_0, loss = mean|R - dat| / spread0, autograd, Adam with
torch.optim.Adam's defaults (restated from torch/optim/adam.py:_single_tensor_adam,
not called), one permutation per epoch cut into batches with the last one short.

It serves two ends: tests/test_nn_train_cpu.py pins it to
tests/golden/nn_train_cases.npz (made with the reference's own class and torch's own
optimiser), and the device trainer (csrc/nn_train.hip) is held against it in any
dtype -- float64 for the gradient tests -- and timed against it on the same device
(tools/perf/nn_train_timing.py).
"""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'golden')
SEED = 343432323        # train_interpolator.py:171
FIXTURE_DIMS = (4, 64, 64, 64, 40, 977)   # indim 4, nlayers 2, width 64, npc 40


def fixture_rows():
    """The training set of nn_train_cases.npz: dats / vec of lib_gold_b.npz as getData
    and main hand them to the loop (train_interpolator.py:28-38, 177-178, 241; the
    library's vec is the mapped one already, so no log10 here).  Returns a dict of
    numpy arrays: dats, x (float32), D0, SD0 (float32), spread0, M, S."""
    d = np.load(os.path.join(GOLD, 'lib_gold_b.npz'))
    dats = np.ascontiguousarray(d['dats'], dtype=np.float32)
    vecs = np.asarray(d['vec'], dtype=np.float32).T
    M, S = vecs.mean(axis=0), vecs.std(axis=0)
    x = np.ascontiguousarray(((vecs - M) / S).astype(np.float32))
    D0, SD0 = np.mean(dats, axis=0), np.std(dats, axis=0)
    spread0 = np.std(dats - np.mean(dats, axis=0))
    return dict(dats=dats, x=x, D0=D0, SD0=SD0, spread0=float(spread0), M=M, S=S)


def init_weights(dims, seed=SEED):
    """torch's default Linear initialisation, layer after layer under one seed: what
    NNInterpolator.__init__ draws (its Linear modules are made in this order)"""
    torch.manual_seed(seed)
    W, b = [], []
    for i in range(len(dims) - 1):
        lin = torch.nn.Linear(int(dims[i]), int(dims[i + 1]))
        W.append(lin.weight.detach().clone())
        b.append(lin.bias.detach().clone())
    return W, b


def forward(W, b, x):
    a = x
    for l in range(len(W) - 1):
        a = torch.nn.functional.silu(a @ W[l].T + b[l])
    return a @ W[-1].T + b[-1]


def loss_and_grads(W, b, x, dat, D0, SD0, spread0, sign=None):
    """-> loss (0-d tensor), residual R - dat, [dW...], [db...].  sign: drive the
    backward pass with this sign pattern instead of sign(residual)"""
    P = [t.detach().clone().requires_grad_(True) for t in list(W) + list(b)]
    n = len(W)
    R = forward(P[:n], P[n:], x) * SD0 + D0
    res = R - dat
    loss = res.abs().mean() / spread0
    if sign is None:
        loss.backward()
    else:
        R.backward(gradient=sign.to(R.dtype) / (res.numel() * spread0))
    return loss.detach(), res.detach(), [p.grad for p in P[:n]], [p.grad for p in P[n:]]


class Adam:
    """betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad"""

    def __init__(self, params):
        self.p = list(params)
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = 0

    def step(self, grads, lr):
        self.t += 1
        bc1, bc2 = 1 - 0.9**self.t, 1 - 0.999**self.t
        for p, m, v, g in zip(self.p, self.m, self.v, grads):
            # (lerp_ and addcmul_ round once where torch's CPU kernels use a fused
            # multiply-add; spelled with * and + the moments differ in the last bit)
            m.lerp_(g, 1 - 0.9)
            v.mul_(0.999).addcmul_(g, g, value=1 - 0.999)
            denom = (v.sqrt() / bc2**0.5).add_(1e-8)
            p.addcdiv_(m, denom, value=-(lr / bc1))


def train_epoch(W, b, opt, dats, x, perm, batch, lr, D0, SD0, spread0):
    """one epoch over the rows perm; -> lossAccum (float), [loss of each step]"""
    npix = dats.shape[1]
    accum, steps = 0.0, []
    for i in range(0, len(perm), batch):
        idx = perm[i:i + batch]
        loss, _, dW, db = loss_and_grads(W, b, x[idx], dats[idx], D0, SD0, spread0)
        opt.step(dW + db, lr)
        steps.append(float(loss))
        accum += float(loss) * len(idx) * npix
    return accum, steps
