"""The cases of tests/test_nn_train_shapes_cpu.py and ..._gpu.py: the networks and
batches at which the trainer's one tile routine (nt_tile of csrc/nn_train.hip: 64 x 64
blocks, K in slabs of 32, the output layer's dA in chunks of 128 pixels) takes another
path.  No tests here.

Data of a case (dims, rows), seeded and made here, nothing committed: T = max(rows, 50)
+ 7 rows of a smooth function of the parameters plus noise (see data()); D_0, SD_0 and
spread0 as nn_train_torch.fixture_rows takes them; weights from nn_train_torch.
init_weights(dims); the batch is the first `rows` entries of a seeded permutation.

Tolerances (machines(), tolerances()): nothing is taken from what the device computes.
Two float32 machines are run on the CPU at the case's own shape against the float64
torch machine, all three driven by the same signs: the torch machine (nn_train_torch,
torch's blocked sums) and the chain machine (nn_train_chain, the kernel's summation
order).  The residual is held to 4 x the larger of their largest |r - r64|, each gradient
tensor to 4 x the larger of their norm-relative errors; both enter because their
summation orders differ (at 1024 rows the chain's error is several times torch's).  For
a tensor of fewer than 64 elements the tolerance is not below 4 (nlayer + 1) 2^-24: the
error of a handful of numbers is one draw and can be 0, and each element has passed at
least nlayer + 1 float32 roundings."""
import collections
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refmachines import nn_train_chain as cm  # noqa: E402
from refmachines import nn_train_torch as rm  # noqa: E402

SEED = 5
MARGIN = 4
TIE_FACTOR = 8          # a near-tie: |r64| < 8 res_tol
TIE_SHARE = 1e-4        # of rows x npix
SMALL = 64              # elements: below it the floor applies

Case = collections.namedtuple('Case', 'name dims rows seed', defaults=(SEED, ))

# name, dims, rows: what it is the smallest input for
CASES = [
    # the reference's default widths; several tiles along both extents of every hidden
    # product; db from blocks with m0 > 0; npc = 3 tiles + 8
    Case('default-net', (4, 256, 256, 256, 200, 1500), 100),
    # K = 100 (three slabs + 4), width and rows one past a tile, second pixel chunk of 2
    Case('odd', (3, 100, 65, 130), 65),
    # nlayer 2 (no hidden dA), batch at its limit, ndim 8, npc one past a slab, a chunk
    # of one pixel
    Case('two-layers', (8, 33, 129), 1024),
    # width and batch at their limits together: chains of 1024 in dA and in dW
    Case('max-width', (8, 1024, 33, 129), 1024),
    # 16 x 16 tiles of one dW
    Case('wide-wide', (4, 1024, 1024, 200, 300), 100),
    # nlayer 8, widths below one slab
    Case('deep', (2, 8, 8, 8, 8, 8, 8, 8, 64), 70),
    # 3 x 66 = 198 loss partials (the fold's loop runs four times, the last short), 33
    # pixel chunks
    Case('many-partials', (4, 70, 97, 4200), 129),
    # npix at its limit, 72 chunks, 144 partials
    Case('npix-max', (4, 32, 16, 9216), 64),
    # every extent an exact multiple of its tile, slab and chunk: the prefetch's
    # last-slab test, no partial tile anywhere
    Case('exact', (4, 64, 128, 256), 128),
    # one chunk, short and exact
    Case('chunk-127', (4, 40, 127), 32),
    Case('chunk-128', (4, 40, 128), 32),
    # every extent 1
    Case('ones-3', (1, 1, 1, 1), 1),
    Case('ones-2', (1, 1, 1), 1),
    # found while reading the kernels: the operand descriptor picks its lane layout by
    # `sk == 1`, and G [rows, N] read along the rows has sk = N: a width of 1 between
    # wider layers takes the other layout for that one operand (dW of the narrow layer).
    # (Seed 6: with seed 5 one of the 8450 residuals is a near-tie, cap 0.)
    Case('width-one', (4, 70, 1, 33, 130), 65, 6),
    # one row, wide layers: M = 1 tiles of every forward product, K = 1 in every dW
    Case('one-row', (4, 65, 200, 300), 1),
]
BY_NAME = {c.name: c for c in CASES}


def data(dims, rows, T=None, seed=SEED):
    """-> dict: x [T, ndim], dats [T, npix] (float32), D0, SD0 (float32), spread0
    (float), W, b (lists of float32 tensors), idx (the batch), T, dims, rows"""
    dims = tuple(int(d) for d in dims)
    ndim, npix = dims[0], dims[-1]
    T = max(rows, 50) + 7 if T is None else int(T)
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(T, ndim)).astype(np.float32)
    A = rng.normal(size=(ndim, 16))
    B = rng.normal(size=(16, npix)) / 4
    dats = (1 + 0.3 * np.tanh(x @ A) @ B / 4 +
            0.01 * rng.normal(size=(T, npix))).astype(np.float32)
    D0, SD0 = np.mean(dats, axis=0), np.std(dats, axis=0)
    spread0 = float(np.std(dats - np.mean(dats, axis=0)))
    W, b = rm.init_weights(dims)
    idx = np.random.default_rng(1).permutation(T)[:rows]
    return dict(x=x, dats=dats, D0=D0, SD0=SD0, spread0=spread0, W=W, b=b, idx=idx, T=T,
                dims=dims, rows=rows)


_cache = {}


def case_data(name):
    if name not in _cache:
        c = BY_NAME[name]
        _cache[name] = data(c.dims, c.rows, seed=c.seed)
    return _cache[name]


def _relerr(g, g64):
    return float((g.double() - g64).norm() / g64.norm())


def machines(D, idx=None, sign=None):
    """The three CPU machines on the rows idx of D.  sign None: the chain machine's own
    signs drive all three backward passes; else the given pattern does.
    -> dict: l64, r64, dW64, db64 (the float64 machine); sign; res_err {'chain',
    'torch'}: largest |r - r64|; gerr {'chain', 'torch'}: norm-relative error of dW0,
    db0, dW1, ... ; chain, torch32: what the two machines returned"""
    idx = D['idx'] if idx is None else idx
    x, dat = D['x'][idx], D['dats'][idx]
    t = torch.as_tensor
    if sign is None:
        chain = cm.loss_and_grads(D['W'], D['b'], x, dat, D['D0'], D['SD0'], D['spread0'])
        sign = torch.sign(chain[1])
    else:
        sign = t(sign).float()
        chain = cm.loss_and_grads(D['W'], D['b'], x, dat, D['D0'], D['SD0'], D['spread0'],
                                  sign=sign)
    t32 = rm.loss_and_grads(D['W'], D['b'], t(x), t(dat), t(D['D0']), t(D['SD0']),
                            np.float32(D['spread0']), sign=sign)
    l64, r64, dW64, db64 = rm.loss_and_grads(
        [w.double() for w in D['W']], [v.double() for v in D['b']], t(x).double(),
        t(dat).double(), t(D['D0']).double(), t(D['SD0']).double(), D['spread0'],
        sign=sign.double())
    out = dict(l64=float(l64), r64=r64, dW64=dW64, db64=db64, sign=sign, chain=chain,
               torch32=t32, res_err={}, gerr={})
    for name, m in (('chain', chain), ('torch', t32)):
        out['res_err'][name] = float((m[1].double() - r64).abs().max())
        out['gerr'][name] = [_relerr(g, g64) for l in range(len(dW64))
                             for g, g64 in ((m[2][l], dW64[l]), (m[3][l], db64[l]))]
    return out


def tolerances(M, nlayer):
    """-> res_tol, [tolerance of dW0, db0, dW1, ...] from machines()'s figures"""
    res_tol = MARGIN * max(M['res_err'].values())
    floor = MARGIN * (nlayer + 1) * 2.0**-24
    gtol = []
    for l in range(nlayer):
        for j, g64 in enumerate((M['dW64'][l], M['db64'][l])):
            tol = MARGIN * max(M['gerr']['chain'][2 * l + j], M['gerr']['torch'][2 * l + j])
            gtol.append(max(tol, floor) if g64.numel() < SMALL else tol)
    return res_tol, gtol


def tie_cap(rows, npix):
    return int(np.floor(TIE_SHARE * rows * npix + 1e-9))
