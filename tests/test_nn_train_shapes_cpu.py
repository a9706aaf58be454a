"""What tests/test_nn_train_shapes_gpu.py stands on, checked without a device: the
chain machine (tests/refmachines/nn_train_chain.py) is a float32 evaluation of the
training step -- it reproduces the fixture's gradients as the torch machine does, and its
`chain` is a float32 dot product -- and at every case of tests/nn_train_shapes.py both
float32 machines lie where the tolerances assume them, with no more near-ties of the
residual than the conditioning cap allows.  The figures printed here (pytest -s) are what
the device test's tolerances are made of."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_train_shapes as shapes  # noqa: E402
from refmachines import nn_train_chain as cm  # noqa: E402
from refmachines import nn_train_torch as rm  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
NL = 5
EPS = float(np.finfo(np.float32).eps)


@pytest.mark.parametrize('nb', [32, 100])
def test_chain_machine_gives_the_fixture_s_gradients(nb):
    """the bound test_refmachine_gradients holds the torch machine to"""
    G = dict(np.load(os.path.join(GOLD, 'nn_train_cases.npz')))
    F = rm.fixture_rows()
    idx, pre = G['idx%d' % nb], 'g%d_' % nb
    W, b = rm.init_weights(rm.FIXTURE_DIMS)
    loss, _, dW, db = cm.loss_and_grads(W, b, F['x'][idx], F['dats'][idx], F['D0'],
                                        F['SD0'], np.float32(F['spread0']))
    assert abs(float(loss) - G[pre + 'loss']) <= 4 * EPS * G[pre + 'loss']
    seen = 0
    for l in range(NL):
        for j, g in enumerate((dW[l], db[l])):
            key = pre + 'd%s%d' % ('Wb'[j], l)
            if key not in G:
                continue
            seen += 1
            e = np.linalg.norm(g.numpy() - G[key]) / np.linalg.norm(G[key])
            print('%s: %.3g (bound %.3g)' % (key, e, 2 * G[pre + 'gerr'][2 * l + j]))
            assert e <= 2 * G[pre + 'gerr'][2 * l + j], (key, e)
    assert seen


def test_chain_is_a_float32_dot_product():
    """against float64 A B^T at K = 100, M and N one past a tile and a slab: per element
    K 2^-24 sum |a| |b|, the standard bound of a float32 dot product of length K"""
    rng = np.random.default_rng(11)
    A = rng.normal(size=(65, 100)).astype(np.float32)
    B = rng.normal(size=(33, 100)).astype(np.float32)
    C = cm.chain(A, B)
    assert C.dtype == np.float32 and C.shape == (65, 33)
    want = A.astype(np.float64) @ B.astype(np.float64).T
    bound = 100 * 2.0**-24 * (np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64).T)
    share = np.max(np.abs(C - want) / bound)
    print('largest share of the bound: %.3g' % share)
    assert share <= 1
    assert np.any(C != want.astype(np.float32))    # and it is not float64 in disguise


@pytest.mark.parametrize('name', [c.name for c in shapes.CASES])
def test_machines_and_conditioning(name):
    """Both float32 machines against the float64 machine, the backward passes driven by
    the chain machine's signs; the conditioning cap: at most floor(1e-4 rows npix)
    residuals of the float64 machine within 8 res_tol of zero, and the chain machine's
    signs differ from float64's only there."""
    c = shapes.BY_NAME[name]
    D = shapes.case_data(name)
    nl = len(c.dims) - 1
    M = shapes.machines(D)
    res_tol, gtol = shapes.tolerances(M, nl)
    print('%s %s x %d rows: residual error chain %.3g torch %.3g -> res_tol %.3g; loss '
          '%.6g' % (name, list(c.dims), c.rows, M['res_err']['chain'],
                    M['res_err']['torch'], res_tol, M['l64']))
    for l in range(nl):
        for j in range(2):
            i = 2 * l + j
            print('  d%s%d: chain %.3g torch %.3g -> tolerance %.3g'
                  % ('Wb'[j], l, M['gerr']['chain'][i], M['gerr']['torch'][i], gtol[i]))
    for i in range(2 * nl):
        for m in ('chain', 'torch'):
            assert np.isfinite(M['gerr'][m][i])
    assert all(t > 0 for t in gtol) and res_tol > 0
    # a float32 residual of values near 1: a few ulp of 1, not more
    assert res_tol <= 4 * 16 * EPS
    r64 = M['r64']
    tie = r64.abs() < shapes.TIE_FACTOR * res_tol
    cap = shapes.tie_cap(c.rows, c.dims[-1])
    print('  near-ties %d of %d (cap %d)' % (int(tie.sum()), r64.numel(), cap))
    assert int(tie.sum()) <= cap
    flip = M['sign'].double() != torch.sign(r64)
    assert not bool((flip & ~tie).any())
