"""CPU-side checks of the MLP trainer: the torch restatement of the loop
(tests/refmachines/nn_train_torch.py) reproduces tests/golden/nn_train_cases.npz, the
restated plateau scheduler gives torch's rates, header / bindings / library agree on
the new entry points, and every stated limit is an argument error before any launch."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refmachines import nn_train_torch as rm  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, 'tests', 'golden')
NL = 5
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope='module')
def G():
    return dict(np.load(os.path.join(GOLD, 'nn_train_cases.npz')))


@pytest.fixture(scope='module')
def T32():
    F = rm.fixture_rows()
    t = {k: torch.as_tensor(F[k]) for k in ('dats', 'x', 'D0', 'SD0')}
    t['spread0'] = np.float32(F['spread0'])
    return t


def test_initial_weights_are_the_reference_class_s(G):
    W, b = rm.init_weights(rm.FIXTURE_DIMS)
    for l in range(NL):
        assert np.array_equal(W[l].numpy(), G['W%d' % l])
        assert np.array_equal(b[l].numpy(), G['b%d' % l])


@pytest.mark.parametrize('nb', [32, 100])
def test_refmachine_gradients(G, T32, nb):
    """loss and gradients of both batches to float32 round-off: a few times the error
    the fixture's float32 gradients themselves have against float64 (gerr), since two
    float32 evaluations may differ by the sum of their errors"""
    idx, pre = G['idx%d' % nb], 'g%d_' % nb
    W, b = rm.init_weights(rm.FIXTURE_DIMS)
    loss, _, dW, db = rm.loss_and_grads(W, b, T32['x'][idx], T32['dats'][idx], T32['D0'],
                                        T32['SD0'], T32['spread0'])
    assert abs(float(loss) - G[pre + 'loss']) <= 4 * EPS * G[pre + 'loss']
    for l in range(NL):
        for j, g in enumerate((dW[l], db[l])):
            key = pre + 'd%s%d' % ('Wb'[j], l)
            if key not in G:
                continue
            e = np.linalg.norm(g.numpy() - G[key]) / np.linalg.norm(G[key])
            assert e <= 2 * G[pre + 'gerr'][2 * l + j], (key, e)


def test_refmachine_ten_steps(G, T32):
    W, b = rm.init_weights(rm.FIXTURE_DIMS)
    opt = rm.Adam(W + b)
    perms = G['step_perms'].astype(np.int64)
    losses = []
    for p in perms:
        losses += rm.train_epoch(W, b, opt, T32['dats'], T32['x'], p, 100, 1e-3,
                                 T32['D0'], T32['SD0'], T32['spread0'])[1]
        if len(losses) >= 10:
            break
    # steps taken: 3 per permutation; the fixture stopped after 10
    for s in (0, 1, 9):
        tol = 4 * abs(G['step_loss'][s] - G['step_loss64'][s])
        assert abs(losses[s] - G['step_loss'][s]) <= tol, s


def test_refmachine_adam_is_torch_s(G):
    """the restated update on the fixture's gradients of layers 0 and 3: torch's Adam's
    weights after 1, 2 and 10 steps within 2 ulp of |w| + lr"""
    lay = (0, 3)
    P = [torch.as_tensor(G['%s%d' % (n, l)]).clone() for l in lay for n in 'Wb']
    opt = rm.Adam(P)
    for s in range(10):
        opt.step([torch.as_tensor(G['adam_d%s%d_s%d' % (n, l, s)]) for l in lay
                  for n in 'Wb'], 1e-3)
        if s + 1 in (1, 2, 10):
            k = 0
            for l in lay:
                for n in 'Wb':
                    want = G['adam_p_%s%d_n%d' % (n, l, s + 1)]
                    e = np.max(np.abs(P[k].numpy() - want) / (np.abs(want) + 1e-3))
                    assert e <= 2 * EPS, (n, l, s, e / EPS)
                    k += 1


def _torch_rates(curve, patience):
    opt = torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=1e-3)
    ts = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=patience,
                                                    eps=1e-9, threshold=1e-5)
    out = []
    for v in curve:
        ts.step(v)
        out.append(opt.param_groups[0]['lr'])
    return out


def test_plateau_scheduler_is_torch_s(G):
    from rvspecfit_amd.nn.train_interpolator import PlateauScheduler
    # ties, an improvement of exactly the threshold's size and one just beyond it,
    # and enough stalls to bring the rate under eps
    hand = [10., 10., 9., 9., 9. * (1 - 1e-5), 9. * (1 - 1.0001e-5), 9., 9., 9., 8.] + \
        [8.] * 120
    curves = [(c, 3) for c in G['conv_accum']] + [(hand, 2), (hand, 0)]
    for curve, patience in curves:
        s = PlateauScheduler(1e-3, patience=patience)
        assert [s.step(v) for v in curve] == _torch_rates(curve, patience)
    for k in range(3):    # and the fixture's own record of the rates
        s = PlateauScheduler(1e-3, patience=3)
        got = [1e-3] + [s.step(v) for v in G['conv_accum'][k]][:-1]
        assert got == list(G['conv_lr'][k])


@pytest.fixture(scope='module')
def lib():
    from rvspecfit_amd import _lib
    return _lib.lib()


NEW = ('rvs_nn_train_work_size', 'rvs_nn_train_grad', 'rvs_nn_adam_step',
       'rvs_nn_train_epoch')


def test_entry_points_and_version(lib):
    from rvspecfit_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
    assert lib.rvs_abi_version() == 18 == _lib.ABI_VERSION
    code = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    for name in NEW:
        m = re.search(r'\b%s\s*\(([^;]*?)\)\s*;' % name, code, flags=re.S)
        assert m, name
        assert len(m.group(1).split(',')) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert int(re.search(r'#define RVS_NN_TRAIN_MAX_NPIX (\d+)', hdr).group(1)) == \
        __import__('rvspecfit_amd.make_interpol').make_interpol.MAX_NPIX


def _dims(*d):
    return np.array(d, dtype=np.int32)


def test_limits_are_argument_errors(lib):
    ws = lambda T, B, d: lib.rvs_nn_train_work_size(T, B, len(d) - 1, d.ctypes.data)  # noqa: E731
    ok = _dims(4, 64, 64, 64, 40, 977)
    assert ws(254, 100, ok) > 0
    bad = [(254, 0, ok), (254, 1025, ok), (0, 100, ok),
           (254, 100, _dims(9, 64, 40, 977)),       # ndim <= 8
           (254, 100, _dims(0, 64, 40, 977)),
           (254, 100, _dims(4, 977)),               # nlayer >= 2
           (254, 100, _dims(4, 2048, 40, 977)),     # widths
           (254, 100, _dims(4, 64, 0, 977)),
           (254, 100, _dims(4, 64, 40, 9217)),      # make_interpol.MAX_NPIX
           (254, 100, _dims(4, 8, 8, 8, 8, 8, 8, 8, 8, 977))]   # nlayer <= 8
    for T, B, d in bad:
        assert ws(T, B, d) == -1, (T, B, list(d))
    # the entry points refuse the same before touching a pointer (all NULL here)
    n = len(ok) - 1
    p8 = (ctypes.c_void_p * 8)()
    arr = ctypes.cast(p8, ctypes.c_void_p)
    assert lib.rvs_nn_train_grad(None, None, 254, None, 100, n, ok.ctypes.data, arr, arr,
                                 None, None, 1.0, None, None, None, None, None,
                                 None) == -1
    one = np.ones(4)
    q = one.ctypes.data
    for i in range(8):
        p8[i] = q
    d9 = _dims(9, 64, 40, 977)
    assert lib.rvs_nn_train_grad(q, q, 254, q, 100, 3, d9.ctypes.data, arr, arr, q, q, 1.0,
                                 None, None, q, None, q, None) == -1
    assert lib.rvs_nn_train_grad(q, q, 254, q, 1025, n, ok.ctypes.data, arr, arr, q, q,
                                 1.0, None, None, q, None, q, None) == -1
    assert lib.rvs_nn_train_grad(q, q, 254, q, 100, n, ok.ctypes.data, arr, arr, q, q,
                                 0.0, None, None, q, None, q, None) == -1   # spread0
    assert lib.rvs_nn_adam_step(n, ok.ctypes.data, arr, arr, arr, arr, arr, arr, arr, arr,
                                1e-3, 0, None) == -1                        # step >= 1
    assert lib.rvs_nn_adam_step(1, ok.ctypes.data, arr, arr, arr, arr, arr, arr, arr, arr,
                                1e-3, 1, None) == -1
    assert lib.rvs_nn_train_epoch(q, q, 254, q, 254, 1025, n, ok.ctypes.data, arr, arr,
                                  arr, arr, arr, arr, q, q, 1.0, 1e-3, 0, q, None, q,
                                  None) == -1
    assert lib.rvs_nn_train_epoch(q, q, 254, q, 0, 100, n, ok.ctypes.data, arr, arr, arr,
                                  arr, arr, arr, q, q, 1.0, 1e-3, 0, q, None, q,
                                  None) == -1


def test_cpu_switch_is_refused():
    from rvspecfit_amd import _lib
    from rvspecfit_amd.nn import train_interpolator as ti
    with pytest.raises(_lib.RvsGpuError, match='no CPU'):
        ti.main(['--cpu', '--setup', 'x'])
    a = ti.make_parser().parse_args(['--setup', 'x', '--batch_on_device'])
    assert a.batch_on_device and a.batch == 100 and a.npc == 200 and a.patience == 20
    assert ti.network_dims(4, 2, 256, 200, 6215) == [4, 256, 256, 256, 200, 6215]
