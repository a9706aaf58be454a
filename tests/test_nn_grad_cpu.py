"""The yardstick of rvs_template_nn_grad, pinned on the CPU before any kernel is held
against it -- tests/nn_grad_truth.py: its autograd Jacobian against central differences
of the float64 network -- and what needs no device of the feature itself: the entry
point's declaration, binding and argument check, and the opt-in of
engine.check_grad_scope.

Observed on the CPU (the 24 golden points): the Jacobian is within 1.3e-9 of the
central difference relative to the column's largest entry (bound 1e-7); the float32
forward-mode statement is within 4.6e-6 of the truth in the tangent metric of the GPU
test, 7.9e-7 in the template itself."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import nn_grad_truth as nt

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. declaration, binding, argument check -------------------------------------------
def test_header_and_binding_agree():
    """rvs_template_nn_grad is declared with the arguments of rvs_template_nn, bound
    with the same kinds and exported; the ABI number did not move"""
    from rvspecfit_amd import _lib
    hdr = open(os.path.join(REPO, 'include', 'rvsgpu.h')).read()
    assert int(re.search(r'#define RVS_ABI_VERSION (\d+)', hdr).group(1)) == 18
    txt = re.sub(r'/\*.*?\*/', ' ', hdr, flags=re.S)
    decl = {}
    for name in ('rvs_template_nn', 'rvs_template_nn_grad'):
        m = re.search(r'\bint\s+%s\s*\(([^;]*?)\)\s*;' % name, txt, flags=re.S)
        assert m, name + ' is not declared'
        decl[name] = [' '.join(a.split()) for a in m.group(1).split(',')]
    assert decl['rvs_template_nn_grad'] == decl['rvs_template_nn']
    assert 'rvs_template_nn_grad' in _lib.SIGNATURES
    assert _lib.SIGNATURES['rvs_template_nn_grad'] == _lib.SIGNATURES['rvs_template_nn']
    res, args = _lib.SIGNATURES['rvs_template_nn_grad']
    kinds = [ctypes.c_void_p if '*' in a else
             {'int': ctypes.c_int, 'uint32_t': ctypes.c_uint32}[a.split()[0]]
             for a in decl['rvs_template_nn_grad']]
    assert res is ctypes.c_int and args == kinds
    L = _lib.lib()
    assert L.rvs_abi_version() == 18
    assert hasattr(L, 'rvs_template_nn_grad')


def _call(dims, ndim=None, B=3, nullW=False):
    """the entry point on pointers that are never dereferenced on the device: every
    case here must be refused before any launch"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    a = ctypes.c_void_p(64)
    nl = len(dims) - 1
    Wp = (ctypes.c_void_p * nl)(*[None if nullW else 64] * nl)
    bp = (ctypes.c_void_p * nl)(*[64] * nl)
    dm = (ctypes.c_int32 * (nl + 1))(*dims)
    return L.rvs_template_nn_grad(a, B, dims[0] if ndim is None else ndim, 1, a, a, nl,
                                  ctypes.cast(Wp, ctypes.c_void_p),
                                  ctypes.cast(bp, ctypes.c_void_p),
                                  ctypes.cast(dm, ctypes.c_void_p), a, a, a, None)


def test_refused_shapes_answer_before_any_launch():
    """RVS_E_ARG (-1) for what the fused hidden stack does not cover"""
    assert _call([4, 64, 48, 64, 40, 333]) == -1        # a hidden width of 48
    assert _call([4, 48, 64, 40, 333]) == -1            # ... in the first layer
    assert _call([7, 64, 64, 40, 333]) == -1            # ndim = 7
    assert _call([4, 64, 333]) == -1                    # two layers
    assert _call([4] + [64] * 7 + [333]) == -1          # more than NH_MAXL hidden layers
    assert _call([4, 64, 288, 40, 333]) == -1           # wider than 256
    assert _call([4, 64, 64, 40, 333], ndim=3) == -1    # dims[0] != ndim
    assert _call([4, 64, 64, 40, 333], B=0) == -1
    assert _call([4, 64, 64, 40, 333], nullW=True) == -1


def test_library_names_the_refused_shape():
    """TemplateLibrary.check_nn_grad_scope: a ValueError that names the network"""
    from rvspecfit_amd.library import TemplateLibrary
    lib = TemplateLibrary.__new__(TemplateLibrary)
    lib.name, lib.ndim = 'x', 4
    lib.nn_dims = np.array([4, 64, 64, 64, 40, 333], dtype=np.int32)
    lib.check_nn_grad_scope()
    lib.nn_dims = np.array([4, 64, 48, 64, 40, 333], dtype=np.int32)
    with pytest.raises(ValueError, match='multiple of 32'):
        lib.check_nn_grad_scope()
    lib.ndim, lib.nn_dims = 7, np.array([7, 64, 64, 333], dtype=np.int32)
    with pytest.raises(ValueError, match='ndim = 7'):
        lib.check_nn_grad_scope()


# ---- 2. the opt-in of the scope check ------------------------------------------------
def test_scope_check_admits_mlp_libraries_only_when_asked():
    from rvspecfit_amd import engine

    class Arm:
        name, G, resol = 'gold_b', 1, None

    class Batch:
        arms = [Arm]

    class Lib:
        ndim, kind = 4, 'nn'

    libs = {'gold_b': Lib}
    # (today's words, whatever the other arguments)
    msg = ('the analytic gradient needs regular-grid (polylinear) or Delaunay '
           'libraries, gold_b is a nn library')
    for kw in (dict(), dict(vsini_grad=True), dict(nn_gradient=False)):
        with pytest.raises(ValueError) as e:
            engine.check_grad_scope(Batch, libs, 10, **kw)
        assert str(e.value) == msg
    engine.check_grad_scope(Batch, libs, 10, nn_gradient=True)
    engine.check_grad_scope(Batch, libs, 10, vsini_grad=True, nn_gradient=True)
    for kind in ('regulargrid', 'triangulation'):
        Lib.kind = kind
        engine.check_grad_scope(Batch, libs, 10, nn_gradient=True)
    Lib.kind, Lib.ndim = 'nn', 6
    engine.check_grad_scope(Batch, libs, 10, nn_gradient=True)
    with pytest.raises(ValueError, match=r'vsini.*ndim = 6'):
        engine.check_grad_scope(Batch, libs, 10, vsini_grad=True, nn_gradient=True)
    Lib.kind, Lib.ndim = 'other', 4
    with pytest.raises(ValueError, match='regular-grid'):
        engine.check_grad_scope(Batch, libs, 10, nn_gradient=True)


# ---- 3. the truth ---------------------------------------------------------------------
def test_jacobian_against_central_differences():
    """dt/dx of the float64 network: central differences with step h = 1e-6 in mapped
    units.  Truncation h^2 / 6 |t'''| ~ 2e-13 |t| for a network whose derivatives are of
    order one; rounding 2 eps |t| / (2 h) = 1.1e-10 |t| with |t| ~ 1 and the columns'
    largest entries 0.05 ... 1: 1e-7 of the column's largest entry leaves a decade and
    a half."""
    net = nt.network()
    p = net['params']
    t, jac = nt.jacobian64(net, p)
    jx = jac / nt.input_scale(net, p)[:, :, None]          # back to d/dx
    x0 = torch.as_tensor(nt.mapped(net, p))
    h = 1e-6
    worst = 0.0
    for k in range(nt.NDIM):
        e = torch.zeros_like(x0)
        e[:, k] = h
        fd = (nt.template64(net, x0 + e) - nt.template64(net, x0 - e)).numpy() / (2 * h)
        err = np.abs(fd - jx[:, k]).max(axis=1) / np.abs(jx[:, k]).max(axis=1)
        print('column %d: largest |central difference - autograd| %.3g of the column\'s '
              'largest entry' % (k, err.max()))
        worst = max(worst, float(err.max()))
    assert worst <= 1e-7
    # the template of the truth is the golden one (float32 network, float64 exp)
    gold = np.load(os.path.join(nt.GOLD, 'nn_case.npz'))['out']
    assert np.abs(t / gold - 1).max() < 3e-6


def test_float32_statement_is_close_to_the_truth():
    """forward32 -- the float32 network with forward-mode tangents, the quantity the
    GPU test's bound is four times of -- agrees with the truth to float32 rounding
    through five layers: below 1e-4 in the tangent metric (observed 4.6e-6), and its
    clipped columns have zero tangents"""
    net = nt.network()
    p = nt.points(net, 27)
    t, jac = nt.jacobian64(net, p)
    t32, jac32 = nt.forward32(net, p)
    m = nt.tangent_metric(jac32, jac)
    print('float32 statement: tangent metric max %.3g, template max rel %.3g'
          % (m.max(), np.abs(t32 / t - 1).max()))
    assert m.shape == (27, nt.NDIM) and m.max() < 1e-4
    hot = dict(net, b=[b.copy() for b in net['b']])
    hot['b'][-1][5], hot['b'][-1][100] = 400.0, -400.0
    t32, jac32 = nt.forward32(hot, p)
    assert (t32[:, 5] == np.exp(300.0)).all() and (t32[:, 100] == np.exp(-300.0)).all()
    assert not jac32[:, :, [5, 100]].any() and jac32[:, :, 6].all()
