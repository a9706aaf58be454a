"""The MLP trainer's kernels (csrc/nn_train.hip through rvspecfit_amd.nn.
train_interpolator.Trainer) at every network and batch shape of tests/nn_train_shapes.py:
tile edges along M, N and K, several tiles along a hidden width, db from blocks with
m0 > 0, 2 and 8 layers, one chunk and 72 chunks of the output layer's dA, 198 loss
partials, every stated limit, every extent 1.

  a  residual, loss and every gradient tensor against the float64 torch machine driven by
     the device's signs.  Tolerances from two float32 machines on the CPU at the case's
     own shape (nn_train_shapes.tolerances): none is taken from the device.
  b  the forward pass does not depend on the launch: the rows of a batch one at a time,
     in reversed order and through eval_rows have the batch's bits.
  c  indices outside [0, T) read the clamped row, bit for bit.
  d  rvs_nn_train_epoch is its steps (grad + adam_step), bit for bit, and repeats.
  e  the step losses of those epochs against the float64 machine.
  f  Adam at other tensor lists (16 tensors, 1-element tensors) against torch's
     arithmetic on the CPU.

Largest errors of the first MI355X run, tolerance in brackets (pytest -s prints them).
Residual: largest |r - r64|; gradients: the range of the norm-relative errors of the
case's tensors, then the tensor nearest its tolerance; flips: residuals whose sign differs
from float64's, all of them near-ties.
  case           residual           loss               gradients            nearest          flips
  default-net    6.1e-8 (2.4e-7)    1.2e-9 (4.3e-6)    9.3e-8 .. 5.4e-7     db0 3.7e-7 (1.4e-6)  0
  odd            6.4e-8 (2.6e-7)    2.4e-9 (4.7e-6)    1.0e-7 .. 3.3e-7     db1 3.3e-7 (1.2e-6)  0
  two-layers     6.6e-8 (2.8e-7)    6.9e-10 (4.3e-6)   4.6e-7 .. 9.2e-7     db0 4.7e-7 (1.9e-6)  0
  max-width      7.3e-8 (2.9e-7)    2.3e-9 (4.4e-6)    3.4e-7 .. 7.5e-7     db1 3.4e-7 (1.2e-6)  0
  wide-wide      6.2e-8 (2.5e-7)    3.0e-9 (4.3e-6)    1.0e-7 .. 3.9e-7     dW3 3.0e-7 (1.2e-6)  0
  deep           6.0e-8 (2.5e-7)    3.4e-9 (5.0e-6)    1.1e-7 .. 6.3e-7     db1 6.3e-7 (2.3e-6)  0
  many-partials  6.5e-8 (2.6e-7)    4.2e-10 (4.6e-6)   1.2e-7 .. 2.1e-7     db0 2.1e-7 (8.1e-7)  0
  npix-max       6.3e-8 (2.5e-7)    5.2e-10 (4.3e-6)   1.1e-7 .. 1.8e-7     dW2 1.5e-7 (6.1e-7)  1
  exact          6.2e-8 (2.7e-7)    7.5e-10 (4.9e-6)   1.1e-7 .. 3.1e-7     dW0 1.9e-7 (7.5e-7)  0
  chunk-127      6.6e-8 (2.7e-7)    6.5e-9 (4.9e-6)    1.0e-7 .. 2.2e-7     db0 2.2e-7 (8.9e-7)  0
  chunk-128      6.2e-8 (2.6e-7)    1.7e-9 (4.6e-6)    8.2e-8 .. 1.8e-7     dW0 1.8e-7 (7.4e-7)  0
  ones-3         1.2e-8 (5.0e-8)    2.2e-7 (8.9e-7)    4e-9 .. 4.9e-7       dW0 4.7e-7 (1.9e-6)  0
  ones-2         5.0e-8 (2.0e-7)    9.0e-7 (3.6e-6)    5.3e-8 .. 4.0e-7     dW0 3.8e-7 (1.9e-6)  0
  width-one      6.3e-8 (2.5e-7)    7.6e-9 (4.2e-6)    9.8e-8 .. 2.8e-7     db3 9.8e-8 (3.9e-7)  0
  one-row        5.9e-8 (2.4e-7)    3.9e-8 (4.2e-6)    3.2e-8 .. 3.1e-7     dW2 1.8e-7 (7.0e-7)  0
On `ones` the floor 4 (nlayer + 1) 2^-24 of the small tensors was not needed: every
tensor lay within 4 x the CPU machines' own error.
e: step losses 2.6e-11 .. 3.3e-8 from float64 (tolerance 3.7e-7 .. 3.9e-7), loss_accum
4.8e-11 .. 1.6e-8 relative (4.8e-7).  f: weights within 0.97 ulp of |w| + lr, 1.83 on the
second update of `odd`, 0 on `ones`; moments equal.  b, c, d: bits.
Teeth, once, on a scratch build with `gk < kend - 1` in nt_fetch (the last k of every
product dropped): a failed on every case (residual, loss and every gradient tensor), c
through its residual check and e on every epoch; b, d and f passed, as they must -- they
compare the device with itself.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_train_shapes as shapes  # noqa: E402
from refmachines import nn_train_torch as rm  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
LR = 1e-3
INT_MAX = 2**31 - 1


def _trainer(D, batch=100):
    from rvspecfit_amd.nn import train_interpolator as ti
    return ti.Trainer(D['dats'], D['x'], D['W'], D['b'], D['D0'], D['SD0'], D['spread0'],
                      batch=batch)


def _state(tr):
    return [t.cpu().clone() for t in tr.W + tr.b + tr.mW + tr.mb + tr.vW + tr.vb]


def _same_bits(a, b):
    """equal as bit patterns (a NaN equals itself, -0 differs from +0)"""
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype
    itype = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    return torch.equal(a.view(itype), b.view(itype))


# ---------------------------------------------------------------------------
# a. gradients against float64
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', [c.name for c in shapes.CASES])
def test_gradients_against_float64(name):
    c = shapes.BY_NAME[name]
    D = shapes.case_data(name)
    nl = len(c.dims) - 1
    tr = _trainer(D)
    loss, dW, db, res = tr.grad(D['idx'], resid=True)
    res = res.cpu()
    assert res.shape == (c.rows, c.dims[-1])
    M = shapes.machines(D, sign=torch.sign(res))
    res_tol, gtol = shapes.tolerances(M, nl)
    r64 = M['r64']
    err = float((res.double() - r64).abs().max())
    print('%s: residual error %.3g (tolerance %.3g)' % (name, err, res_tol))
    lerr = abs(float(loss.item()) - M['l64'])
    print('%s: loss %.9g, float64 %.9g: error %.3g (tolerance %.3g)'
          % (name, float(loss.item()), M['l64'], lerr, res_tol / D['spread0']))
    flip = torch.sign(res).double() != torch.sign(r64)
    tie = r64.abs() < shapes.TIE_FACTOR * res_tol
    print('%s: sign flips %d, near-ties %d' % (name, int(flip.sum()), int(tie.sum())))
    bad = []
    if not err <= res_tol:
        bad.append('residual')
    if not lerr <= res_tol / D['spread0']:
        bad.append('loss')
    if bool((flip & ~tie).any()):
        bad.append('signs')
    for l in range(nl):
        for j, (g, g64) in enumerate(((dW[l], M['dW64'][l]), (db[l], M['db64'][l]))):
            assert g.shape == g64.shape
            e = float((g.cpu().double() - g64).norm() / g64.norm())
            print('%s: d%s%d %.3g (tolerance %.3g)' % (name, 'Wb'[j], l, e,
                                                       gtol[2 * l + j]))
            if not e <= gtol[2 * l + j]:
                bad.append('d%s%d' % ('Wb'[j], l))
    assert not bad, bad


# ---------------------------------------------------------------------------
# b. the forward pass does not depend on the launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['odd', 'default-net', 'many-partials'])
def test_forward_does_not_depend_on_the_launch(name):
    """An output's chain runs over k only, so its value cannot depend on which tile or
    lane computed it: the same rows in a batch, alone, in reversed order, and through
    eval_rows (R = residual + row, compared with the same float32 sum of the batch's
    residual) give the same bits."""
    D = shapes.case_data(name)
    tr = _trainer(D)
    idx = D['idx']
    res = tr.grad(idx, backward=False, resid=True)[3]
    rev = tr.grad(idx[::-1].copy(), backward=False, resid=True)[3]
    assert _same_bits(rev.flip(0), res)
    for i, row in enumerate(idx):
        one = tr.grad([int(row)], backward=False, resid=True)[3]
        assert _same_bits(one[0], res[i]), (name, i)
    loss, pred = tr.eval_rows(idx, pred=True)
    assert _same_bits(pred, res + tr.dats[torch.as_tensor(idx).to(tr.device)])
    want = float(tr.grad(idx, backward=False)[0].item())
    assert abs(loss - want) <= 4 * np.finfo(np.float64).eps * want   # (loss n) / n


def test_eval_rows_over_two_chunks():
    """eval_rows over 1100 rows of `odd` (1024 + 76): the residual bits of other
    partitions of the same rows (550 + 550, and rows alone)"""
    c = shapes.BY_NAME['odd']
    D = shapes.data(c.dims, c.rows, T=1100)
    tr = _trainer(D)
    rows = np.random.default_rng(2).permutation(1100)
    loss, pred = tr.eval_rows(rows, pred=True)
    assert pred.shape == (1100, c.dims[-1])
    dat = tr.dats[torch.as_tensor(rows).to(tr.device)]
    halves = [tr.grad(rows[i:i + 550], backward=False, resid=True) for i in (0, 550)]
    res = torch.cat([h[3] for h in halves])
    assert _same_bits(pred, res + dat)
    for i in (0, 1023, 1024, 1099):
        one = tr.grad([int(rows[i])], backward=False, resid=True)[3]
        assert _same_bits(pred[i], one[0] + dat[i])
    # the mean over all rows from the chunks' means, in float64
    want = sum(float(h[0].item()) * 550 for h in halves) / 1100
    assert abs(loss - want) <= 4 * np.finfo(np.float64).eps * want


# ---------------------------------------------------------------------------
# c. clamped indices
# ---------------------------------------------------------------------------
def test_indices_are_clamped():
    D = shapes.case_data('odd')
    T = D['T']
    idx = D['idx'].astype(np.int64).copy()
    clamped = idx.copy()
    # first row, an inner one, the last of the first tile, the one row of the second
    for pos, (bad, good) in zip((0, 17, 63, 64, 30, 31),
                                ((-3, 0), (T + 5, T - 1), (INT_MAX, T - 1), (-3, 0),
                                 (T, T - 1), (-INT_MAX - 1, 0))):
        idx[pos], clamped[pos] = bad, good
    tr = _trainer(D)
    got = tr.grad(idx, resid=True)
    want = tr.grad(clamped, resid=True)
    assert _same_bits(got[0], want[0])
    assert _same_bits(got[3], want[3])
    for g, w in zip(got[1] + got[2], want[1] + want[2]):
        assert _same_bits(g, w)
    # and the clamped rows are those rows: against the float64 machine's residual
    M = shapes.machines(D, idx=clamped)
    res_tol = shapes.tolerances(M, len(D['dims']) - 1)[0]
    assert float((got[3].cpu().double() - M['r64']).abs().max()) <= res_tol


# ---------------------------------------------------------------------------
# d, e. an epoch is its steps; its losses against float64
# ---------------------------------------------------------------------------
EPOCHS = {      # case: T, batch
    'odd': (150, 64),           # 64 + 64 + 22
    'exact': (128, 64),         # no short batch
    'deep': (70, 1024),         # one short batch, 16 tensors in the Adam launch
    'default-net': (250, 100),  # 100 + 100 + 50
}


@pytest.fixture(scope='module', params=sorted(EPOCHS))
def epoch_run(request):
    """one epoch through rvs_nn_train_epoch from the initial state: -> name, data, perm,
    batch, state afterwards, step losses, loss_accum"""
    name = request.param
    T, batch = EPOCHS[name]
    c = shapes.BY_NAME[name]
    D = shapes.data(c.dims, c.rows, T=T)
    perm = np.random.default_rng(3).permutation(T)
    tr = _trainer(D, batch=batch)
    sl = tr.epoch(perm, LR, step_loss=True)
    return dict(name=name, D=D, perm=perm, batch=batch, state=_state(tr), sl=sl.cpu(),
                accum=tr.loss_accum.cpu().clone(), steps=tr.steps)


def test_an_epoch_is_its_steps(epoch_run):
    """Weights, biases, both moments and the step losses of a loop of grad + adam_step
    over the same batches: the epoch's bits.  rvs_nn_train_grad has no loss_accum; the
    epoch's is the float64 sum, in step order, of sum|r| / spread0 of each step, and an
    epoch of ONE batch returns exactly that term (0 + t = t), so a third trainer run
    batch by batch through one-batch epochs gives the terms, summed here in float64 in
    the same order.  Then the epoch once more from the initial state: the same bits."""
    E = epoch_run
    D, perm, batch = E['D'], E['perm'], E['batch']
    nstep = (len(perm) + batch - 1) // batch
    assert E['steps'] == nstep == len(E['sl'])
    tr = _trainer(D, batch=batch)
    tr1 = _trainer(D, batch=batch)
    accum = torch.zeros(1, dtype=torch.float64)
    for s in range(nstep):
        idx = perm[s * batch:(s + 1) * batch]
        loss, dW, db, _ = tr.grad(idx)
        tr.adam_step(dW, db, LR)
        assert _same_bits(loss.cpu()[0], E['sl'][s]), (E['name'], s)
        sl1 = tr1.epoch(idx, LR, step_loss=True)
        assert _same_bits(sl1.cpu()[0], E['sl'][s])
        accum = accum + tr1.loss_accum.cpu()
    for k, (a, b, b1) in enumerate(zip(E['state'], _state(tr), _state(tr1))):
        assert _same_bits(a, b), (E['name'], 'tensor %d of W b mW mb vW vb' % k)
        assert _same_bits(a, b1), (E['name'], 'tensor %d of W b mW mb vW vb' % k)
    assert _same_bits(accum, E['accum'])
    again = _trainer(D, batch=batch)
    sl = again.epoch(perm, LR, step_loss=True)
    assert _same_bits(sl, E['sl'])
    assert _same_bits(again.loss_accum, E['accum'])
    for a, b in zip(E['state'], _state(again)):
        assert _same_bits(a, b)


def test_epoch_losses_against_float64(epoch_run):
    """nn_train_torch.train_epoch in float64: every step's loss within 4 eps32 loss (the
    bound tests/test_nn_train_cpu.py holds the float32 machine to), loss_accum within
    the same relative bound of sum loss_s rows_s npix.  The weights after the epoch are
    not compared with float64: Adam's first updates are +-lr whatever the gradient's
    size, and a gradient element near zero flips the update's sign."""
    E = epoch_run
    D, perm, batch = E['D'], E['perm'], E['batch']
    t = lambda a: torch.as_tensor(a).double()  # noqa: E731
    W, b = [w.double().clone() for w in D['W']], [v.double().clone() for v in D['b']]
    accum, steps = rm.train_epoch(W, b, rm.Adam(W + b), t(D['dats']), t(D['x']), perm, batch,
                                  LR, t(D['D0']), t(D['SD0']), D['spread0'])
    bad = []
    for s, (got, want) in enumerate(zip(E['sl'].numpy(), steps)):
        print('%s step %d: %.9g, float64 %.9g: error %.3g (tolerance %.3g)'
              % (E['name'], s + 1, got, want, abs(got - want), 4 * EPS * want))
        if not abs(got - want) <= 4 * EPS * want:
            bad.append(s)
    assert len(steps) == len(E['sl'])
    got = float(E['accum'][0])
    print('%s loss_accum: %.9g, float64 %.9g: error %.3g (tolerance %.3g)'
          % (E['name'], got, accum, abs(got - accum), 4 * EPS * accum))
    assert not bad, bad
    assert abs(got - accum) <= 4 * EPS * accum


# ---------------------------------------------------------------------------
# f. Adam at other tensor lists
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['deep', 'odd', 'ones-3', 'ones-2'])
def test_adam_at_other_tensor_lists(name):
    """Two adam_step calls fed the device's own gradients of two batches, against
    nn_train_torch.Adam in float32 on the CPU fed the same gradient bits: the moments
    equal bit for bit, the weights within 2 ulp of |w| + lr after each update -- the
    bounds test_adam_against_torch holds for updates 1 and 2."""
    D = shapes.case_data(name)
    rows = D['rows']
    batches = [D['idx'], np.random.default_rng(1).permutation(D['T'])[::-1][:rows].copy()]
    tr = _trainer(D)
    P = [w.clone() for w in D['W']] + [v.clone() for v in D['b']]
    opt = rm.Adam(P)
    for s, idx in enumerate(batches):
        _, dW, db, _ = tr.grad(idx)
        tr.adam_step(dW, db, LR)
        opt.step([g.cpu() for g in dW + db], LR)
        worst = 0.0
        for k, (p, m, v) in enumerate(zip(tr.W + tr.b, tr.mW + tr.mb, tr.vW + tr.vb)):
            assert _same_bits(m, opt.m[k]), (name, s, k)
            assert _same_bits(v, opt.v[k]), (name, s, k)
            want = opt.p[k].numpy()
            worst = max(worst, float(np.max(np.abs(p.cpu().numpy() - want) /
                                            (np.abs(want) + LR))) / EPS)
        print('%s update %d: weights within %.2f ulp of |w| + lr' % (name, s + 1, worst))
        assert worst <= 2
