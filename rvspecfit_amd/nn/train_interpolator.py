"""rvs_train_nn_interpolator (nn/train_interpolator.py) on the device: trains the MLP
that rvs_template_nn evaluates from the rows make_interpol.build_specs produces.

A whole epoch -- every batch's forward pass, L1 loss, backward pass and Adam update --
runs inside librvsgpu.so (rvs_nn_train_epoch, csrc/nn_train.hip); this module keeps the
per-epoch decisions: the order of the rows, the learning-rate schedule, when to stop,
checkpoints.  The one host synchronisation per epoch is the 8-byte read of lossAccum.
There is no CPU path.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

from .. import _lib

SEED = 343432323            # train_interpolator.py:171
CHECKPOINT_EVERY = 32       # train_interpolator.py:352
MAX_BATCH = 1024            # RVS_NN_TRAIN_MAX_B


class PlateauScheduler:
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', threshold_mode='rel',
    cooldown=0, min_lr=0) as getSchedOptim sets it up (train_interpolator.py:42-47):
    factor 0.5, eps 1e-9, threshold 1e-5"""

    def __init__(self, lr, patience=20, factor=0.5, eps=1e-9, threshold=1e-5):
        self.lr, self.patience, self.factor = float(lr), patience, factor
        self.eps, self.threshold = eps, threshold
        self.best, self.num_bad = float('inf'), 0

    def step(self, metric):
        metric = float(metric)
        if metric < self.best * (1.0 - self.threshold):
            self.best, self.num_bad = metric, 0
        else:
            self.num_bad += 1
        if self.num_bad > self.patience:
            new = self.lr * self.factor
            if self.lr - new > self.eps:
                self.lr = new
            self.num_bad = 0
        return self.lr


def network_dims(indim, nlayers, width, npc, npix):
    """NNInterpolator.initLayers (nn/NNInterpolator.py:39-42, 86)"""
    return [indim] + [width] * (nlayers + 1) + [npc, npix]


def init_weights(dims, seed=SEED):
    """torch's default Linear initialisation in NNInterpolator's order of layers under
    torch.manual_seed(seed) (train_interpolator.py:171, 221); the global generator is
    left as it was"""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lins = [torch.nn.Linear(int(dims[i]), int(dims[i + 1]))
                for i in range(len(dims) - 1)]
    return ([l.weight.detach().clone() for l in lins],
            [l.bias.detach().clone() for l in lins])


def mapper(vec, log_ids):
    """getData's Mapper (train_interpolator.py:28-38): vec [T, ndim] physical units ->
    M, S (float64) and Mapper.forward of the vectors in float64, computed as
    nn_map_kernel computes it (float32 input, log10 on log_ids, (y - M) / S)"""
    vec = np.asarray(vec, dtype=np.float64)
    xv = vec.copy()
    for i in log_ids:
        xv[:, i] = np.log10(vec[:, i])
    M, S = xv.mean(axis=0), xv.std(axis=0)
    y = vec.astype(np.float32)
    for i in log_ids:
        y[:, i] = np.log10(y[:, i].astype(np.float64)).astype(np.float32)
    return M, S, (y.astype(np.float64) - M) / S


def _ptrs(ts):
    return ctypes.cast((ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts]),
                       ctypes.c_void_p)


class Trainer:
    """The device state of one training run and the four entry points around it.
    dats [T, npix], x [T, ndim] float32 device tensors; W, b lists of float32 tensors
    (copied to the device); Adam's moments start at zero."""

    def __init__(self, dats, x, W, b, D0, SD0, spread0, batch=100, device='cuda'):
        _lib.require_gpu()
        f32 = lambda t: torch.as_tensor(t).to(device=device,
                                               dtype=torch.float32).contiguous()
        self.device = device
        self.dats, self.x = f32(dats), f32(x)
        self.W, self.b = [f32(w).clone() for w in W], [f32(v).clone() for v in b]
        self.D0, self.SD0, self.spread0 = f32(D0), f32(SD0), float(spread0)
        self.T, self.npix = self.dats.shape
        self.nl = len(self.W)
        self.dims = np.array([self.W[0].shape[1]] + [w.shape[0] for w in self.W],
                             dtype=np.int32)
        if self.x.shape != (self.T, self.dims[0]) or self.dims[-1] != self.npix:
            raise ValueError('rows, parameters and layers do not fit together')
        self.batch = int(batch)
        self.mW = [torch.zeros_like(w) for w in self.W]
        self.vW = [torch.zeros_like(w) for w in self.W]
        self.mb = [torch.zeros_like(v) for v in self.b]
        self.vb = [torch.zeros_like(v) for v in self.b]
        self.steps = 0
        # (sized for the longest row list grad() takes, whatever the batch)
        nbytes = _lib.lib().rvs_nn_train_work_size(
            self.T, MAX_BATCH if self.batch <= MAX_BATCH else self.batch, self.nl,
            _lib.ptr(self.dims))
        if nbytes < 0:
            raise ValueError('network or batch beyond the limits of rvs_nn_train_*: '
                             'dims %s, batch %d' % (list(self.dims), self.batch))
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.loss_accum = torch.zeros(1, dtype=torch.float64, device=device)

    def _rows(self, rows):
        return torch.as_tensor(rows).to(device=self.device,
                                        dtype=torch.int32).contiguous()

    def grad(self, rows, backward=True, resid=False):
        """rvs_nn_train_grad of the rows: -> loss (device double [1]), dW, db (lists, or
        None without backward), the residual R - dat (or None)"""
        rows = self._rows(rows)
        n = len(rows)
        if not 1 <= n <= MAX_BATCH:
            raise ValueError('%d rows; rvs_nn_train_grad takes 1 to %d' % (n, MAX_BATCH))
        dW = [torch.empty_like(w) for w in self.W] if backward else None
        db = [torch.empty_like(v) for v in self.b] if backward else None
        res = torch.empty((n, self.npix), dtype=torch.float32,
                          device=self.device) if resid else None
        loss = torch.zeros(1, dtype=torch.float64, device=self.device)
        rc = _lib.lib().rvs_nn_train_grad(
            _lib.ptr(self.dats), _lib.ptr(self.x), self.T, _lib.ptr(rows), n, self.nl,
            _lib.ptr(self.dims), _ptrs(self.W), _ptrs(self.b), _lib.ptr(self.D0),
            _lib.ptr(self.SD0), self.spread0, _ptrs(dW) if backward else None,
            _ptrs(db) if backward else None, _lib.ptr(loss), _lib.ptr(res),
            _lib.ptr(self.work), _lib.stream())
        _lib.check(rc, 'rvs_nn_train_grad')
        return loss, dW, db, res

    def eval_rows(self, rows, pred=False):
        """mean|R - dat| / spread0 over the rows (any number of them) and, with pred,
        R [len(rows), npix] as residual + row (float32: within an ulp of the row's
        value of the R the loss was taken of)"""
        rows = self._rows(rows)
        total = torch.zeros(1, dtype=torch.float64, device=self.device)
        out = []
        for i in range(0, len(rows), MAX_BATCH):
            r = rows[i:i + MAX_BATCH]
            loss, _, _, res = self.grad(r, backward=False, resid=pred)
            total += loss * len(r)
            if pred:
                out.append(res + self.dats[r.long()])
        return float(total.item()) / len(rows), (torch.cat(out) if pred else None)

    def adam_step(self, dW, db, lr):
        """rvs_nn_adam_step from the given gradients"""
        self.steps += 1
        rc = _lib.lib().rvs_nn_adam_step(
            self.nl, _lib.ptr(self.dims), _ptrs(self.W), _ptrs(self.b), _ptrs(dW),
            _ptrs(db), _ptrs(self.mW), _ptrs(self.mb), _ptrs(self.vW), _ptrs(self.vb),
            float(lr), self.steps, _lib.stream())
        _lib.check(rc, 'rvs_nn_adam_step')

    def epoch(self, perm, lr, step_loss=False):
        """rvs_nn_train_epoch over the rows perm (queued, no synchronisation):
        self.loss_accum holds the epoch's lossAccum afterwards; -> the per-step losses
        (device) when asked for"""
        perm = self._rows(perm)
        nstep = (len(perm) + self.batch - 1) // self.batch
        sl = torch.zeros(nstep, dtype=torch.float64,
                         device=self.device) if step_loss else None
        self.loss_accum.zero_()
        rc = _lib.lib().rvs_nn_train_epoch(
            _lib.ptr(self.dats), _lib.ptr(self.x), self.T, _lib.ptr(perm), len(perm),
            self.batch, self.nl, _lib.ptr(self.dims), _ptrs(self.W), _ptrs(self.b),
            _ptrs(self.mW), _ptrs(self.mb), _ptrs(self.vW), _ptrs(self.vb),
            _lib.ptr(self.D0), _lib.ptr(self.SD0), self.spread0, float(lr), self.steps,
            _lib.ptr(self.loss_accum), _lib.ptr(sl), _lib.ptr(self.work), _lib.stream())
        _lib.check(rc, 'rvs_nn_train_epoch')
        self.steps += nstep
        return sl

    def state(self):
        """weights as numpy arrays (what a checkpoint holds)"""
        d = {}
        for i in range(self.nl):
            d['W%d' % i] = self.W[i].cpu().numpy()
            d['b%d' % i] = self.b[i].cpu().numpy()
        return d


def save_checkpoint(path, trainer):
    """weights only, as save_checkpoint (nn/NNInterpolator.py:134) -- an .npz"""
    tmp = path + '.tmp.npz'
    np.savez(tmp, dims=trainer.dims, **trainer.state())
    os.replace(tmp, path)


def load_checkpoint(path, dims):
    d = np.load(path, allow_pickle=False)
    if list(d['dims']) != list(dims):
        raise RuntimeError('checkpoint %s is of a network %s, not %s'
                           % (path, list(d['dims']), list(dims)))
    n = len(dims) - 1
    return ([torch.from_numpy(d['W%d' % i]) for i in range(n)],
            [torch.from_numpy(d['b%d' % i]) for i in range(n)])


def pca_components(rows, npc):
    """principal components of the rows (device tensor) by SVD of the centred rows:
    -> components [npc, npix] (orthonormal, float64), mean [npix]"""
    X = rows.to(torch.float64)
    mean = X.mean(dim=0)
    if npc > min(X.shape):
        raise ValueError('%d principal components of %d rows x %d pixels'
                         % (npc, X.shape[0], X.shape[1]))
    _, _, Vt = torch.linalg.svd(X - mean, full_matrices=False)
    return Vt[:npc], mean


def train(D, nlayers=2, width=256, npc=200, learning_rate0=1e-3, min_learning_rate=1e-8,
          log_ids=(0, ), mask_ids=None, batch=100, validation=False,
          validation_fraction=0.05, n_subset_data=None, patience=20,
          num_epochs=1_000_000, pca_init=False, random_pca=False, weights=None,
          checkpoint=None, resume=False, generator=None, perms=None, revision='',
          info=None, verbose=True, device='cuda'):
    """main's training (train_interpolator.py:170-363) of the dictionary
    make_interpol.build_specs or regularize_grid.regularize returns (specs may be the
    device tensor).  Returns the record of a library of kind 'nn': what
    TemplateLibrary(name, record) takes.
      weights = (W, b): initial weights instead of torch's default initialisation;
      generator: torch.Generator of the per-epoch torch.randperm (the order
      DataLoader(shuffle=True) draws); perms: an iterable of explicit permutations of
      range(number of training rows) instead;
      checkpoint: path of the weights-only .npz written every 32 epochs, read back
      with resume=True;
      info: a dict that receives losses, lrs, val_losses (per epoch), pred [T, npix]
      (numpy), final_loss, spread0, D0, SD0, x (the mapped vectors), train_set, loss0."""
    _lib.require_gpu()
    log_ids = [int(_) for _ in log_ids]
    dats = torch.as_tensor(D['specs']).to(device=device, dtype=torch.float32).contiguous()
    nspec, npix = dats.shape
    vecs = np.asarray(D['vec'], dtype=np.float64).T
    M, S, pts = mapper(vecs, log_ids)
    rstate = np.random.default_rng(44)
    d64 = dats.to(torch.float64)
    D0_64 = d64.mean(dim=0)
    D0 = D0_64.to(torch.float32)
    SD0 = d64.std(dim=0, unbiased=False).to(torch.float32)
    spread0 = float((d64 - D0_64).std(unbiased=False).item())
    del d64
    if validation:
        train_set = rstate.uniform(size=nspec) > validation_fraction
        validation_set = ~train_set
    else:
        train_set = np.ones(nspec, dtype=bool)
    if mask_ids is not None:
        mask = np.zeros(nspec, dtype=bool)
        mask[list(mask_ids)] = True
        train_set = train_set & (~mask)
    if n_subset_data is not None:
        train_ids = np.nonzero(train_set)[0]
        train_set[:] = False
        train_set[rstate.permutation(train_ids)[:n_subset_data]] = True
    train_ids = torch.as_tensor(np.nonzero(train_set)[0], dtype=torch.int64)
    ntrain = len(train_ids)
    dims = network_dims(vecs.shape[1], nlayers, width, npc, npix)
    restored = False
    if resume and checkpoint is not None and os.path.exists(checkpoint):
        W, b = load_checkpoint(checkpoint, dims)
        restored = True
    elif weights is not None:
        W, b = [torch.as_tensor(w) for w in weights[0]], [torch.as_tensor(v)
                                                          for v in weights[1]]
    else:
        W, b = init_weights(dims)
    loss0 = None
    if pca_init and not restored:
        rows = dats[train_ids.to(device)]
        comps, mean = pca_components(rows, npc)
        X = rows.to(torch.float64) - mean
        loss0 = float(((X - (X @ comps.T) @ comps).abs().mean()).item()) / spread0
        if random_pca:
            comps = torch.as_tensor(rstate.normal(size=(npc, npc)),
                                    device=device) @ comps
        comps = comps / torch.sqrt((comps**2).sum(dim=1))[:, None]
        W[-1] = (comps.T / SD0.to(torch.float64)[:, None]).to(torch.float32)
        b[-1] = torch.zeros(npix, dtype=torch.float32)
        if verbose:
            print('loss0', loss0)
    x = torch.as_tensor(pts.astype(np.float32))
    tr = Trainer(dats, x, W, b, D0, SD0, spread0, batch=batch, device=device)
    sched = PlateauScheduler(learning_rate0, patience=patience)
    losses, lrs, val_losses = [], [], []
    perms = iter(perms) if perms is not None else None
    counter = 0
    while True:
        counter += 1
        if perms is not None:
            perm = torch.as_tensor(next(perms), dtype=torch.int64)
        else:
            g = generator
            if g is None:   # RandomSampler.__iter__: a generator seeded from the global one
                g = torch.Generator()
                g.manual_seed(int(torch.empty((), dtype=torch.int64).random_().item()))
            perm = torch.randperm(ntrain, generator=g)
        lrs.append(sched.lr)
        tr.epoch(train_ids[perm], sched.lr)
        loss_accum = float(tr.loss_accum.item())   # the epoch's only synchronisation
        sched.step(loss_accum)
        val_loss = tr.eval_rows(np.nonzero(validation_set)[0])[0] if validation else 0
        loss_V = loss_accum / (nspec * npix)
        losses.append(loss_V)
        val_losses.append(val_loss)
        if verbose:
            print('it %d loss %.5f' % (counter, loss_V), 'val %.5f' % val_loss, 'lr',
                  sched.lr)
        if counter >= num_epochs or sched.lr < min_learning_rate:
            break
        if counter % CHECKPOINT_EVERY == 0 and checkpoint is not None:
            save_checkpoint(checkpoint, tr)
    final_loss, pred = tr.eval_rows(np.arange(nspec), pred=True)
    # train_interpolator.py:361-363: SD_0, D_0 folded into pc_layer
    tr.b[-1] = tr.D0 + tr.b[-1] * tr.SD0
    tr.W[-1] = tr.SD0[:, None] * tr.W[-1]
    rec = dict(nn_dims=np.array(dims, dtype=np.int32), nn_M=M, nn_S=S, nn_pts=pts,
               lam=np.asarray(D['lam'], dtype=np.float64),
               log_step=np.array(bool(D['log_step'])),
               log_spec=np.array(bool(D.get('log_spec', True))),
               parnames=np.array([str(_) for _ in D['parnames']]),
               log_ids=np.array(log_ids, dtype=np.int64), revision=np.array(str(revision)))
    for i in range(tr.nl):
        rec['nn_W%d' % i] = tr.W[i].cpu().numpy()
        rec['nn_b%d' % i] = tr.b[i].cpu().numpy()
    if checkpoint is not None and os.path.exists(checkpoint):
        os.unlink(checkpoint)
    if info is not None:
        info.update(losses=losses, lrs=lrs, val_losses=val_losses,
                    pred=pred.cpu().numpy(), final_loss=final_loss, spread0=spread0,
                    x=pts, train_set=train_set, loss0=loss0, vecs_orig=vecs,
                    D0=tr.D0.cpu().numpy(), SD0=tr.SD0.cpu().numpy())
    return rec


def make_parser():
    p = argparse.ArgumentParser(
        description='Train a neural network interpolator for stellar template spectra')
    flag = lambda name, help: p.add_argument(name, action='store_true', default=False,
                                             help=help)
    flag('--cpu', 'refused: there is no CPU path')
    flag('--batch_on_device', 'accepted and ignored: the data always lives on the device')
    flag('--validation', 'Enable validation during training')
    flag('--random_pca', 'Use random PCA initialization')
    flag('--pca_init', 'initialize with pca')
    flag('--resume', 'Resume training from checkpoint')
    p.add_argument('--dir', type=str, default='./',
                   help='Directory containing template data')
    p.add_argument('--nlayers', type=int, default=2, help='number of inner fc layers')
    p.add_argument('--revision', default='', help='Revision string')
    p.add_argument('--width', type=int, default=256, help='Network width')
    p.add_argument('--npc', type=int, default=200, help='Number of principal components')
    p.add_argument('--learning_rate0', type=float, default=1e-3,
                   help='Initial learning rate')
    p.add_argument('--min_learning_rate', type=float, default=1e-8,
                   help='Minimum learning rate')
    p.add_argument('--parnames', type=str, default='teff,logg,feh,alpha',
                   help='Comma-separated parameter names')
    p.add_argument('--log_ids', type=str, default='0',
                   help='Comma-separated indices of parameters to log-transform')
    p.add_argument('--mask_ids', type=str, default=None,
                   help='Comma-separated indices of parameters to mask')
    p.add_argument('--setup', type=str, required=True,
                   help='Name of the spectral configuration')
    p.add_argument('--batch', type=int, default=100, help='Training batch size')
    p.add_argument('--validation_fraction', type=float, default=0.05,
                   help='Validation fraction')
    p.add_argument('--n_subset_data', type=int, default=None,
                   help='Select a small subset of data (useful for testing)')
    p.add_argument('--patience', type=int, default=20)
    p.add_argument('--num_epochs', type=int, default=1_000_000)
    return p


def main(args=None):
    """reads <dir>/specs_<setup>.npz (python -m rvspecfit_amd.make_interpol --save_specs),
    writes <dir>/lib_<setup>.npz, which TemplateLibrary.from_npz reads, and
    <dir>/pred_<setup>.npz (train_interpolator.py:395-403)"""
    a = make_parser().parse_args(sys.argv[1:] if args is None else args)
    if a.cpu:
        raise _lib.RvsGpuError('rvspecfit_amd needs a ROCm GPU (MI355X); '
                               'there is no CPU path')
    D = dict(np.load(os.path.join(a.dir, 'specs_%s.npz' % a.setup), allow_pickle=False))
    D['parnames'] = a.parnames.split(',')
    info = {}
    rec = train(D, nlayers=a.nlayers, width=a.width, npc=a.npc,
                learning_rate0=a.learning_rate0, min_learning_rate=a.min_learning_rate,
                log_ids=[int(_) for _ in a.log_ids.split(',')],
                mask_ids=None if a.mask_ids is None else
                [int(_) for _ in a.mask_ids.split(',')],
                batch=a.batch, validation=a.validation,
                validation_fraction=a.validation_fraction,
                n_subset_data=a.n_subset_data, patience=a.patience,
                num_epochs=a.num_epochs, pca_init=a.pca_init, random_pca=a.random_pca,
                checkpoint=os.path.join(a.dir, 'tmp_state_%s.npz' % a.setup),
                resume=a.resume, revision=a.revision, info=info)
    fname = os.path.join(a.dir, 'lib_%s.npz' % a.setup)
    np.savez(fname, **rec)
    np.savez(os.path.join(a.dir, 'pred_%s.npz' % a.setup), pred=info['pred'],
             vecs=info['x'], dats=np.asarray(torch.as_tensor(D['specs']).cpu()),
             vecs_orig=info['vecs_orig'])
    return fname


if __name__ == '__main__':
    main()
