#!/usr/bin/env python3
"""Epoch time of the MLP trainer (rvs_nn_train_epoch) against the same loop in eager
torch on the same device (tests/refmachines/nn_train_torch.py: whole data on the device,
same batch order).

    python tools/perf/nn_train_timing.py --size desi --out profiles/nn_train_timing_desi.json
    python tools/perf/nn_train_timing.py --size fixture --variant hip --epochs 3   # under rocprofv3 --kernel-trace --stats

Each variant runs in a fresh child process, the two alternating --rounds times; an
epoch is bracketed by device events after --warmup epochs; the medians over all timed
epochs of a variant are reported with the ratio torch / hip.  Rows are generated on the
device from a seed (sizes: desi = 10 000 x 6215, width 256, npc 200, batch 100;
fixture = 254 x 977, width 64, npc 40)."""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
SIZES = dict(desi=(10000, 6215, 256, 200), fixture=(254, 977, 64, 40))


def child(a):
    import torch
    from refmachines import nn_train_torch as rm
    from rvspecfit_amd.nn import train_interpolator as ti
    T, npix, width, npc = SIZES[a.size]
    g = torch.Generator(device='cuda').manual_seed(1)
    x = torch.randn(T, 4, generator=g, device='cuda')
    dats = 0.1 * torch.randn(T, npix, generator=g, device='cuda') + \
        0.3 * torch.sin(x[:, :1] + torch.linspace(0, 20, npix, device='cuda'))
    D0, SD0 = dats.mean(0), dats.std(0)
    spread0 = float((dats - D0).std())
    dims = ti.network_dims(4, 2, width, npc, npix)
    W, b = ti.init_weights(dims)
    pg = torch.Generator().manual_seed(2)
    perms = [torch.randperm(T, generator=pg) for _ in range(a.warmup + a.epochs)]
    if a.variant == 'hip':
        tr = ti.Trainer(dats, x, W, b, D0, SD0, spread0, batch=100)
        run = lambda p: tr.epoch(p, 1e-3)  # noqa: E731
    else:
        W, b = [w.cuda() for w in W], [v.cuda() for v in b]
        opt = rm.Adam(W + b)
        run = lambda p: rm.train_epoch(W, b, opt, dats, x, p.cuda(), 100, 1e-3, D0, SD0,  # noqa: E731
                                       spread0)
    times = []
    for i, p in enumerate(perms):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run(p)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            times.append(e0.elapsed_time(e1))
    print(json.dumps(dict(variant=a.variant, size=a.size, epoch_ms=times,
                          steps=(T + 99) // 100)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--size', choices=list(SIZES), default='desi')
    p.add_argument('--variant', choices=['hip', 'torch'], default=None)
    p.add_argument('--epochs', type=int, default=5)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--rounds', type=int, default=2)
    p.add_argument('--out', default=None)
    a = p.parse_args()
    if a.variant:
        return child(a)
    import numpy as np
    ms = dict(hip=[], torch=[])
    steps = 0
    for _ in range(a.rounds):
        for v in ('hip', 'torch'):
            out = subprocess.check_output(
                [sys.executable, os.path.abspath(__file__), '--size', a.size, '--variant', v,
                 '--epochs', str(a.epochs), '--warmup', str(a.warmup)], timeout=900)
            r = json.loads(out.decode().strip().splitlines()[-1])
            ms[v] += r['epoch_ms']
            steps = r['steps']
    res = dict(size=a.size, rows_pixels_width_npc=SIZES[a.size], steps_per_epoch=steps,
               epochs_timed=len(ms['hip']))
    for v in ms:
        res[v + '_epoch_ms'] = float(np.median(ms[v]))
        res[v + '_step_us'] = 1e3 * res[v + '_epoch_ms'] / steps
        res[v + '_epoch_ms_all'] = ms[v]
    res['torch_over_hip'] = res['torch_epoch_ms'] / res['hip_epoch_ms']
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
