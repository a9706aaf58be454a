"""Time the kernels behind regularize_grid.regularize on one window of PHOENIX-like size:
N nodes of a holey 4-D rank grid (13 teff values x logg x feh x alpha), S pixels of a
DESI arm, M points to predict.

    python tools/perf/regularize_timing.py [--nodes 3000] [--pixels 6215] [--points 4000]
                                           [--reps 3] [--scipy 1]

Prints one JSON line: HIP-event times (ms, median of --reps after a warm-up) of
rvs_rbf_factor (assembly + blocked Cholesky; the split between the two is in the kernel
trace), rvs_rbf_solve and rvs_rbf_eval, the float64 operations of each (N^3 / 3,
2 N^2 (S + 1), 2 M N S: the products alone, not the square roots) and their rate against
the 78.6 TF float64 peak, the largest difference from scipy, and -- with --scipy -- the
time scipy's RBFInterpolator takes for the same window in a CPU process of its own."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))))
from rvspecfit_amd import _lib   # noqa: E402

PEAK_TF = 78.6

SCIPY = r'''
import json, sys, time
import numpy as np
import scipy.interpolate
z = np.load(sys.argv[1])
t0 = time.time()
rr = scipy.interpolate.RBFInterpolator(z['y'], z['d'], kernel='multiquadric', epsilon=1)
t1 = time.time()
out = rr(z['x'])
t2 = time.time()
np.save(sys.argv[2], out[:, :8])
print(json.dumps(dict(fit=t1 - t0, call=t2 - t1)))
'''


def window(N, S, M, seed=1):
    rng = np.random.default_rng(seed)
    G = np.array(np.meshgrid(np.arange(13.), np.arange(8.), np.arange(10.), np.arange(6.),
                             indexing='ij')).reshape(4, -1).T
    if N > len(G):
        raise SystemExit('--nodes: at most %d' % len(G))
    y = G[rng.permutation(len(G))[:N]] + 0.05 * rng.standard_normal((N, 4))
    ph = rng.random((4, S)) * 6
    d = sum(np.sin(0.4 * y[:, k][:, None] + ph[k][None, :]) for k in range(4))
    x = rng.random((M, 4)) * G.max(axis=0)
    return y, d.astype(np.float32), x


def ev():
    return torch.cuda.Event(enable_timing=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--nodes', type=int, default=3000)
    ap.add_argument('--pixels', type=int, default=6215)
    ap.add_argument('--points', type=int, default=4000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--scipy', type=int, default=1)
    a = ap.parse_args()
    _lib.require_gpu()
    N, S, M = a.nodes, a.pixels, a.points
    y, d, x = window(N, S, M)
    L = _lib.lib()
    dy, dd, dx = (torch.as_tensor(v).to('cuda') for v in (y, d, x))
    work = torch.empty(L.rvs_rbf_work_size(N, S), dtype=torch.float64, device='cuda')
    status = torch.zeros(1, dtype=torch.int32, device='cuda')
    out = torch.empty((M, S), dtype=torch.float32, device='cuda')
    t = dict(factor=[], solve=[], eval=[])
    for rep in range(a.reps + 1):
        e = [ev() for _ in range(4)]
        e[0].record()
        _lib.check(L.rvs_rbf_factor(_lib.ptr(dy), N, 4, 1.0, None, _lib.ptr(work),
                                    _lib.ptr(status), _lib.stream()), 'rvs_rbf_factor')
        e[1].record()
        _lib.check(L.rvs_rbf_solve(_lib.ptr(dd), 1, S, N, S, _lib.ptr(work),
                                   _lib.ptr(status), _lib.stream()), 'rvs_rbf_solve')
        e[2].record()
        _lib.check(L.rvs_rbf_eval(_lib.ptr(dx), M, _lib.ptr(dy), N, 4, 1.0, _lib.ptr(work),
                                  S, 32, _lib.ptr(out), S, _lib.stream()), 'rvs_rbf_eval')
        e[3].record()
        torch.cuda.synchronize()
        if rep:
            for k, name in enumerate(('factor', 'solve', 'eval')):
                t[name].append(e[k].elapsed_time(e[k + 1]))
    if int(status.item()):
        raise SystemExit('status 0x%x' % int(status.item()))
    ops = dict(factor=N**3 / 3., solve=2. * N * N * (S + 1), eval=2. * M * N * S)
    res = dict(N=N, S=S, M=M, ndim=4, reps=a.reps)
    for k in ('factor', 'solve', 'eval'):
        ms = float(np.median(t[k]))
        res[k + '_ms'] = round(ms, 3)
        res[k + '_gflop'] = round(ops[k] / 1e9, 1)
        res[k + '_tflops'] = round(ops[k] / (ms * 1e-3) / 1e12, 2)
        res[k + '_of_peak'] = round(ops[k] / (ms * 1e-3) / 1e12 / PEAK_TF, 3)
    res['total_ms'] = round(sum(res[k + '_ms'] for k in ('factor', 'solve', 'eval')), 3)
    if a.scipy:
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            np.savez(tmp + '/in.npz', y=y, d=d.astype(np.float64), x=x)
            env = dict(os.environ, HIP_VISIBLE_DEVICES='')
            got = subprocess.check_output([sys.executable, '-c', SCIPY, tmp + '/in.npz',
                                           tmp + '/out.npy'], env=env)
            sc = json.loads(got.decode().strip().splitlines()[-1])
            ref = np.load(tmp + '/out.npy')
        res.update(scipy_fit_s=round(sc['fit'], 2), scipy_call_s=round(sc['call'], 2),
                   scipy_threads=int(os.environ.get('OMP_NUM_THREADS', 0)),
                   max_diff_scipy_f32=float(np.abs(out[:, :8].cpu().numpy() - ref).max()))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
