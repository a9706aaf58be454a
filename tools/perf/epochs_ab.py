#!/usr/bin/env python3
"""The joint fit of a star's epochs (vel_fit.process_epochs) against the independent
Levenberg-Marquardt polish of the same spectra (lm.minimize_lockstep_device, rvs_lm_run),
alternating, in one process.
usage: epochs_ab.py [--stars N] [--epochs E] [--npoly P] [--rounds R]
The workload is bench.py's (its synthetic DESI-shape 3-arm libraries and seeded spectra):
N stars with bench.truth_params' parameters, E epochs each at the star's velocity plus
N(0, 30 km/s), noise of their own.  vel_fit.process runs once on the N E spectra without
the second minimiser; its simplex optimum is the common start:
  (a) process_epochs from the per-star plain mean of that optimum's parameters and its
      velocities (rvs_alm_run: the rounds inside the library);
  (b) the existing polish, lm.minimize_lockstep_device, on the same N E spectra fitted
      independently from that optimum.
R rounds after a warm-up, the legs taking turns inside every round; one JSON line:
seconds per leg (median, minimum, the spread max - min), rows, rows per spectrum and
template-stage rows per spectrum, statuses, and at E = 1 whether leg (a) is slower
than leg (b) by more than the spread between rounds (`e1_criterion_met`).  Leg (a)'s seconds are all of process_epochs
(sorting the batch, building the chain, the closing evaluation and the uncertainties on
the host); `a.minimise_s` is its minimiser alone.  Times are to be held against leg (b)
of the SAME line.  (Profiles kept: profiles/epochs_ab_250x8.json, epochs_ab_2000x1.json.)"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stars', type=int, default=250)
    ap.add_argument('--epochs', type=int, default=8)
    ap.add_argument('--npoly', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import bench
    from rvspecfit_amd import _lib, engine, lm, optimizer, pipeline, spec_inter
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    dev = torch.device('cuda', 0)
    N, E = args.stars, args.epochs
    S = N * E

    def gpu_convolve(lam, templ, vsini):
        t = torch.as_tensor(np.ascontiguousarray(templ)).to(dev)
        v = torch.as_tensor(np.ascontiguousarray(vsini)).to(dev)
        return engine.convolve_vsini(lam, t, v).cpu().numpy()

    bench.EVALUATOR = 'polylinear'
    for name, d in bench.build_library_dicts(64, gpu_convolve).items():
        spec_inter.register_library(TemplateLibrary(name, d, device=dev),
                                    bench.CONFIG['template_lib'])
    tp = bench.truth_params(N, seed=3)
    star = np.repeat(np.arange(N), E)
    rng = np.random.RandomState(5)
    tpe = {k: (np.asarray(v)[star] if k != 'seed' else v) for k, v in tp.items()}
    tpe['vel'] = tpe['vel'] + rng.normal(0, 30.0, S)
    batch = engine.SpecBatch([engine.ArmData(n, lam, sp, es, bad, device=dev)
                              for n, lam, sp, es, bad in
                              bench.make_spectra_device(tpe, dev)])
    cfg, opt = dict(bench.CONFIG), dict(bench.OPTIONS, npoly=args.npoly)
    rec = pipeline.fit_batch(batch, cfg, options=opt)
    F = pipeline.RECORD_FIELDS
    names = ['teff', 'logg', 'feh', 'alpha']
    pd0 = {k: rec[:, F.index('p%d' % i)].contiguous() for i, k in enumerate(names)}
    vs = rec[:, F.index('vsini')]
    pd0['vsini'] = torch.where(torch.isfinite(vs), vs, torch.zeros_like(vs)).contiguous()
    r = vel_fit.process(batch, dict(pd0), options=opt,
                        config=dict(cfg, second_minimizer=False))
    cols = ['vel', 'vsini'] + names
    v = dict(vel=r['nm_vel'], vsini=r['vsini'])
    v.update(r['param'])
    x0 = torch.stack([v[c].double() for c in cols], dim=1).contiguous()
    libs = spec_inter.get_libs(batch.names, cfg)
    pdt = {k: t.double().contiguous() for k, t in pd0.items()}
    safe = torch.stack([pdt[k] for k in names], dim=1).contiguous()
    pobj = optimizer.ProcessObjective(batch, libs, names, pdt, [], True, cfg, opt, None,
                                      safe)
    fchain = optimizer.GradChain(pobj, fisher=True)
    x0h = x0.cpu().numpy()
    pds = {c: x0h[:, i].reshape(N, E).mean(axis=1) for i, c in enumerate(cols)
           if c != 'vel'}
    vel0 = x0h[:, 0].copy()

    def leg_a():
        return vel_fit.process_epochs(batch, star, dict(pds), vel0, options=opt,
                                      config=cfg)

    def leg_b():
        return lm.minimize_lockstep_device(pobj, x0, chain=fchain)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    timed(leg_a), timed(leg_b)                 # warm-up
    ta, tb = [], []
    for _ in range(args.rounds):
        t, a = timed(leg_a)
        ta.append(t)
        t, b = timed(leg_b)
        tb.append(t)

    def secs(ts):
        return dict(median=round(float(np.median(ts)), 4), min=round(min(ts), 4),
                    spread=round(max(ts) - min(ts), 4))

    verr = np.abs(a['vel'] - tpe['vel'])
    bvel = b['x'][:, 0].cpu().numpy()
    print(json.dumps(dict(
        stars=N, epochs=E, spectra=S, npoly=args.npoly, rounds=args.rounds, m=5,
        a=dict(seconds=secs(ta), minimise_s=round(a['seconds']['minimise'], 4),
               setup_s=round(a['seconds']['setup'], 4),
               closing_s=round(a['seconds']['closing'], 4),
               lockstep_rounds=a['rounds'], star_rows=int(a['nfev'].sum()),
               rows_per_spectrum=round(float((a['nfev'] * E).sum()) / S, 2),
               template_rows_per_spectrum=round(float(a['nfev'].sum()) / S, 2),
               nit_mean=round(float(a['nit'].mean()), 2),
               status_counts=np.bincount(a['status'], minlength=4).tolist(),
               median_abs_vel_error=float(np.median(verr))),
        b=dict(seconds=secs(tb), lockstep_rounds=b['rounds'],
               rows_launched=b['rows_launched'],
               rows_per_spectrum=round(b['rows_launched'] / S, 2),
               template_rows_per_spectrum=round(b['rows_launched'] / S, 2),
               nit_mean=round(float(b['nit'].double().mean()), 2),
               status_counts=np.bincount(b['status'].cpu().numpy(),
                                         minlength=4).tolist(),
               median_abs_vel_error=float(np.median(np.abs(bvel - tpe['vel'])))),
        a_over_b_time=round(float(np.median(ta) / np.median(tb)), 3),
        # the criterion at E = 1: leg (a) no slower than leg (b) by more than the spread
        # between rounds this line reports (null for E > 1, where the figure is the finding)
        e1_slower_by_s=round(float(np.median(ta) - np.median(tb)), 4),
        e1_criterion_met=(bool(np.median(ta) - np.median(tb) <=
                               max(max(ta) - min(ta), max(tb) - min(tb)))
                          if E == 1 else None))), flush=True)


if __name__ == '__main__':
    main()
