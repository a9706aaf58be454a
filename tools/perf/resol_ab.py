#!/usr/bin/env python3
"""The optimiser with resolution matrices: the band inside the objective kernel
against the chain of stand-alone kernels (engine.FUSED_OBJECTIVE_RESOL = False),
alternating, every run a fresh process.
usage: resol_ab.py [--reps N] [--spectra S] [--evaluator polylinear|nn] [--npoly P]
                   [--no-bfgs]
The workload is bench.py's (its synthetic DESI-shape libraries and spectra, its CCF +
velocity-grid step for the starting parameters) with per-spectrum resolution matrices
of 11 diagonals on every arm -- Gaussian rows of sigma 0.45-0.65 A on 0.8-A pixels,
normalised: what `bench.py --resolution-matrix` puts on its batch -- and
vel_fit.process on ALL S spectra WITH their matrices (the `--process` add-on of
bench.py builds its sub-batch from spectra and errors alone; this tool is where the
optimiser with matrices is timed).  One JSON line per run: which objective ran, the
rate, the stage times of a second single-stream run, the optimiser's counts."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(args):
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import bench
    from rvspecfit_amd import _lib, engine, pipeline, spec_inter, vel_fit
    from rvspecfit_amd.library import TemplateLibrary
    engine.FUSED_OBJECTIVE_RESOL = (args.child == 'kernel')
    bench.EVALUATOR = args.evaluator
    bench.OPTIONS['npoly'] = args.npoly
    _lib.require_gpu()
    dev = torch.device('cuda', 0)
    S = args.spectra

    def gpu_convolve(lam, templ, vsini):
        t = torch.as_tensor(np.ascontiguousarray(templ)).to(dev)
        v = torch.as_tensor(np.ascontiguousarray(vsini)).to(dev)
        return engine.convolve_vsini(lam, t, v).cpu().numpy()

    for name, d in bench.build_library_dicts(64, gpu_convolve).items():
        spec_inter.register_library(TemplateLibrary(name, d, device=dev),
                                    bench.CONFIG['template_lib'])
    tp = bench.truth_params(S, seed=3)
    arms = bench.make_spectra_device(tp, dev) if args.evaluator != 'nn' else \
        bench.make_spectra_from_library(tp, dev, bench.CONFIG)
    batch = engine.SpecBatch([engine.ArmData(n, lam, sp, es, bad, device=dev)
                              for n, lam, sp, es, bad in arms])
    g = torch.Generator(device=dev)
    g.manual_seed(991)
    for a in batch.arms:
        sig = 0.45 + 0.2 * torch.rand((S, 1, 1), device=dev, generator=g,
                                      dtype=torch.float64)
        d = torch.arange(-5, 6, device=dev, dtype=torch.float64)[None, None]
        k = torch.arange(a.npix, device=dev)[None, :, None]
        t = torch.exp(-0.5 * (d / (sig / 0.8))**2).expand(S, a.npix, 11).clone()
        q = k + d.long()
        t = torch.where((q >= 0) & (q < a.npix), t, torch.zeros_like(t))
        t = t / t.sum(dim=2, keepdim=True)
        a.resol = dict(taps=t.contiguous(), nd=11, stride=a.npix * 11,
                       unit=t.sum(dim=2).contiguous())
    rec = pipeline.fit_batch(batch, bench.CONFIG, options=bench.OPTIONS)
    F = pipeline.RECORD_FIELDS
    names = ['teff', 'logg', 'feh', 'alpha']
    pd0 = {k: rec[:, F.index('p%d' % i)].contiguous() for i, k in enumerate(names)}
    vs = rec[:, F.index('vsini')]
    pd0['vsini'] = torch.where(torch.isfinite(vs), vs, torch.zeros_like(vs)).contiguous()
    cfg = dict(bench.CONFIG)
    cfg.setdefault('max_vsini', 500)
    cfg['second_minimizer'] = not args.no_bfgs
    opt = bench.OPTIONS
    libs = spec_inter.get_libs(batch.names, cfg)
    form = engine.objective_form(batch, libs, None, opt['npoly'])
    vel_fit.process(batch, pd0, options=opt, config=cfg)   # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = vel_fit.process(batch, pd0, options=opt, config=cfg)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tm = {}
    t1 = time.perf_counter()
    vel_fit.process(batch, pd0, options=opt, config=cfg, timers=tm)
    torch.cuda.synchronize()
    dt1 = time.perf_counter() - t1
    fin = torch.isfinite(r['chisq'])
    print(json.dumps(dict(
        which=args.child, objective=form,
        rounds_in_library=bool(engine.rounds_in_library(batch, libs, form)),
        spectra=S, evaluator=args.evaluator, npoly=opt['npoly'],
        second_minimizer=not args.no_bfgs, diagonals=11,
        spectra_per_s=round(S / dt, 1), seconds=round(dt, 3),
        single_stream_seconds=round(dt1, 3),
        stage_s={k: round(v, 3) for k, v in tm.items()},
        nm_rounds=int(r['nm_rounds']), objective_evals=int(r['objective_evals']),
        nm_iterations_mean=round(float(r['nm_nit'].float().mean()), 1),
        minimize_success=round(float(r['minimize_success'].float().mean()), 4),
        chisq_sum=float(r['chisq'][fin].sum()), finite=int(fin.sum()),
        vel_rms_vs_truth=round(float((
            r['vel'].cpu().double() - torch.as_tensor(tp['vel'])).pow(2).mean().sqrt()), 3))),
        flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--spectra', type=int, default=2000)
    ap.add_argument('--evaluator', choices=['polylinear', 'nn'], default='polylinear')
    ap.add_argument('--npoly', type=int, default=10)
    ap.add_argument('--no-bfgs', action='store_true')
    ap.add_argument('--child', choices=['chain', 'kernel'], default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    pas = [a for a in sys.argv[1:]]
    for rep in range(args.reps):
        for which in ('chain', 'kernel'):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', which]
                               + pas, cwd=REPO, capture_output=True, text=True)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
            if p.returncode != 0 or not lines:
                print(json.dumps(dict(which=which, rep=rep, failed=p.returncode,
                                      stderr=p.stderr[-600:])), flush=True)
                continue
            d = json.loads(lines[-1])
            d['rep'] = rep
            print(json.dumps(d), flush=True)


if __name__ == '__main__':
    main()
