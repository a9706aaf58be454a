#!/usr/bin/env python3
"""Template rows with their tangents on an MLP library: ONE rvs_template_nn_grad call
(TemplateLibrary.eval_batch_grad) against the 1 + ndim rvs_template_nn calls
(eval_batch) a forward difference of the template needs -- the same matrix products
and the same B (1 + ndim) ntp doubles written on either side.
usage: nn_grad_ab.py [--jobs J [J ...]] [--ntp N] [--rounds R]
       nn_grad_ab.py --chain [--jobs J] [--spectra S] [--npoly P] [--rounds R]
The network is bench.py's seeded DESI-shape MLP (4 -> 256 -> 256 -> 256 -> 200 -> ntp,
ntp = 6215: the b arm).  Both sides run alternately in one process, R rounds after a
warm-up; one JSON line: per job count the median and minimum seconds of each side,
their ratio, and the largest difference between the tangent rows and the forward
difference relative to the row's largest entry (a sanity figure: the difference is
the forward difference's error in float32 templates).
--chain: one line for spec_fit.chisq_grad_jobs with config['nn_gradient'] on bench.py's
three-arm MLP libraries (the workload of grad_ab.py, whose regular-grid line it stands
beside): median and minimum seconds of the call."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, nargs='+', default=None)
    ap.add_argument('--ntp', type=int, default=6215)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--chain', action='store_true')
    ap.add_argument('--spectra', type=int, default=512)
    ap.add_argument('--npoly', type=int, default=10)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import bench
    from rvspecfit_amd import _lib, engine, spec_fit, spec_inter
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    dev = torch.device('cuda', 0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    if args.chain:
        S, J = args.spectra, (args.jobs or [8192])[0]
        bench.EVALUATOR = 'nn'

        def gpu_convolve(lam, templ, vsini):
            t = torch.as_tensor(np.ascontiguousarray(templ)).to(dev)
            v = torch.as_tensor(np.ascontiguousarray(vsini)).to(dev)
            return engine.convolve_vsini(lam, t, v).cpu().numpy()
        for name, d in bench.build_library_dicts(64, gpu_convolve).items():
            spec_inter.register_library(TemplateLibrary(name, d, device=dev),
                                        bench.CONFIG['template_lib'])
        tp = bench.truth_params(S, seed=3)
        cfg = dict(bench.CONFIG, nn_gradient=True)
        batch = engine.SpecBatch([engine.ArmData(n, lam, sp, es, bad, device=dev)
                                  for n, lam, sp, es, bad in
                                  bench.make_spectra_from_library(tp, dev, bench.CONFIG)])
        opt = dict(bench.OPTIONS, npoly=args.npoly)
        g = torch.Generator(device=dev)
        g.manual_seed(17)
        idx = torch.arange(J, device=dev) % S
        par = torch.stack([torch.as_tensor(np.asarray(tp[k], dtype=np.float64)).to(dev)[idx]
                           for k in ('teff', 'logg', 'feh', 'alpha')], dim=1)
        par = par * (1 + 1e-3 * (torch.rand(par.shape, device=dev, generator=g,
                                            dtype=torch.float64) - 0.5))
        vel = torch.as_tensor(np.asarray(tp['vel'], dtype=np.float64)).to(dev)[idx] + \
            torch.rand(J, device=dev, generator=g, dtype=torch.float64)
        call = lambda: spec_fit.chisq_grad_jobs(batch, idx, vel, par, None, opt, cfg)  # noqa
        timed(call)
        ts = []
        for _ in range(args.rounds):
            t, (chi, grad, st) = timed(call)
            ts.append(t)
        print(json.dumps(dict(
            what='chisq_grad_jobs', evaluator='nn', jobs=J, spectra=S, npoly=args.npoly,
            arms=len(batch.arms), rounds=args.rounds,
            s_median=round(float(np.median(ts)), 6), s_min=round(min(ts), 6),
            jobs_ok=int(((st == 0) & torch.isfinite(grad).all(dim=1)).sum()))),
            flush=True)
        return

    lam = np.exp(np.linspace(np.log(3600.), np.log(5800.), args.ntp))
    w = bench.nn_weights(args.ntp, 11)
    lib = TemplateLibrary('desi_b', dict(
        w, lam=lam, log_step=np.array(True), log_ids=np.array([0]),
        parnames=np.array(['teff', 'logg', 'feh', 'alpha'])), device=dev)
    nd = lib.ndim
    out = []
    for J in (args.jobs or [2000, 8192]):
        g = torch.Generator(device=dev)
        g.manual_seed(J)
        u = torch.rand((J, nd), device=dev, generator=g, dtype=torch.float64)
        lo = torch.tensor([4000., 1., -2., 0.], dtype=torch.float64, device=dev)
        hi = torch.tensor([7000., 4.5, 0., 0.6], dtype=torch.float64, device=dev)
        par = lo + u * (hi - lo)
        # (float32 templates: a step of 1e-3 of the parameter's scale, not sqrt(eps64))
        h = 1e-3 * torch.tensor([100., 1., 1., 1.], dtype=torch.float64, device=dev)

        def analytic():
            return lib.eval_batch_grad(par)[0]

        pts = [par]
        for k in range(nd):
            y = par.clone()
            y[:, k] += h[k]
            pts.append(y)

        def differenced():   # (the calls alone: the subtraction is not timed)
            return [lib.eval_batch(y)[0] for y in pts]
        timed(analytic), timed(differenced)
        ta, td = [], []
        for _ in range(args.rounds):
            t, ga = timed(analytic)
            ta.append(t)
            t, gd = timed(differenced)
            td.append(t)
        rel = max((((gd[1 + k] - gd[0]) / h[k] - ga[:, 1 + k]).abs().amax(dim=1) /
                   ga[:, 1 + k].abs().amax(dim=1)).max().item() for k in range(nd))
        same = bool(torch.equal(ga[:, 0], gd[0]))
        del ga, gd
        out.append(dict(jobs=J, grad_s_median=round(float(np.median(ta)), 6),
                        grad_s_min=round(min(ta), 6),
                        value_calls_s_median=round(float(np.median(td)), 6),
                        value_calls_s_min=round(min(td), 6),
                        ratio_median=round(float(np.median(td) / np.median(ta)), 3),
                        row0_is_the_value_call=same,
                        tangent_vs_forward_difference_max_rel=rel))
    print(json.dumps(dict(what='rvs_template_nn_grad', dims=[int(_) for _ in lib.nn_dims],
                          value_calls=1 + nd, rounds=args.rounds, cases=out)),
          flush=True)


if __name__ == '__main__':
    main()
