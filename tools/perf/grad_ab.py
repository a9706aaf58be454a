#!/usr/bin/env python3
"""Value + gradient of the objective for J jobs: ONE spec_fit.chisq_grad_jobs call
against the (2 + ndim) spec_fit.chisq_jobs calls of a forward difference (the point
itself, then one call per displaced coordinate: velocity and the ndim parameters --
what a caller without the gradient has to do, and what BFGS does per gradient).
usage: grad_ab.py [--jobs J] [--spectra S] [--npoly P] [--rounds R] [--vsini]
                  [--vsini-grad] [--evaluator polylinear|tri] [--resolution-matrix]
                  [--fused]
--fused: a third leg, the same chisq_grad_jobs call with config['fused_gradient']
(rvs_objective_grad: value and gradient in one kernel per (job, arm)), alternating
with the two (fused_s_*, chain_over_fused_median, differenced_over_fused_median, and
the largest difference of the fused gradient from the chain's).
--evaluator tri: bench.py's Delaunay library (the same grid nodes triangulated, its
`--evaluator tri`): rvs_template_tri_buckets_grad in front of the same chain.
--vsini-grad (implies --vsini): the analytic call carries the vsini tangent row
(vsini_grad=True) and the forward difference displaces vsini too: 3 + ndim calls.
--resolution-matrix: every spectrum carries resolution matrices of 11 diagonals
(tools/perf/_resol.py, as resol_ab.py builds them); the analytic call runs with
config['resol_gradient'] (rvs_chisq_point_grad_resol), the forward difference under the
same matrices, and a third arm is the same analytic call on the same spectra WITHOUT
matrices, alternating with the two (no_matrix_s_*, resol_over_no_matrix_median).
With --fused beside it the fused leg runs under the same matrices with both keys
(rvs_objective_grad_resol: the band and its transpose inside the kernel),
and one more leg is the fused call on the same spectra WITHOUT matrices
(fused_no_matrix_s_*, fused_resol_over_fused_no_matrix_median: what the band costs there).
The workload is bench.py's (its synthetic DESI-shape libraries and
spectra); the jobs are its truth parameters, jittered inside the grid, spread over the
S spectra.  Both arms run alternately in one process, R rounds after a warm-up; one
JSON line: median and minimum seconds of each arm, their ratio, and the largest
difference between the analytic and the differenced gradient relative to
max(|g_k|, 1e-6 |g|_inf) (a sanity figure: the difference is the forward
difference's error)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--jobs', type=int, default=8192)
    ap.add_argument('--spectra', type=int, default=512)
    ap.add_argument('--npoly', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--vsini', action='store_true')
    ap.add_argument('--vsini-grad', action='store_true')
    ap.add_argument('--evaluator', choices=['polylinear', 'tri'], default='polylinear')
    ap.add_argument('--resolution-matrix', action='store_true')
    ap.add_argument('--fused', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import bench
    from rvspecfit_amd import _lib, engine, spec_fit, spec_inter
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    dev = torch.device('cuda', 0)
    S, J = args.spectra, args.jobs

    def gpu_convolve(lam, templ, vsini):
        t = torch.as_tensor(np.ascontiguousarray(templ)).to(dev)
        v = torch.as_tensor(np.ascontiguousarray(vsini)).to(dev)
        return engine.convolve_vsini(lam, t, v).cpu().numpy()

    bench.EVALUATOR = args.evaluator
    for name, d in bench.build_library_dicts(64, gpu_convolve).items():
        spec_inter.register_library(TemplateLibrary(name, d, device=dev),
                                    bench.CONFIG['template_lib'])
    tp = bench.truth_params(S, seed=3)
    batch = engine.SpecBatch([engine.ArmData(n, lam, sp, es, bad, device=dev)
                              for n, lam, sp, es, bad in
                              bench.make_spectra_device(tp, dev)])
    cfg, opt = dict(bench.CONFIG), dict(bench.OPTIONS, npoly=args.npoly)
    plain = None
    if args.resolution_matrix:
        import _resol
        plain = engine.SpecBatch([engine.ArmData(n, lam, sp, es, bad, device=dev)
                                  for n, lam, sp, es, bad in
                                  bench.make_spectra_device(tp, dev)])
        _resol.attach(batch, S, dev)
        cfg['resol_gradient'] = True
    libs = spec_inter.get_libs(batch.names, cfg)
    ndim = libs[batch.names[0]].ndim
    g = torch.Generator(device=dev)
    g.manual_seed(17)
    idx = torch.arange(J, device=dev) % S
    names = ['teff', 'logg', 'feh', 'alpha'][:ndim]
    par = torch.stack([torch.as_tensor(np.asarray(tp[k], dtype=np.float64)).to(dev)[idx]
                       for k in names], dim=1)
    par = par * (1 + 1e-3 * (torch.rand(par.shape, device=dev, generator=g,
                                        dtype=torch.float64) - 0.5))
    vel = torch.as_tensor(np.asarray(tp['vel'], dtype=np.float64)).to(dev)[idx] + \
        torch.rand(J, device=dev, generator=g, dtype=torch.float64)
    vg = args.vsini_grad
    vs = torch.full((J, ), 20.0, dtype=torch.float64, device=dev) \
        if args.vsini or vg else None
    x = torch.cat([vel[:, None], par] + ([vs[:, None]] if vg else []), dim=1)
    h = 1.4901161193847656e-08 * torch.clamp(x.abs(), min=1.0)

    def analytic():
        return spec_fit.chisq_grad_jobs(batch, idx, vel, par, vs, opt, cfg,
                                        vsini_grad=vg)

    def no_matrix():
        return spec_fit.chisq_grad_jobs(plain, idx, vel, par, vs, opt, cfg,
                                        vsini_grad=vg)

    fcfg = dict(cfg, fused_gradient=True)

    def fused():
        return spec_fit.chisq_grad_jobs(batch, idx, vel, par, vs, opt, fcfg,
                                        vsini_grad=vg)

    def fused_no_matrix():
        return spec_fit.chisq_grad_jobs(plain, idx, vel, par, vs, opt, fcfg,
                                        vsini_grad=vg)

    def differenced():
        f0, _ = spec_fit.chisq_jobs(batch, idx, vel, par, vs, opt, cfg)
        cols = []
        for k in range(x.shape[1]):
            y = x.clone()
            y[:, k] += h[:, k]
            fk, _ = spec_fit.chisq_jobs(batch, idx, y[:, 0].contiguous(),
                                        y[:, 1:1 + ndim].contiguous(),
                                        y[:, -1].contiguous() if vg else vs, opt, cfg)
            cols.append((fk - f0) / (y[:, k] - x[:, k]))
        return f0, torch.stack(cols, dim=1)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    timed(analytic), timed(differenced)          # warm-up: tables, caches, clocks
    if plain is not None:
        timed(no_matrix)
    if args.fused:
        timed(fused)
        if plain is not None:
            timed(fused_no_matrix)
    ta, td, tn, tf, tfn = [], [], [], [], []
    for _ in range(args.rounds):
        t, (ca, ga, st) = timed(analytic)
        ta.append(t)
        t, (cd, gd) = timed(differenced)
        td.append(t)
        if plain is not None:
            tn.append(timed(no_matrix)[0])
        if args.fused:
            t, (cf, gf, sf) = timed(fused)
            tf.append(t)
            if plain is not None:
                tfn.append(timed(fused_no_matrix)[0])
    more = {}
    if args.fused:
        okf = (st == 0) & (sf == 0)
        sc = torch.maximum(ga.abs(), 1e-6 * ga.abs().max(dim=1, keepdim=True).values)
        more.update(
            fused_s_median=round(float(np.median(tf)), 6), fused_s_min=round(min(tf), 6),
            chain_over_fused_median=round(float(np.median(ta) / np.median(tf)), 3),
            differenced_over_fused_median=round(float(np.median(td) / np.median(tf)), 3),
            fused_status_equal=bool(torch.equal(st, sf)),
            fused_vs_chain_grad_max_rel=float(((gf - ga).abs() / sc)[okf].max()),
            # (... and relative to |g|_inf of the job: components at the 1e-6 floor of
            # the figure above carry the rounding of the whole sum)
            fused_vs_chain_grad_max_rel_to_norm=float(
                ((gf - ga).abs() / ga.abs().max(dim=1, keepdim=True).values)[okf].max()),
            fused_vs_chain_value_max_rel=float(
                ((cf - ca).abs() / ca.abs().clamp(min=1e3))[okf].max()))
    if tfn:
        more.update(fused_no_matrix_s_median=round(float(np.median(tfn)), 6),
                    fused_no_matrix_s_min=round(min(tfn), 6),
                    fused_resol_over_fused_no_matrix_median=round(
                        float(np.median(tf) / np.median(tfn)), 3))
    if plain is not None:
        more.update(no_matrix_s_median=round(float(np.median(tn)), 6),
                    no_matrix_s_min=round(min(tn), 6),
                    resol_over_no_matrix_median=round(
                        float(np.median(ta) / np.median(tn)), 3))
    ok = (st == 0) & torch.isfinite(gd).all(dim=1)
    scale = torch.maximum(ga.abs(), 1e-6 * ga.abs().max(dim=1, keepdim=True).values)
    rel = ((ga - gd).abs() / scale)[ok]
    print(json.dumps(dict(
        jobs=J, spectra=S, npoly=args.npoly, ndim=ndim, evaluator=args.evaluator,
        vsini=vs is not None, resolution_matrix=args.resolution_matrix,
        diagonals=11 if args.resolution_matrix else 0,
        vsini_grad=vg, rounds=args.rounds, chisq_jobs_calls=1 + x.shape[1],
        analytic_s_median=round(float(np.median(ta)), 6),
        analytic_s_min=round(min(ta), 6),
        differenced_s_median=round(float(np.median(td)), 6),
        differenced_s_min=round(min(td), 6),
        speedup_median=round(float(np.median(td) / np.median(ta)), 2),
        jobs_ok=int(ok.sum()),
        value_max_rel_diff=float(((ca - cd).abs() / cd.abs().clamp(min=1e3))[ok].max()),
        grad_vs_forward_difference_max_rel=float(rel.max()) if rel.numel() else None,
        **more)), flush=True)


if __name__ == '__main__':
    main()
