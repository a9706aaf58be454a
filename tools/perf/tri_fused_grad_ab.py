#!/usr/bin/env python3
"""Value and gradient of the objective on Delaunay libraries, three legs alternating in
one process:
  differenced   the 2 + ndim spec_fit.chisq_jobs calls of a forward difference
  chain         spec_fit.chisq_grad_jobs (forward mode: rvs_template_tri_buckets_grad ->
                FIR -> spline construct -> rvs_chisq_point_grad)
  fused         the same call with config['fused_gradient'] and config['tri_gradient']
                (reverse mode: rvs_template_tri_buckets ->
                rvs_objective_grad_from_template -> rvs_template_tri_vjp ->
                rvs_objective_grad_join)
usage: tri_fused_grad_ab.py [--jobs J] [--spectra S] [--npoly P] [--rounds R] [--once LEG]
                            [--out FILE]
The workload is that of bench.py --evaluator tri: its seeded DESI-shape Delaunay libraries
on the three arms, J jobs over S spectra at jittered truth parameters.  R rounds after a
warm-up; one JSON line (also written to FILE) with the median, minimum and maximum seconds
of each leg, their ratios, and the largest difference of value and gradient between the
two exact legs (relative to max(|g_k|, 1e-6 |g|_inf), with the size of the component
where it occurs, and relative to the job's largest component).  --once LEG: that leg alone, once after a warm-up, for a kernel trace
run of its own (rocprofv3 --kernel-trace --stats -- python tri_fused_grad_ab.py --once
fused)."""
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
    ap.add_argument('--once', choices=['differenced', 'chain', 'fused'], default=None)
    ap.add_argument('--out', default=None)
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

    S, J = args.spectra, args.jobs
    bench.EVALUATOR = 'tri'

    def gpu_convolve(lam, templ, vsini):
        t = torch.as_tensor(np.ascontiguousarray(templ)).to(dev)
        v = torch.as_tensor(np.ascontiguousarray(vsini)).to(dev)
        return engine.convolve_vsini(lam, t, v).cpu().numpy()
    for name, d in bench.build_library_dicts(64, gpu_convolve).items():
        spec_inter.register_library(TemplateLibrary(name, d, device=dev),
                                    bench.CONFIG['template_lib'])
    tp = bench.truth_params(S, seed=3)
    cfg = dict(bench.CONFIG)
    both = dict(cfg, fused_gradient=True, tri_gradient=True)
    batch = engine.SpecBatch([engine.ArmData(n, lam, sp, es, bad, device=dev)
                              for n, lam, sp, es, bad in
                              bench.make_spectra_device(tp, dev)])
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
    nd = par.shape[1]
    pts = [(vel, par), (vel + 1e-2, par)]
    for k in range(nd):
        q = par.clone()
        q[:, k] *= 1 + 1e-6
        pts.append((vel, q))
    legs = dict(
        differenced=lambda: [spec_fit.chisq_jobs(batch, idx, v, q, None, opt, cfg)
                             for v, q in pts],
        chain=lambda: spec_fit.chisq_grad_jobs(batch, idx, vel, par, None, opt, cfg),
        fused=lambda: spec_fit.chisq_grad_jobs(batch, idx, vel, par, None, opt, both))
    if args.once:
        timed(legs[args.once])
        t, _ = timed(legs[args.once])
        print(json.dumps(dict(what='tri_fused_grad_ab --once', leg=args.once, jobs=J,
                              s=round(t, 6))), flush=True)
        return
    for f in legs.values():
        timed(f)
    ts = {k: [] for k in legs}
    res = {}
    for _ in range(args.rounds):
        for k, f in legs.items():
            t, res[k] = timed(f)
            ts[k].append(t)
    (c0, g0, s0), (c1, g1, s1) = res['chain'], res['fused']
    floor = torch.maximum(g0.abs(), 1e-6 * g0.abs().amax(dim=1, keepdim=True))
    med = {k: float(np.median(v)) for k, v in ts.items()}
    # (where the two exact legs differ most in the floor's metric: how large that
    # component is beside the largest of its job)
    rel = (g1 - g0).abs() / floor
    at = int(rel.argmax())
    size = (g0.abs() / g0.abs().amax(dim=1, keepdim=True)).flatten()[at]
    line = json.dumps(dict(
        what='chisq_grad_jobs on Delaunay libraries: differenced, chain, fused + VJP',
        jobs=J, spectra=S, npoly=args.npoly, arms=len(batch.arms), rounds=args.rounds,
        value_calls=len(pts),
        s_median={k: round(v, 6) for k, v in med.items()},
        s_min={k: round(min(v), 6) for k, v in ts.items()},
        s_max={k: round(max(v), 6) for k, v in ts.items()},
        fused_over_chain=round(med['fused'] / med['chain'], 4),
        fused_over_differenced=round(med['fused'] / med['differenced'], 4),
        status_equal=bool(torch.equal(s0, s1)),
        value_max_rel_diff=float(((c1 - c0).abs() / c0.abs()).max().item()),
        grad_max_rel_diff=float(rel.max().item()),
        grad_max_rel_diff_at=dict(job=at // g0.shape[1], component=at % g0.shape[1],
                                  size_of_job_norm=float(size.item())),
        grad_max_diff_of_job_norm=float(
            ((g1 - g0).abs() / g0.abs().amax(dim=1, keepdim=True)).max().item()),
        jobs_ok=int(((s1 == 0) & torch.isfinite(g1).all(dim=1)).sum())))
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
