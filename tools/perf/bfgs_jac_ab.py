#!/usr/bin/env python3
"""The BFGS polish of vel_fit.process on S spectra: the forward-difference polish
(rvs_bfgs_run) against the polish on the analytic gradient (rvs_bfgs_run_grad,
config['second_minimizer_jac']), alternating, in one process.
usage: bfgs_jac_ab.py [--spectra S] [--npoly P] [--rounds R] [--evaluator polylinear|tri|nn]
                      [--fused] [--resolution-matrix]
--fused: a third polish, the analytic gradient from rvs_objective_grad
(rvs_bfgs_run_grad_fused, config['fused_gradient']), alternating with the two.
--evaluator nn: bench.py's MLP libraries; the chain then runs with config['nn_gradient']
and --fused through rvs_bfgs_run_grad_fused_nn.
--evaluator tri: bench.py's Delaunay libraries; --fused then runs with
config['tri_gradient'] through rvs_bfgs_run_grad_fused_tri.
--resolution-matrix: every spectrum carries resolution matrices of 11 diagonals
(tools/perf/_resol.py, what `bench.py --resolution-matrix` puts on its batch) and every
polish runs with config['resol_gradient']: the differenced one on the value kernel's
band, the chain through rvs_chisq_point_grad_resol, --fused through
rvs_bfgs_run_grad_fused_resol.
The workload is bench.py's, built as `bench.py --process` builds it (its synthetic
DESI-shape libraries and seeded spectra, the start parameters from the CCF stage of
pipeline.fit_batch).  vel_fit.process runs once without the second minimiser; its
simplex optimum is the start of both polishes, which then run on ONE
optimizer.ProcessObjective with get_hess_inv's hess_inv0 and scipy's default gtol and
Wolfe constants, as the BFGS stage of process runs them.  R rounds after a warm-up;
one JSON line: stage seconds per mode (median, minimum, maximum), nit / nfev / njev per
spectrum, the histogram of scipy's statuses per mode, and the distribution of f_jac - f_fd at the
end (negative: the jac polish ended lower)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--spectra', type=int, default=2000)
    ap.add_argument('--npoly', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--evaluator', choices=['polylinear', 'tri', 'nn'], default='polylinear')
    ap.add_argument('--fused', action='store_true')
    ap.add_argument('--resolution-matrix', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import bench
    from rvspecfit_amd import _lib, bfgs, engine, optimizer, pipeline, spec_inter
    from rvspecfit_amd import vel_fit
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    dev = torch.device('cuda', 0)
    S = args.spectra

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
                              (bench.make_spectra_device(tp, dev) if args.evaluator != 'nn'
                               else bench.make_spectra_from_library(tp, dev, bench.CONFIG))])
    cfg, opt = dict(bench.CONFIG), dict(bench.OPTIONS, npoly=args.npoly)
    if args.resolution_matrix:
        import _resol
        _resol.attach(batch, S, dev)
        cfg['resol_gradient'] = True
    if args.evaluator == 'nn':
        cfg['nn_gradient'] = True
    if args.evaluator == 'tri' and args.fused:
        cfg['tri_gradient'] = True     # (read by GradChain(fused=True) alone)
    # the start of process: the CCF stage's parameters (bench.run_process_addon)
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
    hess_inv0 = vel_fit.get_hess_inv(cols)
    libs = spec_inter.get_libs(batch.names, cfg)
    pdt = {k: t.double().contiguous() for k, t in pd0.items()}
    safe = torch.stack([pdt[k] for k in names], dim=1).contiguous()
    pobj = optimizer.ProcessObjective(batch, libs, names, pdt, [], True, cfg, opt, None,
                                      safe)
    chain = optimizer.GradChain(pobj)

    def fd():
        return bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=hess_inv0)

    def jac():
        return bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=hess_inv0, jac=True,
                                             chain=chain)

    fchain = optimizer.GradChain(pobj, fused=True) if args.fused else None

    def fused():
        return bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=hess_inv0, jac=True,
                                             chain=fchain)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    timed(fd), timed(jac)          # warm-up
    if args.fused:
        timed(fused)
    t_fd, t_jac, t_fu = [], [], []
    for _ in range(args.rounds):
        t, a = timed(fd)
        t_fd.append(t)
        t, b = timed(jac)
        t_jac.append(t)
        if args.fused:
            t, c = timed(fused)
            t_fu.append(t)

    def per(res, k):
        x = res[k].double()
        return dict(mean=round(float(x.mean()), 2), median=float(x.median()),
                    max=int(x.max()))

    def hist(res):
        return np.bincount(res['status'].cpu().numpy(), minlength=4).tolist()

    d = (b['fun'] - a['fun']).cpu().numpy()
    q = [0, 1, 5, 25, 50, 75, 95, 99, 100]
    more = {}
    if args.fused:
        df = (c['fun'] - a['fun']).cpu().numpy()
        dj = (c['fun'] - b['fun']).cpu().numpy()
        more = dict(
            fused=dict(stage_s_median=round(float(np.median(t_fu)), 4),
                       stage_s_min=round(min(t_fu), 4),
                       stage_s_max=round(max(t_fu), 4), lockstep_rounds=c['rounds'],
                       rows_launched=c['rows_launched'], nit=per(c, 'nit'),
                       nfev=per(c, 'nfev'), njev=per(c, 'njev'), status_counts=hist(c),
                       work_bytes=fchain.nbytes),
            fused_over_fd_time=round(float(np.median(t_fu) / np.median(t_fd)), 3),
            fused_over_jac_time=round(float(np.median(t_fu) / np.median(t_jac)), 3),
            f_fused_minus_f_fd=dict(
                percentiles={str(p): float(np.percentile(df, p)) for p in q},
                fused_lower=int((df < 0).sum()), equal=int((df == 0).sum()),
                fused_higher=int((df > 0).sum()), mean=float(df.mean())),
            f_fused_minus_f_jac_abs_max=float(np.abs(dj).max()),
            f_fused_equals_f_jac=int((dj == 0).sum()))
    print(json.dumps(dict(
        spectra=S, npoly=args.npoly, evaluator=args.evaluator, rounds=args.rounds,
        resolution_matrix=args.resolution_matrix,
        n=len(cols), chain_cap=chain.cap, chain_bytes=chain.nbytes,
        fd=dict(stage_s_median=round(float(np.median(t_fd)), 4),
                stage_s_min=round(min(t_fd), 4), stage_s_max=round(max(t_fd), 4),
                lockstep_rounds=a['rounds'],
                rows_launched=a['rows_launched'], nit=per(a, 'nit'),
                nfev=per(a, 'nfev'), status_counts=hist(a)),
        jac=dict(stage_s_median=round(float(np.median(t_jac)), 4),
                 stage_s_min=round(min(t_jac), 4), stage_s_max=round(max(t_jac), 4),
                 lockstep_rounds=b['rounds'],
                 rows_launched=b['rows_launched'], nit=per(b, 'nit'),
                 nfev=per(b, 'nfev'), njev=per(b, 'njev'), status_counts=hist(b)),
        jac_over_fd_time=round(float(np.median(t_jac) / np.median(t_fd)), 3),
        f_jac_minus_f_fd=dict(
            percentiles={str(p): float(np.percentile(d, p)) for p in q},
            jac_lower=int((d < 0).sum()), equal=int((d == 0).sum()),
            jac_higher=int((d > 0).sum()), mean=float(d.mean())), **more)), flush=True)


if __name__ == '__main__':
    main()
