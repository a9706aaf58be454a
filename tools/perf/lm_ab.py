#!/usr/bin/env python3
"""The polish of vel_fit.process on S spectra, three ways: the forward-difference BFGS
(rvs_bfgs_run), BFGS on the analytic gradient (rvs_bfgs_run_grad,
config['second_minimizer_jac']) and Levenberg-Marquardt on the Fisher matrix (rvs_lm_run,
config['second_minimizer_lm']), alternating, in one process.
usage: lm_ab.py [--spectra S] [--npoly P] [--rounds R] [--evaluator polylinear|tri]
                [--tau T] [--resolution-matrix] [--fused]
--fused: two more legs in every round -- Levenberg-Marquardt on the rows of
rvs_objective_fisher (rvs_lm_run_fused, config['fused_fisher']) and BFGS on the rows of
rvs_objective_grad (rvs_bfgs_run_grad_fused, config['fused_gradient']); the line then
carries both and their ratios to the legs of the same rounds.  (Profile kept:
profiles/lm_fused_ab_2000.json.)
--resolution-matrix: every spectrum carries resolution matrices of 11 diagonals
(tools/perf/_resol.py, as resol_ab.py builds them); the differenced polish runs through
the objective kernel's band, the other two through config['resol_gradient'].
The workload is bench.py's, built as `bench.py --process` builds it (its synthetic
DESI-shape libraries and seeded spectra, the start parameters from the CCF stage of
pipeline.fit_batch).  vel_fit.process runs once without the second minimiser; its
simplex optimum is the start of all three polishes, which then run on ONE
optimizer.ProcessObjective as the polish stage of process runs them (get_hess_inv's
hess_inv0 and scipy's constants for BFGS, the machine's defaults for LM, gtol 1e-5 for
all).  R rounds after a warm-up, the modes taking turns inside every round; one JSON
line: stage seconds per mode (median, minimum), rows, rounds and nit per spectrum, the
histogram of statuses per mode, and the distribution of f_lm - f_fd and f_lm - f_jac at
the end (negative: LM ended lower).  Times are to be held against the differenced polish
of the SAME line, never against a number from another day.  (Profile kept:
profiles/lm_ab_2000.json.)"""
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
    ap.add_argument('--evaluator', choices=['polylinear', 'tri'], default='polylinear')
    ap.add_argument('--tau', type=float, default=1e-3)
    ap.add_argument('--resolution-matrix', action='store_true')
    ap.add_argument('--fused', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import bench
    from rvspecfit_amd import _lib, bfgs, engine, lm, optimizer, pipeline, spec_inter
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
                              bench.make_spectra_device(tp, dev)])
    cfg, opt = dict(bench.CONFIG), dict(bench.OPTIONS, npoly=args.npoly)
    if args.resolution_matrix:
        import _resol
        _resol.attach(batch, S, dev)
        cfg['resol_gradient'] = True
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
    fchain = optimizer.GradChain(pobj, fisher=True)

    def fd():
        return bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=hess_inv0)

    def jac():
        return bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=hess_inv0, jac=True,
                                             chain=chain)

    def lmq():
        return lm.minimize_lockstep_device(pobj, x0, tau=args.tau, chain=fchain)

    if args.fused:
        gchain = optimizer.GradChain(pobj, fused=True)
        uchain = optimizer.GradChain(pobj, fused_fisher=True)

    def jac_fused():
        return bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=hess_inv0, jac=True,
                                             chain=gchain)

    def lm_fused():
        return lm.minimize_lockstep_device(pobj, x0, tau=args.tau, chain=uchain)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    timed(fd), timed(jac), timed(lmq)          # warm-up
    if args.fused:
        timed(jac_fused), timed(lm_fused)
    t_fd, t_jac, t_lm, t_jf, t_lf = [], [], [], [], []
    for _ in range(args.rounds):
        if args.fused:
            t, e = timed(lm_fused)
            t_lf.append(t)
            t, g = timed(jac_fused)
            t_jf.append(t)
        t, a = timed(fd)
        t_fd.append(t)
        t, b = timed(jac)
        t_jac.append(t)
        t, c = timed(lmq)
        t_lm.append(t)

    def per(res, k):
        x = res[k].double()
        return dict(mean=round(float(x.mean()), 2), median=float(x.median()),
                    max=int(x.max()))

    def hist(res):
        return np.bincount(res['status'].cpu().numpy(), minlength=4).tolist()

    def mode(ts, res, **more):
        return dict(stage_s_median=round(float(np.median(ts)), 4),
                    stage_s_min=round(min(ts), 4), lockstep_rounds=res['rounds'],
                    rows_launched=res['rows_launched'],
                    rows_per_spectrum=round(res['rows_launched'] / S, 2),
                    nit=per(res, 'nit'), nfev=per(res, 'nfev'),
                    status_counts=hist(res), **more)

    q = [0, 1, 5, 25, 50, 75, 95, 99, 100]

    def dist(hi, lo):
        d = (hi['fun'] - lo['fun']).cpu().numpy()
        return dict(percentiles={str(p): float(np.percentile(d, p)) for p in q},
                    lm_lower=int((d < 0).sum()), equal=int((d == 0).sum()),
                    lm_higher=int((d > 0).sum()), mean=float(d.mean()))

    more = {}
    if args.fused:
        more = dict(
            lm_fused=mode(t_lf, e, mu_median=float(e['mu'].median()),
                          stage_s_all=[round(x, 4) for x in t_lf],
                          work_bytes=uchain.nbytes),
            jac_fused=mode(t_jf, g, njev=per(g, 'njev'),
                           stage_s_all=[round(x, 4) for x in t_jf]),
            lm_stage_s_all=[round(x, 4) for x in t_lm],
            lm_fused_over_lm_time=round(float(np.median(t_lf) / np.median(t_lm)), 3),
            lm_fused_over_jac_fused_time=round(float(np.median(t_lf) / np.median(t_jf)), 3),
            lm_fused_over_fd_time=round(float(np.median(t_lf) / np.median(t_fd)), 3),
            jac_fused_over_fd_time=round(float(np.median(t_jf) / np.median(t_fd)), 3),
            f_lmfused_minus_f_lm=dist(e, c), f_lmfused_minus_f_jacfused=dist(e, g))
    print(json.dumps(dict(
        spectra=S, npoly=args.npoly, evaluator=args.evaluator, rounds=args.rounds,
        resolution_matrix=args.resolution_matrix,
        diagonals=11 if args.resolution_matrix else 0, objective=pobj.form,
        n=len(cols), tau=args.tau, chain_cap=chain.cap, chain_bytes=chain.nbytes,
        fisher_chain_cap=fchain.cap, fisher_chain_bytes=fchain.nbytes,
        fd=mode(t_fd, a), jac=mode(t_jac, b, njev=per(b, 'njev')),
        lm=mode(t_lm, c, mu_median=float(c['mu'].median())),
        jac_over_fd_time=round(float(np.median(t_jac) / np.median(t_fd)), 3),
        lm_over_fd_time=round(float(np.median(t_lm) / np.median(t_fd)), 3),
        f_lm_minus_f_fd=dist(c, a), f_lm_minus_f_jac=dist(c, b), **more)), flush=True)


if __name__ == '__main__':
    main()
