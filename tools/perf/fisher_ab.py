#!/usr/bin/env python3
"""Value + gradient + Fisher matrix of the objective for J jobs: ONE
spec_fit.chisq_fisher_jobs call against ONE spec_fit.chisq_grad_jobs call on the same
jobs, and against vel_fit.param_uncertainties (the finite-difference Hessian of the
stellar parameters: 33+ objective evaluations per spectrum) on the same S spectra.
usage: fisher_ab.py [--jobs J] [--spectra S] [--npoly P] [--rounds R] [--vsini-grad]
                    [--resolution-matrix] [--fused]
--fused: a fourth leg, the same chisq_fisher_jobs call under config['fused_fisher']
(rvs_objective_fisher: one forward-mode kernel per (job, arm)), alternating with the
others; the line then carries its seconds, its ratio to the chain's Fisher call of the
same round set and its largest differences from the chain's results.  (Profile kept:
profiles/fisher_fused_ab_8192.json.)
--resolution-matrix: every spectrum carries resolution matrices of 11 diagonals
(tools/perf/_resol.py, as resol_ab.py builds them) and all three run under them, the
first two with config['resol_gradient'] (rvs_chisq_point_fisher_resol / _grad_resol).
The workload is bench.py's (its synthetic DESI-shape 3-arm libraries and spectra); the
jobs are its truth parameters, jittered inside the grid, spread over the S spectra; the
Hessian is taken at the first S jobs (one per spectrum).  The three run alternately in
one process, R rounds after a warm-up; one JSON line: median and minimum seconds of
each, the ratio Fisher call / gradient call, the shares of spectra with bad_fisher (the
host inversion of the first S jobs' matrices) and with bad_hessian, and sanity figures
of the matrices (asymmetry, smallest eigenvalue after scaling by the diagonal)."""
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
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--vsini-grad', action='store_true')
    ap.add_argument('--resolution-matrix', action='store_true')
    ap.add_argument('--fused', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import numpy as np
    import torch
    import bench
    from rvspecfit_amd import _lib, engine, spec_fit, spec_inter, vel_fit
    from rvspecfit_amd.library import TemplateLibrary
    _lib.require_gpu()
    dev = torch.device('cuda', 0)
    S, J = args.spectra, args.jobs

    def gpu_convolve(lam, templ, vsini):
        t = torch.as_tensor(np.ascontiguousarray(templ)).to(dev)
        v = torch.as_tensor(np.ascontiguousarray(vsini)).to(dev)
        return engine.convolve_vsini(lam, t, v).cpu().numpy()

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
    vs = torch.full((J, ), 20.0, dtype=torch.float64, device=dev) if vg else None

    def fisher():
        return spec_fit.chisq_fisher_jobs(batch, idx, vel, par, vs, opt, cfg,
                                          vsini_grad=vg)

    def fused():
        return spec_fit.chisq_fisher_jobs(batch, idx, vel, par, vs, opt,
                                          dict(cfg, fused_fisher=True), vsini_grad=vg)

    def gradient():
        return spec_fit.chisq_grad_jobs(batch, idx, vel, par, vs, opt, cfg,
                                        vsini_grad=vg)

    def hessian():
        return vel_fit.param_uncertainties(batch, vel[:S], par[:S].contiguous(),
                                           vsini=None if vs is None else vs[:S],
                                           options=opt, config=cfg)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    timed(fisher), timed(gradient), timed(hessian)   # warm-up: tables, caches, clocks
    if args.fused:
        timed(fused)
    tf, tg, th, tu = [], [], [], []
    for _ in range(args.rounds):
        t, (cf, gf, F, stf) = timed(fisher)
        tf.append(t)
        if args.fused:
            t, (cu, gu, Fu, stu) = timed(fused)
            tu.append(t)
        t, (cg, gg, stg) = timed(gradient)
        tg.append(t)
        t, hs = timed(hessian)
        th.append(t)
    same = bool(torch.equal(cf, cg) and torch.equal(gf, gg) and torch.equal(stf, stg))
    nm = ['vel'] + names + (['vsini'] if vg else [])
    fu = vel_fit._uncertainties_from_fisher(F[:S].cpu().numpy(), nm, names)
    Fn = F.cpu().numpy()
    d = np.sqrt(np.clip(np.diagonal(Fn, axis1=1, axis2=2), 1e-300, None))
    ev = np.linalg.eigvalsh(Fn / (d[:, :, None] * d[:, None, :]))
    med = lambda v: round(float(np.median(v)), 6)   # noqa: E731
    more = {}
    if args.fused:
        Fun = Fu.cpu().numpy()
        relF = np.abs(Fun - Fn) / (d[:, :, None] * d[:, None, :])
        gn, gun = gf.cpu().numpy(), gu.cpu().numpy()
        relg = np.abs(gun - gn) / np.maximum(np.abs(gn), 1e-6 * np.abs(gn).max(
            axis=1, keepdims=True))
        more = dict(
            fused_s_median=med(tu), fused_s_min=round(min(tu), 6),
            fused_s_all=[round(x, 6) for x in tu], fisher_s_all=[round(x, 6) for x in tf],
            fused_over_fisher_median=round(float(np.median(tu) / np.median(tf)), 3),
            fused_over_grad_median=round(float(np.median(tu) / np.median(tg)), 3),
            fused_status_equal=bool(torch.equal(stu, stf)),
            fused_value_bits_equal=bool(torch.equal(cu, cf)),
            fused_value_max_rel=float(((cu - cf).abs() / cf.abs().clamp(min=1e3)).max()),
            fused_fisher_max_err_of_sqrt_FiiFll=float(np.nanmax(relF)),
            fused_grad_max_rel=float(np.nanmax(relg)),
            fused_asymmetry_max=float(np.abs(Fun - Fun.transpose(0, 2, 1)).max()))
    print(json.dumps(dict(
        jobs=J, spectra=S, npoly=args.npoly, ndim=ndim, vsini_grad=vg, rounds=args.rounds,
        resolution_matrix=args.resolution_matrix,
        diagonals=11 if args.resolution_matrix else 0,
        fisher_s_median=med(tf), fisher_s_min=round(min(tf), 6),
        grad_s_median=med(tg), grad_s_min=round(min(tg), 6),
        fisher_over_grad_median=round(float(np.median(tf) / np.median(tg)), 3),
        param_uncertainties_s_median=med(th), param_uncertainties_s_min=round(min(th), 6),
        value_and_gradient_bits_equal=same,
        bad_fisher_share=float(np.mean(fu['bad_fisher'])),
        bad_hessian_share=float(np.mean(hs['bad_hessian'])),
        fisher_asymmetry_max=float(np.abs(Fn - Fn.transpose(0, 2, 1)).max()),
        fisher_scaled_min_eigenvalue=float(ev.min()), **more)), flush=True)


if __name__ == '__main__':
    main()
