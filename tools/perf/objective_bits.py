#!/usr/bin/env python3
"""Outputs of the objective kernels' six entry points on seeded cases, for a bit
comparison of two builds:

    python tools/perf/objective_bits.py path/to/librvsgpu.so out.npz     (once per build,
                                                                  a process of its own)
    python tools/perf/objective_bits.py --compare a.npz b.npz out.json   (CPU only)

rvs_objective_fused, _fused_n, _from_template, _from_template_n: value and status per job
and the per-arm value / outside / status rows of the work buffer; rvs_objective_grad:
value, gradient, status (`grad%d`, by vsini_grad); rvs_objective_fisher wherever
engine.can_fuse_objective_fisher holds: value, gradient, Fisher matrix, status, once with
the default work buffer (`fisher%d`) and once with the one-job buffer, one launch per job
(`fisher%d/onejob`; `fisher%d/forms_agree`: the two gave the same bits).  The cases come
from the builders of the tests (tests/objective_grad_shapes.py, the jobs of
tests/chisq_grad_truth.py, the goldens of tests/conftest.py) at the smallest shapes that
reach each branch of csrc/objective.hip, csrc/objective_grad.hip and
csrc/objective_fisher.hip."""
import ctypes
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

OUT = {}
SKIPPED = {}


def put(key, *tensors):
    for i, t in enumerate(tensors):
        OUT['%s/%d' % (key, i)] = t.detach().cpu().numpy()


def call(entry, batch, libs, npoly, vel, par=None, vs=None, idx=None, rbf=True, flags=1,
         njobs=None, templs=None, outsides=None):
    """one launch through the C ABI: (out, status, armchi, armout, armst)"""
    import torch
    from rvspecfit_amd import _lib, engine
    L = _lib.lib()
    J, narm = vel.shape[0], len(batch.arms)
    arr = (_lib.ObjectiveArm * narm)()
    keep = engine.fill_objective_arms(arr, batch, libs, npoly, rbf, 0.0, None)
    dev = batch.device
    out = torch.full((J, ), -7.0, dtype=torch.float64, device=dev)
    status = torch.zeros(J, dtype=torch.int32, device=dev)
    nb = L.rvs_objective_work_size(J, narm)
    scratch = torch.zeros((nb + 7) // 8, dtype=torch.float64, device=dev)
    tail = (_lib.ptr(vel), float(batch.badchi), int(flags), _lib.ptr(scratch),
            _lib.ptr(out), _lib.ptr(status), _lib.stream())
    head = (ctypes.addressof(arr), narm, npoly)
    if templs is None:
        mid = (_lib.ptr(par), _lib.ptr(vs), _lib.ptr(idx), J)
        if entry == 'fused':
            rc = L.rvs_objective_fused(*head, *mid, *tail)
        else:
            rc = L.rvs_objective_fused_n(*head, *mid, _lib.ptr(njobs), *tail)
    else:
        tp = (ctypes.c_void_p * narm)(*[t.data_ptr() for t in templs])
        op = (ctypes.c_void_p * narm)(*[o.data_ptr() for o in outsides])
        mid = (ctypes.cast(tp, ctypes.c_void_p), ctypes.cast(op, ctypes.c_void_p),
               _lib.ptr(vs), _lib.ptr(idx), J)
        if entry == 'from_template':
            rc = L.rvs_objective_from_template(*head, *mid, *tail)
        else:
            rc = L.rvs_objective_from_template_n(*head, *mid[:-1], J, _lib.ptr(njobs),
                                                 *tail)
    _lib.check(rc, entry)
    torch.cuda.synchronize()
    del keep
    n = narm * J
    armst = scratch[2 * n:2 * n + (n + 1) // 2].view(torch.int32)[:n]
    return out, status, scratch[:n], scratch[n:2 * n], armst


def value_forms(key, batch, libs, npoly, vel, par, vs, idx, rbf=True):
    """rvs_objective_fused with the cell search in the block and from the record (the
    taps of a narrow rotational kernel: block-built and record-built), jobs in the
    caller's order and in cell order; rvs_objective_fused_n with fewer live jobs"""
    import torch
    from rvspecfit_amd import _lib
    res = {}
    for form, inblk, sort in (('inblk', 1 << 30, 1), ('record', 0, 1), ('unsorted', 0, 0)):
        with _lib.option('obj_inblk_max', inblk), _lib.option('obj_sort', sort):
            res[form] = call('fused', batch, libs, npoly, vel, par, vs, idx, rbf)
        put('%s/%s' % (key, form), *res[form])
    J = vel.shape[0]
    live = torch.tensor([max(1, (2 * J) // 3)], dtype=torch.int32, device=vel.device)
    with _lib.option('obj_inblk_max', 0):
        put(key + '/live', *call('fused_n', batch, libs, npoly, vel, par, vs, idx, rbf,
                                 njobs=live))
    # one job, whichever form evaluated it
    same = all(np.array_equal(res['inblk'][i].cpu().numpy(), res[f][i].cpu().numpy(),
                              equal_nan=True)
               for f in ('record', 'unsorted') for i in range(5))
    OUT[key + '/forms_agree'] = np.array(same)


def point_kernels(key, batch, libs, npoly, rbf, par, vs, vel, idx, vg):
    """rvs_objective_grad and, with both work buffers, rvs_objective_fisher, where each
    admits the case"""
    from rvspecfit_amd import _lib, engine
    args = (batch, libs, par, vs, vel, npoly, rbf, idx, vg)
    if engine.can_fuse_objective_grad(batch, libs, npoly=npoly, vsini_grad=vg):
        put('%s/grad%d' % (key, vg), *engine.objective_grad_fused(*args))
    if engine.can_fuse_objective_fisher(batch, libs, npoly=npoly, vsini_grad=vg):
        ntan = libs[batch.arms[0].name].ndim + int(vg)
        one = _lib.lib().rvs_objective_fisher_work_size(
            1, len(batch.arms), ntan, max(a.npix for a in batch.arms))
        full = engine.objective_fisher_fused(*args)
        single = engine.objective_fisher_fused(*args, work_bytes=one)
        put('%s/fisher%d' % (key, vg), *full)
        put('%s/fisher%d/onejob' % (key, vg), *single)
        OUT['%s/fisher%d/forms_agree' % (key, vg)] = np.array(all(
            np.array_equal(a.cpu().numpy(), b.cpu().numpy(), equal_nan=True)
            for a, b in zip(full, single)))


def shapes_cases():
    """every case of tests/objective_grad_shapes.py through rvs_objective_grad,
    rvs_objective_fisher and, in all launch forms, rvs_objective_fused; more value-kernel
    shapes on its libraries"""
    import torch
    import objective_grad_shapes as shapes
    from rvspecfit_amd import engine, spec_fit, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    C = shapes.Case
    cut, fine = shapes.cut, shapes.fine
    extra = [
        # rotational kernels: none / vsini 0 / half width 3 / 8 / 11 (8-wide trips, then
        # 4-wide) / 21; refused (R = 12.5 on 32 knots)
        C('bits-rot-cut263', 'bits', [(cut(263), 131)], 10,
          Rs=(None, 0.0, 1.6, 6.6, 9.3, 19.5), seed=301),
        C('bits-rot-refused', 'bits', [(cut(32), 16)], 5, Rs=(12.5, 1.6), seed=302),
        # 2 npix > ntp: the spline value formed again in the passes over the pixels
        C('bits-uncached-cut263', 'bits', [(cut(263), 200)], 10, Rs=(None, 1.6), seed=303),
        C('bits-uncached-linear', 'bits', [(shapes.linear(cut(263)), 200)], 7,
          Rs=(None, 1.6), seed=304),
        # chunks of 15 rows (ntp above 6658: npoly <= 4 leaves the LDS for it), and the
        # length whose chunks do not cover the template (6657: the wide kernels' loop)
        C('bits-ch15-fine6700', 'bits', [(fine(6700), 3300)], 2, Rs=(None, 1.6, 9.3),
          seed=305),
        C('bits-fine6657', 'bits', [(fine(6657), 3300)], 1, Rs=(None, 1.6, 6.6), seed=306),
    ]
    # the wave totals in the template buffer, split passes, one row buffer
    extra += [C('bits-p%d-cut873' % p, 'bits', [(cut(873), 300)], p, Rs=(None, 1.6),
                seed=310 + p) for p in (11, 14, 15, 16)]
    registered = set()
    for c in shapes.cases() + extra:
        for n, _ in c.arms:
            if n not in registered:
                spec_inter.register_library(TemplateLibrary(n, shapes.lib_dict(n)),
                                            shapes.ROOT)
                registered.add(n)
        batch = SpecBatch.from_specdata(shapes.specdata(c, spec_fit.SpecData))
        f64 = dict(dtype=torch.float64, device=batch.device)
        d = dict(batch=batch, libs=spec_inter.get_libs(batch.names, shapes.config()),
                 vs=None,
                 idx=torch.tensor([j[0] for j in c.jobs], dtype=torch.int32,
                                  device=batch.device),
                 vel=torch.tensor([j[1] for j in c.jobs], **f64),
                 par=torch.tensor([list(j[2]) for j in c.jobs], **f64))
        if any(j[3] is not None for j in c.jobs):
            d['vs'] = torch.tensor([j[3] or 0.0 for j in c.jobs], **f64)
        key = 'shapes/' + c.name
        for vg in ((False, True) if d['vs'] is not None else (False, )):
            point_kernels(key, d['batch'], d['libs'], c.npoly, c.rbf, d['par'], d['vs'],
                          d['vel'], d['idx'], vg)
        if engine.can_fuse_objective(d['batch'], d['libs'], None, npoly=c.npoly):
            value_forms(key, d['batch'], d['libs'], c.npoly, d['vel'], d['par'], d['vs'],
                        d['idx'], c.rbf)
        else:
            SKIPPED[key] = 'value kernel does not admit the case'


def _jobs(J, seed, S=1, rot=True):
    import torch
    rng = np.random.RandomState(seed)
    par = np.stack([rng.uniform(5000, 6800, J), rng.uniform(1.5, 4.5, J),
                    rng.uniform(-1.5, -0.1, J), rng.uniform(0.0, 0.4, J)], 1)
    par[::17, 0] = 9000.0          # points outside the grid: nearest neighbour
    vel = rng.uniform(-300, 300, J)
    vel[5::23] = 60000.0           # the pixels leave the knots: range status
    vs = torch.as_tensor(rng.uniform(0, 200, J)).to('cuda') if rot else None
    return (torch.as_tensor(rng.randint(0, S, J), dtype=torch.int32).to('cuda'),
            torch.as_tensor(vel).to('cuda'), torch.as_tensor(par).to('cuda'), vs)


def golden_point_jobs():
    """the jobs of tests/chisq_grad_truth.py on the golden arms (in the cell, outside the
    grid, a non-finite parameter), one and two arms, without rotation, at the jobs' own
    vsini and at rotational kernels of half width 2 .. 11 with the vsini column"""
    import torch
    import chisq_grad_truth as truth
    from conftest import GOLD, GOLD_CONFIG, gold_lib_dict
    from rvspecfit_amd import spec_fit, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, gold_lib_dict(n)), 'golden://')
    cases = dict(np.load(os.path.join(GOLD, 'cases.npz')))
    for narm in (1, 2):
        batch = SpecBatch.from_specdata(
            [sd[:narm] for sd in truth.spectra(cases, spec_fit.SpecData)])
        libs = spec_inter.get_libs(batch.names, dict(GOLD_CONFIG, template_lib='golden://'))
        f64 = dict(dtype=torch.float64, device=batch.device)
        idx = torch.tensor([j[0] for j in truth.JOBS], dtype=torch.int32,
                           device=batch.device)
        vel = torch.tensor([j[1] for j in truth.JOBS], **f64)
        par = torch.tensor([j[2] for j in truth.JOBS], **f64)
        own = torch.tensor([j[3] or 0.0 for j in truth.JOBS], **f64)
        wide = torch.tensor([r * truth.C_KMS * libs['gold_b'].lnstep for r in
                             (0.4, 1.6, 3 + 5e-4, 9.3, 0.0, 0.7, 2 - 4e-4)], **f64)
        for npoly in (1, 5, 10):
            for tag, vs, vg in (('plain', None, False), ('own', own, False),
                                ('own', own, True), ('wide', wide, True)):
                point_kernels('point/arms%d/p%d/%s' % (narm, npoly, tag), batch, libs,
                              npoly, True, par, vs, vel, idx, vg)


def golden_cases():
    """the golden spectra: launches in cell order (J >= 512), sum flags, grid sets with
    pen_scale, resolution bands, templates from HBM, a library with a NaN row"""
    import torch
    from conftest import GOLD, GOLD_CONFIG, gold_lib_dict, gold_specdata
    from rvspecfit_amd import _lib, spec_fit, spec_inter
    from rvspecfit_amd.engine import SpecBatch
    from rvspecfit_amd.library import TemplateLibrary
    from test_resol_objective import _band
    for n in ('gold_b', 'gold_r'):
        spec_inter.register_library(TemplateLibrary(n, gold_lib_dict(n)), 'golden://')
    cases = dict(np.load(os.path.join(GOLD, 'cases.npz')))
    cfg = dict(GOLD_CONFIG, template_lib='golden://')
    base = gold_specdata(cases, 'c1', spec_fit.SpecData)
    b, _ = spec_fit.as_batch(base)
    libs = spec_inter.get_libs(b.names, cfg)
    idx, vel, par, vs = _jobs(600, 11)
    for npoly in (10, 12):
        value_forms('gold/J600/p%d' % npoly, b, libs, npoly, vel, par, vs, idx)
    # the sum kernel's flags: no outside penalty, status stored, arms not summed
    idx, vel, par, vs = _jobs(40, 12)
    for flags in (0, 1, 3, 4, 5):
        put('gold/flags%d' % flags, *call('fused', b, libs, 10, vel, par, vs, idx,
                                          flags=flags))
    # templates from HBM (rows of any evaluator), outside flags 0 / > 0 / > 0 with a NaN
    # in the row / an all-zero row (no positive pivot)
    J = 24
    idx, vel, par, vs = _jobs(J, 13)
    rng = np.random.RandomState(14)
    templs, outs = [], []
    for arm in b.arms:
        ntp = libs[arm.name].ntp
        t = 1.0 + 0.2 * np.sin(np.arange(ntp)[None, :] * 0.05 + rng.uniform(0, 6, (J, 1)))
        o = np.zeros(J)
        o[3::6] = 0.25
        t[9, ntp // 2] = np.nan
        t[4] = 0.0
        templs.append(torch.as_tensor(t).to('cuda').contiguous())
        outs.append(torch.as_tensor(o).to('cuda'))
    live = torch.tensor([17], dtype=torch.int32, device='cuda')
    for npoly in (2, 10, 15):
        for v in (None, vs):
            k = 'gold/templ/p%d/rot%d' % (npoly, v is not None)
            put(k, *call('from_template', b, libs, npoly, vel, vs=v, idx=idx,
                         templs=templs, outsides=outs))
            put(k + '/live', *call('from_template_n', b, libs, npoly, vel, vs=v, idx=idx,
                                   templs=templs, outsides=outs, njobs=live))
    # a grid node whose row holds a NaN, as the nearest node of a point outside the grid
    d = {k: v for k, v in gold_lib_dict('gold_b').items() if not k.startswith('ccf')}
    dats = np.array(d['dats'])
    far = int(np.argmax(np.asarray(d['vec'])[0]))     # a node of the hottest teff
    dats[far, 100] = np.nan
    d['dats'] = dats
    spec_inter.register_library(TemplateLibrary('gold_b', d), 'golden-nan://')
    sdb = [s for s in base if s.name == 'gold_b']
    bn, _ = spec_fit.as_batch(sdb)
    libn = spec_inter.get_libs(bn.names, dict(cfg, template_lib='golden-nan://'))
    idx, vel, par, vs = _jobs(34, 15)
    par[::17, 0] = 20000.0
    par[::17, 1:] = torch.as_tensor(np.asarray(d['vec'])[1:, far]).to('cuda')
    value_forms('gold/nan-row', bn, libn, 10, vel, par, vs, idx)
    # resolution bands of 1, 3, 11, 33 diagonals on one arm, none on the other; three
    # spectra with matrices of their own
    for nd in (1, 3, 11, 33):
        rng = np.random.RandomState(nd)
        many = [[spec_fit.SpecData(
            sd.name, sd.lam, sd.spec * (1 + 0.01 * rng.normal(size=len(sd.lam))), sd.espec,
            badmask=sd.badmask,
            resolution=_band(len(sd.lam), nd, 100 * nd + 10 * s) if ia == 0 else None)
            for ia, sd in enumerate(base)] for s in range(3)]
        br = SpecBatch.from_specdata(many)
        libr = spec_inter.get_libs(br.names, cfg)
        idx, vel, par, vs = _jobs(40, 20 + nd, S=3)
        for npoly in (10, 12):
            value_forms('gold/resol%d/p%d' % (nd, npoly), br, libr, npoly, vel, par, vs,
                        idx)
    # a grid set (G > 1: per-spectrum grids, pen_scale), with and without bands
    sd = [s for s in base if s.name == 'gold_r'][0]
    cuts = [(0, 301, 9), (0, 280, 13), (12, 290, 21), (5, 301, 11)]
    for banded in (False, True):
        sds = [[spec_fit.SpecData('gold_r', sd.lam[a:z], sd.spec[a:z], sd.espec[a:z],
                                  badmask=sd.badmask[a:z],
                                  resolution=_band(z - a, nd, 50 + i) if banded else None)]
               for i, (a, z, nd) in enumerate(cuts)]
        bg = SpecBatch.from_specdata(sds)
        assert bg.arms[0].G > 1 and bg.pen_scale is not None
        libg = spec_inter.get_libs(bg.names, cfg)
        idx, vel, par, vs = _jobs(60, 30, S=len(cuts))
        value_forms('gold/gridset%d' % banded, bg, libg, 10, vel, par, vs, idx)


def five_dimensions():
    """a 5-D grid (32 vertices: the cell search is always in the block): gold_b's rows
    twice along a fifth axis, the second copy scaled"""
    import torch
    from conftest import GOLD, GOLD_CONFIG, gold_lib_dict, gold_specdata
    from rvspecfit_amd import engine, spec_fit, spec_inter
    from rvspecfit_amd.library import TemplateLibrary
    d = {k: v for k, v in gold_lib_dict('gold_b').items() if not k.startswith('ccf')}
    idg = np.asarray(d['idgrid'])
    nrow = np.asarray(d['dats']).shape[0]
    d['idgrid'] = np.stack([idg, np.where(idg >= 0, idg + nrow, -1)], axis=-1)
    d['dats'] = np.concatenate([d['dats'], np.asarray(d['dats']) * np.float32(1.01)])
    vec = np.asarray(d['vec'])
    d['vec'] = np.concatenate([np.concatenate([vec, np.zeros((1, nrow))]),
                               np.concatenate([vec, np.ones((1, nrow))])], axis=1)
    d['uvec4'] = np.array([0.0, 1.0])
    d['parnames'] = np.array(list(d['parnames']) + ['x5'])
    if 'logmask' in d:
        d['logmask'] = np.array(list(d['logmask']) + [False])
    spec_inter.register_library(TemplateLibrary('gold_b', d), 'golden-5d://')
    cases = dict(np.load(os.path.join(GOLD, 'cases.npz')))
    sdb = [s for s in gold_specdata(cases, 'c1', spec_fit.SpecData) if s.name == 'gold_b']
    b, _ = spec_fit.as_batch(sdb)
    libs = spec_inter.get_libs(b.names, dict(GOLD_CONFIG, template_lib='golden-5d://'))
    assert libs['gold_b'].ndim == 5
    idx, vel, par, vs = _jobs(34, 40)
    par = torch.cat([par, torch.linspace(0.05, 0.95, 34, dtype=torch.float64,
                                         device='cuda')[:, None]], 1).contiguous()
    put('gold/5d', *call('fused', b, libs, 10, vel, par, vs, idx))


def compare(a, b, out):
    A, B = np.load(a), np.load(b)
    keys = sorted(k for k in A.files if not k.startswith('meta/'))
    assert keys == sorted(k for k in B.files if not k.startswith('meta/')), 'other arrays'
    differ = [k for k in keys if A[k].shape != B[k].shape or
              A[k].tobytes() != B[k].tobytes()]
    forms = [k for k in keys if k.endswith('/forms_agree')]
    rec = dict(arrays=len(keys), differ=len(differ), differing=differ[:20],
               launch_forms_checked=len(forms),
               launch_forms_disagree=[k for k in forms if not (A[k] and B[k])],
               skipped={n: json.loads(str(X['meta/skipped'])) for n, X in
                        (('a', A), ('b', B))})
    json.dump(rec, open(out, 'w'), indent=1, sort_keys=True)
    print(json.dumps(rec, sort_keys=True))
    return 1 if differ else 0


def main():
    if sys.argv[1] == '--compare':
        sys.exit(compare(*sys.argv[2:5]))
    from rvspecfit_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    _lib.require_gpu()
    rc = 0
    for part in (shapes_cases, golden_point_jobs, golden_cases, five_dimensions):
        try:
            with np.errstate(all='ignore'):
                part()
        except Exception as e:
            SKIPPED[part.__name__] = '%s: %s' % (type(e).__name__, e)
            print('part %s stopped: %r' % (part.__name__, e), flush=True)
            # a case this script built wrongly ends its part; anything else (an error
            # of the device or the library) ends the run with what there is
            if not isinstance(e, (ValueError, KeyError, TypeError, IndexError,
                                  AttributeError, AssertionError)):
                rc = 3
                break
    OUT['meta/skipped'] = np.array(json.dumps(SKIPPED))
    np.savez(sys.argv[2], **OUT)
    print('%d arrays, skipped: %s' % (len(OUT) - 1, SKIPPED))
    sys.exit(rc)


if __name__ == '__main__':
    main()
