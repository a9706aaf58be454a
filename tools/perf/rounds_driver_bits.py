#!/usr/bin/env python3
"""Results and statistics of the entry points behind the round driver (csrc/rounds_dev.h),
for a bit comparison of two builds:

    python tools/perf/rounds_driver_bits.py path/to/librvsgpu.so out.npz   (once per build,
                                                                    a process of its own)
    python tools/perf/rounds_driver_bits.py --compare a.npz b.npz out.json  (CPU only)

The runs of tests/test_rounds_driver_gpu.py (tests/rounds_driver_cases.py): rvs_bfgs_run,
rvs_bfgs_run_grad, rvs_bfgs_run_grad_fused, rvs_lm_run and rvs_lm_run_fused on five
spectra in chunks of three rows, the host looking every 1, 4 and 9 rounds; the 640 runs of
rvs_bfgs_run whose first rounds are above the one-look-per-round threshold, looking every
1 and 4 rounds; and, where tests/golden holds its network, rvs_bfgs_run_grad_fused_nn on
the two spectra of tests/test_nn_vjp_gpu.py.  Per run: every result array, and `stats` =
(rounds, objective calls, rows launched) -- equal statistics say that the host looked and
launched at the same moments."""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]

OUT = {}
SKIPPED = {}


def put(key, r, keys):
    import rounds_driver_cases as rc
    for k in keys:
        OUT['%s/%s' % (key, k)] = np.asarray(r[k])
    OUT[key + '/stats'] = np.array([int(r[k]) for k in rc.STATS], dtype=np.int64)
    print(key, {k: int(r[k]) for k in rc.STATS}, flush=True)


def driver_cases():
    import rounds_driver_cases as rc
    import test_bfgs_jac_gpu as tj
    cases = dict(np.load(os.path.join(REPO, 'tests', 'golden', 'cases.npz')))
    su = tj.setups.__wrapped__(cases)['grid']
    x0 = rc.start(su, tj._start(su, 8))
    for form in rc.FORMS:
        for k in rc.SYNC:
            put('%s/sync%d' % (form, k), rc.run(form, su, x0, k), rc.keys(form))
    big, xb = rc.big_setup(cases, su)
    for k in (1, 4):
        put('big/sync%d' % k, rc.run('bfgs', big, xb, k), rc.keys('bfgs'))


def nn_case():
    """rvs_bfgs_run_grad_fused_nn as test_nn_vjp_gpu.py runs it"""
    import torch
    import test_nn_vjp_gpu as tv
    from rvspecfit_amd import bfgs, optimizer, vel_fit
    if not os.path.exists(os.path.join(REPO, 'tests', 'golden', 'nn_case.npz')):
        SKIPPED['nn_fused'] = 'tests/golden/nn_case.npz is not there'
        return
    nets = tv.nets.__wrapped__()
    su = tv.chain.__wrapped__(nets, tv.libs.__wrapped__(nets))
    n = 2
    x0 = np.column_stack([tv.VEL[:n], [300.0] * n, su['par'][:n]])
    x0[:, 0] += 4.0
    xt = torch.as_tensor(x0).to(su['lib'].device)
    for k in (1, 4, 9):
        pobj, names = tv._objective(su, n, su['both'])
        chain = optimizer.GradChain(pobj, cap=1, fused=True)
        assert chain.fused_nn
        r = bfgs.minimize_lockstep_device(
            pobj, xt, hess_inv0=vel_fit.get_hess_inv(['vel', 'vsini'] + names), jac=True,
            chain=chain, sync_every=k)
        keys = ('x', 'fun', 'nit', 'nfev', 'njev', 'status')
        put('nn_fused/sync%d' % k, dict(r, **{q: r[q].cpu().numpy() for q in keys}), keys)


def compare(a, b, out):
    A, B = np.load(a), np.load(b)
    keys = sorted(k for k in A.files if not k.startswith('meta/'))
    assert keys == sorted(k for k in B.files if not k.startswith('meta/')), 'other arrays'
    stats = [k for k in keys if k.endswith('/stats')]
    arrays = [k for k in keys if not k.endswith('/stats')]
    differ = lambda ks: [k for k in ks if A[k].shape != B[k].shape or  # noqa: E731
                         A[k].tobytes() != B[k].tobytes()]
    da, ds = differ(arrays), differ(stats)
    rec = dict(arrays=len(arrays), arrays_differ=len(da), differing=da[:20],
               runs=len(stats), statistics_differ=len(ds), differing_statistics=ds[:20],
               statistics={k[:-len('/stats')]: [int(v) for v in A[k]] for k in stats},
               skipped={n: json.loads(str(X['meta/skipped'])) for n, X in
                        (('a', A), ('b', B))})
    json.dump(rec, open(out, 'w'), indent=1, sort_keys=True)
    print(json.dumps(rec, sort_keys=True))
    return 1 if da or ds else 0


def main():
    if sys.argv[1] == '--compare':
        sys.exit(compare(*sys.argv[2:5]))
    from rvspecfit_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    _lib.require_gpu()
    with np.errstate(all='ignore'):
        driver_cases()
        nn_case()
    OUT['meta/skipped'] = np.array(json.dumps(SKIPPED))
    np.savez(sys.argv[2], **OUT)
    print('%d arrays, skipped: %s' % (len(OUT) - 1, SKIPPED))


if __name__ == '__main__':
    main()
