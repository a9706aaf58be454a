"""The runs of tests/test_rounds_driver_gpu.py and tools/perf/rounds_driver_bits.py: the
five entry points that go through the round driver of csrc/rounds_dev.h, on the set-ups
of tests/test_bfgs_jac_gpu.py, and the batch whose first rounds are above the driver's
one-look-per-round threshold."""
import numpy as np
import torch

from conftest import gold_specdata
from test_bfgs_jac_gpu import _objective, _x0

S, CAP = 5, 3            # 5 runs in chunks of 3 rows: two chunks per round
SYNC = (1, 4, 9)
S_BIG = 640              # 640 runs x (n + 1 = 7) rows = 4480 > 4096 in the first rounds
BFGS_KEYS = ('x', 'fun', 'nit', 'nfev', 'status')
LM_KEYS = ('x', 'fun', 'grad', 'hess', 'mu', 'nit', 'nfev', 'status')
STATS = ('rounds', 'calls', 'rows_launched')
# form: (entry point, GradChain keywords -- None: the value-only form, no chain)
FORMS = dict(bfgs=('rvs_bfgs_run', None),
             bfgs_grad=('rvs_bfgs_run_grad', dict()),
             bfgs_grad_fused=('rvs_bfgs_run_grad_fused', dict(fused=True)),
             lm=('rvs_lm_run', dict(fisher=True)),
             lm_fused=('rvs_lm_run_fused', dict(fused_fisher=True)))


def keys(form):
    if form.startswith('lm'):
        return LM_KEYS
    return BFGS_KEYS + (('njev', ) if form != 'bfgs' else ())


def start(su, nm_optimum, S=S):
    """x0 [S, 6]: the simplex optimum of the first S spectra"""
    return _x0(nm_optimum, su['names'], S, ['vel', 'vsini'] + su['names'])


def run(form, su, x0, sync_every):
    """one call of the form's entry point on an objective of its own: the result arrays
    (numpy) and the three statistics"""
    from rvspecfit_amd import bfgs, lm, optimizer, vel_fit
    n_runs = x0.shape[0]
    pobj, _ = _objective(su, n_runs)
    kw = FORMS[form][1]
    chain = None if kw is None else optimizer.GradChain(pobj, cap=CAP, **kw)
    if form.startswith('lm'):
        r = lm.minimize_lockstep_device(pobj, x0, sync_every=sync_every, chain=chain)
    else:
        H0 = vel_fit.get_hess_inv(['vel', 'vsini'] + su['names'])
        r = bfgs.minimize_lockstep_device(pobj, x0, hess_inv0=H0, sync_every=sync_every,
                                          jac=chain is not None, chain=chain)
    out = {k: r[k].cpu().numpy() for k in keys(form)}
    out.update({k: int(r[k]) for k in STATS})
    return out


def big_setup(cases, su, S=S_BIG):
    """the batch of test_gpu_parity.py::test_process_bfgs_device_equals_host (S copies of
    the golden spectra c1 / c3 under seeded noise, seeded starting parameters) as a set-up
    of `_objective`, and x0 [S, 6]: its simplex optimum"""
    from rvspecfit_amd import spec_fit, vel_fit
    from rvspecfit_amd.engine import SpecBatch
    rng = np.random.RandomState(16)
    lists = [gold_specdata(cases, ('c1', 'c3')[i % 2], spec_fit.SpecData)
             for i in range(S)]
    batch = SpecBatch.from_specdata(lists)
    for a in batch.arms:
        a.spec.mul_(torch.as_tensor(
            1 + 0.02 * rng.normal(size=tuple(a.spec.shape))).to(a.spec.device))
    pd0 = dict(teff=rng.uniform(5000, 6800, S), logg=rng.uniform(1.5, 4.5, S),
               feh=rng.uniform(-1.5, -0.1, S), alpha=rng.uniform(0, 0.4, S),
               vsini=rng.uniform(1, 60, S))
    r = vel_fit.process(batch, dict(pd0), options=dict(npoly=10), config=dict(su['cfg']))
    big = dict(su, batch=batch, sds=lists)
    return big, start(big, r, S)
