"""The round driver of the device optimisers (csrc/rounds_dev.h: rounds_run) through every
entry point that calls it: rvs_bfgs_run, rvs_bfgs_run_grad, rvs_bfgs_run_grad_fused,
rvs_lm_run and rvs_lm_run_fused, S = 5 runs of n = 6 in two chunks per round, the host
looking at the device counts every 1, 4 and 9 rounds; and the branch that looks every round
while a round holds more than 4096 rows, on 640 runs of the value-only form.

Every assertion is exact: a run's path does not depend on when the host looks, the host
only bounds the launches and sees the end.  Below 4096 rows it looks every sync_every
rounds, so it leaves the loop at the first multiple of sync_every at or after the round in
which the last run ended -- R1, what a look every round counts."""
import numpy as np
import pytest

import rounds_driver_cases as rc
from test_bfgs_jac_gpu import nm_optimum, setups   # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('form', list(rc.FORMS))
def test_results_do_not_depend_on_the_look(setups, nm_optimum, form):   # noqa: F811
    su = setups['grid']
    x0 = rc.start(su, nm_optimum)
    assert x0.shape == (rc.S, 6)
    out = {k: rc.run(form, su, x0, k) for k in rc.SYNC}
    for k in rc.SYNC:
        print(form, 'sync_every', k, {s: out[k][s] for s in rc.STATS}, 'nit',
              out[k]['nit'], 'nfev', out[k]['nfev'], 'status', out[k]['status'])
    one = out[1]
    R1 = one['rounds']
    assert R1 >= 2 and (one['nit'] >= 1).any()
    if form == 'bfgs':
        # the row capacity (S rows) splits the first round's S (n + 1) rows
        assert one['calls'] >= 7
    else:
        # cap = 3: two chunks while more than three runs are live
        assert one['calls'] >= R1 + 1
    for k in rc.SYNC[1:]:
        for key in rc.keys(form):
            assert np.array_equal(out[k][key], one[key], equal_nan=True), (k, key)
        assert out[k]['rounds'] == -(-R1 // k) * k, (k, out[k]['rounds'], R1)
    assert one['rows_launched'] <= out[4]['rows_launched'] <= out[9]['rows_launched']


def test_one_look_per_round_above_4096_rows(cases, setups):   # noqa: F811
    """640 runs of the value-only form: the first rounds hold 640 x 7 = 4480 rows, and
    the driver looks after each of them whatever sync_every says"""
    big, x0 = rc.big_setup(cases, setups['grid'])
    assert x0.shape == (rc.S_BIG, 6)
    one, four = rc.run('bfgs', big, x0, 1), rc.run('bfgs', big, x0, 4)
    for r in (one, four):
        print({s: r[s] for s in rc.STATS}, 'nfev', r['nfev'].min(), r['nfev'].max())
    # (the first round alone: every run asks for its value and n differences)
    assert one['rows_launched'] >= rc.S_BIG * 7 > 4096
    for key in rc.keys('bfgs'):
        assert np.array_equal(four[key], one[key], equal_nan=True), key
    assert one['rounds'] <= four['rounds'] <= one['rounds'] + 3
