"""The velocity-grid kernel on the node table (rvs_chisq_grid_tab): jobs that
share a few templates, one velocity grid and one wavelength grid stream the
resampled template of their (node, velocity block) from a table that
chisq_resample_kernel fills once per arm and call, instead of evaluating the
spline per job.  The table holds the numbers the spline evaluation gives and the
sums receive them in the same order, so chi^2 and status are those of the
kernels the other tests tie to the oracle, bit for bit: every comparison here is
exact, except the one against the oracle itself."""
import contextlib
import ctypes
import threading

import numpy as np
import pytest
import torch

from conftest import GOLD_CONFIG
from oracle import rvs_oracle as orc
from test_gpu_parity import _sds, _linear_grid_config, rel, CHI_RTOL
from test_gpu_parity import gpu, config  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


class _Setup:
    """7 perturbed copies of golden case c1, one parameter list with a template
    outside the grid (a penalty), the list's templates built once"""

    def __init__(self, cases, cfg, rot=None, sds=None, S=7):
        from rvspecfit_amd import spec_fit, spec_inter, engine
        from rvspecfit_amd.engine import SpecBatch
        lists = [list(sds) if sds is not None else _sds(cases, 'c1')
                 for _ in range(S)]
        self.batch = SpecBatch.from_specdata(lists)
        rng = np.random.RandomState(3)
        for a in self.batch.arms:   # make the spectra differ
            a.spec.mul_(torch.as_tensor(
                1 + 0.05 * rng.normal(size=tuple(a.spec.shape))).to(a.spec.device))
        self.pl = [tuple(_) for _ in cases['c1/g3/params_list']] + \
            [(3400., 2., -1., 0.2)]
        self.T = len(self.pl)
        self.S = S
        dev = self.batch.device
        self.libs = spec_inter.get_libs(self.batch.names, cfg)
        flat = torch.as_tensor(np.array(self.pl)).to(dev).contiguous()
        vs = None if rot is None else torch.full(
            (self.T, ), float(rot[0]), dtype=torch.float64, device=dev)
        self.coefs, self.outs = [], []
        for arm in self.batch.arms:
            c, o = engine.build_templates(self.libs[arm.name], flat, vs)
            self.coefs.append(c)
            self.outs.append(o)

    def jobs(self, J):
        """J jobs: template 1 unused, the last template (the one outside the
        grid) used by one job only (the third; with J < 3 by none), the jobs of
        a template never adjacent; spectra cycle"""
        used = [t for t in range(self.T - 1) if t != 1]
        jt = [used[j % len(used)] for j in range(J)]
        if J >= 3:
            jt[2] = self.T - 1
        js = [(3 * j) % self.S for j in range(J)]
        dev = self.batch.device
        return (torch.as_tensor(js, dtype=torch.int32).to(dev),
                torch.as_tensor(jt, dtype=torch.int32).to(dev))

    def grid_now(self, J, vg, npoly, outs=None):
        """chi^2 [J, Nv], status [J], how many arms the table served, with the
        engine's knobs as they stand"""
        from rvspecfit_amd import engine
        js, jt = self.jobs(J)
        chisq, st = engine.chisq_grid(
            self.batch, self.libs, self.coefs, outs or self.outs,
            torch.as_tensor(np.ascontiguousarray(vg)).to(self.batch.device),
            npoly=npoly, job_spec=js, job_templ=jt)
        return chisq.cpu().numpy(), st.cpu().numpy(), engine.cg_tab_took()

    def grid(self, J, vg, npoly, tab, outs=None, pack=1):
        """the same with the table path forced (tab) or off"""
        with _knobs(tab, pack):
            return self.grid_now(J, vg, npoly, outs)

    def same(self, J, vg, npoly, served=True, **kw):
        """table path against the path off; `served`: the table must have served
        every arm (else: none)"""
        a, sa, took = self.grid(J, vg, npoly, True, **kw)
        b, sb, took0 = self.grid(J, vg, npoly, False, **kw)
        assert took0 == 0
        assert took == (len(self.batch.arms) if served else 0), took
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(sa, sb)
        return a, sa


@contextlib.contextmanager
def _knobs(tab, pack=1):
    """engine.CG_TAB_MIN_JOBS forced (1) or off (-1), CG_PACK_MIN_JOBS = pack;
    module globals: set from one thread at a time"""
    from rvspecfit_amd import engine
    keep = engine.CG_TAB_MIN_JOBS, engine.CG_PACK_MIN_JOBS
    engine.CG_TAB_MIN_JOBS = 1 if tab else -1
    engine.CG_PACK_MIN_JOBS = pack
    try:
        yield
    finally:
        engine.CG_TAB_MIN_JOBS, engine.CG_PACK_MIN_JOBS = keep


_setups = {}


def _setup(cases, config, rot=None):
    if rot not in _setups:
        _setups[rot] = _Setup(cases, config, rot)
    return _setups[rot]


@pytest.mark.parametrize('nv', [400, 64, 69, 128, 40])
def test_node_table_velocity_grids(cases, config, nv):
    """400 velocities: 6 full waves on the table + 16 packed; 64 and 128: full
    waves only; 69: one full wave + 5 left over; 40: no full wave -- the path
    declines and the old kernels give the old result.  21 jobs (not a multiple
    of 8), a penalty in one of them (template outside the grid)."""
    su = _setup(cases, config)
    vg = cases['vel_grid'].astype(np.float64)
    assert len(vg) == 400
    chisq, st = su.same(21, vg[:nv], 10, served=nv >= 64)
    assert np.all(np.isfinite(chisq))
    # the job on the template outside the grid carries a penalty
    assert all(float(o[su.T - 1].item()) > 0 for o in su.outs)
    if nv == 69:   # the left-over velocities as a ragged wave of the old kernel
        r, _, _ = su.grid(21, vg[:nv], 10, False, pack=-1)
        np.testing.assert_array_equal(chisq, r)
        # "never pack": the table serves whole blocks only and declines
        su.same(21, vg[:nv], 10, served=False, pack=-1)


def test_node_table_declines_ragged_left_overs(cases, config):
    """125 velocities leave 61 over, more than the old launch packs: it keeps a
    ragged wave for them, and the table is not taken"""
    su = _setup(cases, config)
    vg = cases['vel_grid'].astype(np.float64)
    su.same(21, vg[:125], 10, served=False)


@pytest.mark.parametrize('npoly', [1, 7, 13, 15])
def test_node_table_npoly(cases, config, npoly):
    """other basis sizes (10 is the test above); 15 runs the pixel loop twice
    and reads the stream in both passes"""
    su = _setup(cases, config)
    vg = cases['vel_grid'].astype(np.float64)
    su.same(11, vg[:133], npoly)


@pytest.mark.parametrize('J', [1, 3, 8, 29])
def test_node_table_job_counts(cases, config, J):
    """J = 1 and J = 3 with 2 blocks of velocities: Q = 2 and 6 work items, fewer
    than the 8 ranges the list is cut into (some are empty); 8: every range one
    job's worth; 29: ranges that end inside a node"""
    su = _setup(cases, config)
    vg = cases['vel_grid'].astype(np.float64)
    su.same(J, vg[:128 + 7], 10)


@pytest.mark.parametrize('npix', [2, 3, 5, 8])
def test_node_table_short_arms(cases, config, npix):
    """arms shorter than, as long as and longer than the 4 pixels the table
    values are requested ahead"""
    from rvspecfit_amd import spec_fit
    sd0 = _sds(cases, 'c1')[0]
    i0 = len(sd0.lam) // 3
    sds = [spec_fit.SpecData(sd0.name, sd0.lam[i0:i0 + npix].copy(),
                             sd0.spec[i0:i0 + npix].copy(),
                             sd0.espec[i0:i0 + npix].copy())]
    su = _Setup(cases, config, sds=sds, S=3)
    su.same(5, np.linspace(-310.0, 295.0, 70), 1)


def test_node_table_linear_template_grid(cases, config):
    """a template library on LINEAR knots: the other instance of the resampling"""
    cfg, _ = _linear_grid_config()
    sd = [x for x in _sds(cases, 'c1') if x.name == 'gold_b'][:1]
    su = _Setup(cases, cfg, sds=sd, S=3)
    chisq, st = su.same(7, np.linspace(-310.0, 295.0, 70), 10)
    assert np.all(np.isfinite(chisq))


def test_node_table_unusable_template(cases, config):
    """a node whose outside flag is not finite: its waves leave before the loop"""
    su = _setup(cases, config)
    outs = [o.clone() for o in su.outs]
    outs[0][2] = float('inf')
    vg = cases['vel_grid'].astype(np.float64)
    chisq, st = su.same(13, vg[:133], 10, outs=outs)
    js, jt = su.jobs(13)
    hit = (jt == 2).cpu().numpy()
    assert hit.sum() >= 2 and np.all(np.isfinite(chisq))


def test_node_table_rotation(cases, config):
    """templates broadened by rotation (30 km/s)"""
    su = _setup(cases, config, rot=(30., ))
    vg = cases['vel_grid'].astype(np.float64)
    su.same(10, vg[:133], 10)


def test_node_table_two_host_threads(cases, config):
    """two host threads, each on a torch stream of its own, at the same time:
    each call owns its table, and each thread sees that the table served it"""
    su = _setup(cases, config)
    vg = cases['vel_grid'].astype(np.float64)
    want = {k: su.grid(21, vg + 0.37 * k, 10, False)[0] for k in range(2)}
    got, took, errs = {}, {}, []

    def run(k):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                for _ in range(3):
                    got[k], _, t = su.grid_now(21, vg + 0.37 * k, 10)
                    took.setdefault(k, []).append(t)
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=run, args=(k, )) for k in range(2)]
    with _knobs(True):     # (set once, around the threads)
        for t in th:
            t.start()
        for t in th:
            t.join()
    assert not errs, errs
    for k in range(2):
        assert took[k] == [len(su.batch.arms)] * 3, took
        np.testing.assert_array_equal(got[k], want[k])


def test_node_table_find_best_vs_oracle(cases, config, gold_config, gold_libs):
    """find_best over one parameter list with the table forced on, against the
    oracle's chi^2 grid at the tolerance the grid tests hold"""
    from rvspecfit_amd import spec_fit, engine
    su = _setup(cases, config)
    vg = cases['vel_grid'].astype(np.float64)
    with _knobs(True, pack=0):
        a = spec_fit.find_best(su.batch, vg, su.pl, options=dict(npoly=10),
                               config=config)
        took = engine.cg_tab_took()
    assert took == len(su.batch.arms)
    chisq = a['chisq'].cpu().numpy().reshape(su.S, su.T, len(vg))
    sds = _sds(cases, 'c1')
    for s in (0, 4):
        osds = [orc.SpecData(sd.name, sd.lam, arm.spec[s].cpu().numpy(), sd.espec,
                             badmask=sd.badmask)
                for sd, arm in zip(sds, su.batch.arms)]
        for t in (0, 2):
            fast = orc.chisq_grid_fast(osds, vg, su.pl[t], None, dict(npoly=10),
                                       gold_config, gold_libs)
            assert rel(chisq[s, t], fast) < CHI_RTOL, (s, t)


def _raw_call(su, vg, table, entry='tab', rows=None, no_templ=False,
              per_job_vels=False, grid_id=False, tab_state=0, **over):
    """rvs_chisq_grid_tab (or, entry 'g', rvs_chisq_grid_g) for the first arm of
    `su` with the arguments engine.chisq_grid gives it (11 jobs, npoly 10), some
    of them replaced.  rows = (a, b): only jobs a..b-1 of the 11, as one chunk
    of a longer call (call_start / J_call stay the whole list's); no_templ:
    job_templ NULL (job j on template j, as many jobs as templates);
    per_job_vels: vels [J, Nv], vel_stride Nv; grid_id: a grid index per
    spectrum beside G = 1.  -> chi^2 [J, Nv], took"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    dev = su.batch.device
    arm, coef = su.batch.arms[0], su.coefs[0]
    lib = su.libs[arm.name]
    js, jt = su.jobs(11)
    if no_templ:
        js = js[:su.T].contiguous()
        jt = torch.arange(su.T, dtype=torch.int32, device=dev)
    Jc, Nv, npoly = int(jt.shape[0]), len(vg), 10
    nodes = torch.arange(su.T + 1, dtype=torch.int32, device=dev)

    def by_node(t):
        srt, order = torch.sort(t, stable=True)
        return (order.to(torch.int32).contiguous(),
                torch.searchsorted(srt, nodes, out_int32=True).contiguous())
    call_start = by_node(jt)[1]
    if rows is not None:
        js, jt = js[rows[0]:rows[1]].contiguous(), jt[rows[0]:rows[1]].contiguous()
    J = int(jt.shape[0])
    order, start = by_node(jt)
    work = arm.work(lib, 0.0)
    polysT, logdet_off = arm.basis_ortho(npoly, True)
    pen = (su.outs[0][jt.long()] * su.batch.badchi_jobs(js) + logdet_off
           ).contiguous()
    vels = torch.as_tensor(np.ascontiguousarray(vg)).to(dev)
    if per_job_vels:
        vels = vels[None].expand(J, Nv).contiguous()
    out = torch.zeros((J, Nv), dtype=torch.float64, device=dev)
    status = torch.zeros(J, dtype=torch.int32, device=dev)
    took = ctypes.c_int32(-1)
    gid, G = arm.grid_args()
    assert gid is None and G == 1
    gids = torch.zeros(arm.S, dtype=torch.int32, device=dev)
    a = dict(order=_lib.ptr(order), start=_lib.ptr(start),
             call_start=_lib.ptr(call_start), J_call=Jc, min_jobs=1,
             tab=_lib.ptr(table), tab_size=table.numel(), pack=1)
    a.update(over)
    if a['start'] is None:
        a['call_start'] = None
    args = [_lib.ptr(arm.lam), _lib.ptr(polysT), _lib.ptr(work), arm.npix, npoly,
            arm.S, _lib.ptr(gids) if grid_id else None, G,
            arm.basis_stride(npoly), _lib.ptr(lib.knots), _lib.ptr(coef), lib.ntp,
            coef.shape[0], int(lib.log_step), _lib.ptr(js),
            None if no_templ else _lib.ptr(jt), J, _lib.ptr(vels),
            Nv if per_job_vels else 0, Nv, _lib.ptr(pen), float(su.batch.badchi),
            0.0, a['pack'], _lib.ptr(su.batch.pen_scale), _lib.ptr(out),
            _lib.ptr(status)]
    if entry == 'g':
        rc = L.rvs_chisq_grid_g(*args, _lib.stream())
    else:
        rc = L.rvs_chisq_grid_tab(
            *args, a['order'], a['start'], a['call_start'], a['J_call'],
            a['min_jobs'], a['tab'], a['tab_size'], tab_state,
            ctypes.byref(took), _lib.stream())
    _lib.check(rc, 'rvs_chisq_grid_' + entry)
    torch.cuda.synchronize()
    return out.cpu().numpy(), took.value


PAT = -7.25


def _table(su, vg, J=11):
    from rvspecfit_amd import _lib
    arm = su.batch.arms[0]
    n = _lib.lib().rvs_chisq_grid_tab_work_size(arm.npix, su.T, len(vg), J, 1, 1)
    assert n == su.T * (len(vg) // 64) * arm.npix * 64
    return torch.full((n, ), PAT, dtype=torch.float64, device=su.batch.device)


def test_node_table_gate_declines_and_leaves_the_table_alone(cases, config):
    """option "cg_tab" off, or any condition of the gate false: the call is
    rvs_chisq_grid_g -- its result, took = 0, and the table buffer keeps the
    pattern it was filled with"""
    from rvspecfit_amd import _lib
    L = _lib.lib()
    su = _setup(cases, config)
    vg = cases['vel_grid'].astype(np.float64)[:133]
    arm = su.batch.arms[0]
    size = lambda *a: L.rvs_chisq_grid_tab_work_size(*a)  # noqa: E731
    table = _table(su, vg)
    n = table.numel()
    assert size(arm.npix, su.T, 63, 11, 1, 1) == 0
    assert size(arm.npix, su.T, len(vg), 11, -1, 1) == 0
    assert size(arm.npix, su.T, len(vg), 11, 3, 1) == 0
    assert size(arm.npix, su.T, len(vg), 3 * su.T, 3, 1) == n
    assert size(arm.npix, su.T, len(vg), 11, 1, -1) == 0     # 5 left over, never packed
    assert size(arm.npix, su.T, 128, 11, 1, -1) > 0          # none left over
    assert size(arm.npix, su.T, 125, 11, 1, 1) == 0          # 61 left over
    # (over the byte cap of 1 GiB: no buffer of that size is made for a call)
    assert size(1 << 20, 64, 128, 1 << 20, 1, 1) == 0
    want, took = _raw_call(su, vg, table)
    assert took == 1
    np.testing.assert_array_equal(want, _raw_call(su, vg, table, entry='g')[0])
    filled = table.cpu().numpy().reshape(su.T, -1)
    used = set(su.jobs(11)[1].tolist())
    assert 1 not in used and len(used) >= 3
    for t in range(su.T):   # an unused template is not resampled
        assert np.all(filled[t] == PAT) if t not in used else \
            np.all(filled[t] != PAT), t
    # every condition of the gate, one at a time, against rvs_chisq_grid_g
    # called with the same arguments
    declines = [dict(min_jobs=-1), dict(min_jobs=2 * su.T), dict(J_call=5),
                dict(tab_size=n - 1), dict(tab=None), dict(order=None),
                dict(start=None), dict(pack=-1), dict(no_templ=True),
                dict(per_job_vels=True), dict(grid_id=True), 'option']
    for d in declines:
        table.fill_(PAT)
        if d == 'option':
            assert L.rvs_option_set(b'cg_tab', 0) == 0
            try:
                assert size(arm.npix, su.T, len(vg), 11, 1, 1) == 0
                got, took = _raw_call(su, vg, table)
            finally:
                assert L.rvs_option_set(b'cg_tab', 1) == 0
            ref = want
        else:
            got, took = _raw_call(su, vg, table, **d)
            how = {k: v for k, v in d.items()
                   if k in ('no_templ', 'per_job_vels', 'grid_id', 'pack')}
            ref = _raw_call(su, vg, table, entry='g', **how)[0]
        assert took == 0, d
        np.testing.assert_array_equal(got, ref, err_msg=str(d))
        assert bool((table == PAT).all().item()), d
    # (a grid of 125 velocities: 61 left over, which stay a ragged wave)
    table = _table(su, cases['vel_grid'][:128].astype(np.float64))
    v125 = cases['vel_grid'].astype(np.float64)[:125]
    got, took = _raw_call(su, v125, table)
    assert took == 0 and bool((table == PAT).all().item())
    np.testing.assert_array_equal(got, _raw_call(su, v125, table, entry='g')[0])
    # the engine does not ask for a table where the call cannot use one:
    # per-job velocity grids
    from rvspecfit_amd import engine
    with _knobs(True):
        js, jt = su.jobs(11)
        vv = torch.as_tensor(np.tile(vg, (11, 1))).to(su.batch.device)
        c, _ = engine.chisq_grid(su.batch, su.libs, su.coefs, su.outs, vv,
                                 npoly=10, job_spec=js, job_templ=jt)
        assert engine.cg_tab_took() == 0
    ref, _, _ = su.grid(11, vg, 10, False)
    np.testing.assert_array_equal(c.cpu().numpy(), ref)


def test_node_table_one_table_for_the_chunks_of_a_call(cases, config):
    """a job list fed in two calls that share one table (engine.chisq_grid cuts
    lists of more than 65 535 jobs): the first call fills the table from the
    WHOLE list's counts -- a template only the second chunk uses included --,
    the second (tab_state 1) reads it and resamples nothing"""
    su = _setup(cases, config)
    vg = cases['vel_grid'].astype(np.float64)[:133]
    jt = su.jobs(11)[1].tolist()
    last = su.T - 1
    assert last not in jt[:2] and last in jt[2:]
    ref = _raw_call(su, vg, _table(su, vg), entry='g')[0]
    table = _table(su, vg)
    a, took = _raw_call(su, vg, table, rows=(0, 2))
    assert took == 1
    filled = table.cpu().numpy().reshape(su.T, -1)
    assert np.all(filled[last] != PAT) and np.all(filled[1] == PAT)
    before = table.clone()
    b, took = _raw_call(su, vg, table, rows=(2, 11), tab_state=1)
    assert took == 1
    assert torch.equal(table, before)      # the second call wrote nothing to it
    np.testing.assert_array_equal(np.concatenate([a, b]), ref)
