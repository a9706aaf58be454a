"""Device-resident optimiser stage of vel_fit.process.

`DeviceNelderMead` drives the rvs_nm_* kernels (csrc/nm.hip): the S simplices
and all their bookkeeping live in HBM, a round is a fixed sequence of launches
whose job counts are read on the device, and the host only looks at the counts
every `sync_every` rounds (to shrink its launch bound, to run parked shrinks and
to notice that everything has converged).  `ProcessObjective` is chisq_func of
vel_fit.py:229-254 as a fixed launch sequence on preallocated buffers:
rvs_proc_map -> per arm rvs_template_polylinear, rvs_vsini_convolve,
rvs_spline_construct -> rvs_chisq_point (all arms) -> rvs_proc_finish (the 'chain'
form of engine.objective_form; in the 'fused' and 'from_template' forms one
objective kernel stands between the map and the finish).

tests/refmachines/neldermead_torch.py is the same state machine in torch: the CPU
suite pins it to scipy (identical nit, nfev, final simplex), the GPU suite pins
these kernels to it bit for bit.  Its ~70 small torch calls and three host
synchronisations per round cost more than the GPU work, hence the kernels.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import engine


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class ProcessObjective:
    """chisq_func for rows (list[j], X[j]) on preallocated buffers."""

    def __init__(self, batch, libs, names, pd0, fixParam, fitVsini, config,
                 options, priors, safe_params, resols=None):
        L = _lib.lib()
        self.L = L
        self.batch, self.libs = batch, libs
        dev = batch.device
        S = batch.S
        self.S, self.dev = S, dev
        self.npoly = options.get('npoly') or 5
        self.rbf = options.get('rbf_continuum', True)
        self.resols = resols
        self.ndim = len(names)
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        # parameter vector layout (vel, [vsini], free stellar parameters)
        k = 1
        self.vsini_col = -1
        self.has_vsini = 'vsini' in pd0
        if fitVsini:
            self.vsini_col = k
            k += 1
        src = []
        for x in names:
            if x in fixParam:
                src.append(-1)
            else:
                src.append(k)
                k += 1
        self.n = k
        self.src = (ctypes.c_int32 * self.ndim)(*src)
        self.fixed = torch.stack([pd0[_] for _ in names], dim=1).contiguous()
        self.vsini_fixed = pd0['vsini'].contiguous() if (
            self.has_vsini and not fitVsini) else None
        self.safe = safe_params.contiguous()
        self.prior_mean = self.prior_isig = None
        if priors:
            pm = torch.zeros((S, self.ndim), **f64)
            ps = torch.zeros((S, self.ndim), **f64)
            for i, x in enumerate(names):
                if x in priors:
                    m, sg = priors[x]
                    pm[:, i] = torch.as_tensor(m, **f64)
                    ps[:, i] = 1.0 / torch.as_tensor(sg, **f64)
            self.prior_mean, self.prior_isig = pm, ps
        self.min_vel, self.max_vel = float(config['min_vel']), float(
            config['max_vel'])
        self.max_vsini = float(config['max_vsini'])
        # (MLP libraries in the gradient chain are opt-in: engine.check_grad_scope)
        self.nn_gradient = bool(config.get('nn_gradient'))
        # (Delaunay libraries in the fused gradient too: engine.check_fused_grad_scope)
        self.tri_gradient = bool(config.get('tri_gradient'))
        # (and so are resolution matrices)
        self.resol_gradient = bool(config.get('resol_gradient'))
        cap = S
        self.cap = cap
        self.job_spec = torch.zeros(cap, **i32)
        self.vel = torch.zeros(cap, **f64)
        self.vsini = torch.zeros(cap, **f64) if self.has_vsini else None
        self.params = torch.zeros((cap, self.ndim), **f64)
        self.extra = torch.zeros(cap, **f64)
        self.bad = torch.zeros(cap, **i32)
        self.chi = torch.zeros(cap, **f64)
        self.jstatus = torch.zeros(cap, **i32)
        self.status = torch.zeros(S, **i32)
        self.badchi = float(batch.badchi)
        # (which form the objective takes decides which row buffers exist: the one-kernel
        # objective keeps no template or spline record in HBM, the from-template form
        # only the evaluator's rows -- 0.6 GB per 1000 rows less to allocate for the
        # sub-batches of vel_fit.process: its halves, the spectra of a second run)
        self.form = engine.objective_form(batch, libs, resols, self.npoly)
        # the optimisers' rounds can run inside the library (rvs_nm_run, rvs_bfgs_run)
        self.native = engine.rounds_in_library(batch, libs, self.form)
        chain = self.form == 'chain'
        narm = len(batch.arms)
        self.arm_buf = []
        for arm in batch.arms:
            lib = libs[arm.name]
            self.arm_buf.append(dict(
                templ=None if self.form == 'fused' else
                torch.empty((cap, lib.ntp), **f64),
                templ2=torch.empty((cap, lib.ntp), **f64)
                if (self.has_vsini and chain) else None,
                coef=torch.empty((cap, lib.ntp, 4), **f64) if chain else None,
                pen=torch.empty(cap, **f64) if chain else None,
                outside=torch.empty(cap, **f64),
                sx=torch.empty(cap, **i32),
                nn=None if lib.kind != 'nn' else dict(
                    a0=torch.empty((cap, lib.nn_width()),
                                   dtype=torch.float32, device=dev),
                    a1=torch.empty((cap, lib.nn_width()),
                                   dtype=torch.float32, device=dev))))
        if chain:
            # rvs_chisq_point reads the spline records and penalties of a round
            self.arr = (_lib.PointArm * narm)()
            self._keep = [engine.fill_point_arm(
                self.arr[ia], arm, libs[arm.name], self.npoly, self.rbf, 0.0,
                engine._arm_resol(arm, ia, resols), b['coef'], b['pen'])
                for ia, (arm, b) in enumerate(zip(batch.arms, self.arm_buf))]
            nb = L.rvs_chisq_point_work_size(cap, narm)
        else:
            self.oarr = (_lib.ObjectiveArm * narm)()
            self._keep = engine.fill_objective_arms(self.oarr, batch, libs,
                                                    self.npoly, self.rbf, 0.0,
                                                    resols)
            nb = L.rvs_objective_work_size(cap, narm)
        self.scratch = torch.empty((nb + 7) // 8, **f64)
        # the evaluators whose rows of a round the library builds itself (from-template
        # form, rounds in the library): MLP or Delaunay libraries on every arm
        self.nn_arr = self.tri_arr = None
        if self.native and self.form == 'from_template':
            if libs[batch.arms[0].name].kind == 'nn':
                self.nn_arr = self._nn_arms()
            else:
                self.tri_arr = self._tri_arms()
        self.streams = [torch.cuda.Stream(device=dev) for _ in batch.arms]
        self.ev_in = torch.cuda.Event()
        self.ev_out = [torch.cuda.Event() for _ in batch.arms]
        self.calls = 0    # objective calls,
        self.jobs = 0     # function values computed
        self.slots = 0    # and rows launched by the rounds inside the library

    def _nn_arms(self):
        """rvs_nm_nn_arm descriptors: the MLP of every arm and its row buffers"""
        arr = (_lib.NmNNArm * len(self.arm_buf))()
        self._nn_keep = []
        for ia, (arm, b) in enumerate(zip(self.batch.arms, self.arm_buf)):
            lib = self.libs[arm.name]
            a = arr[ia]
            nl = len(lib.nn_W)
            Wp = (ctypes.c_void_p * nl)(*[w.data_ptr() for w in lib.nn_W])
            bp = (ctypes.c_void_p * nl)(*[x.data_ptr() for x in lib.nn_b])
            self._nn_keep += [Wp, bp]
            a.M, a.S = lib.nn_M.data_ptr(), lib.nn_S.data_ptr()
            a.W = ctypes.cast(Wp, ctypes.c_void_p)
            a.b = ctypes.cast(bp, ctypes.c_void_p)
            a.dims = lib.nn_dims.ctypes.data
            a.act0 = b['nn']['a0'].data_ptr()
            a.act1 = b['nn']['a1'].data_ptr()
            a.templ, a.outside = b['templ'].data_ptr(), b['outside'].data_ptr()
            hull = lib.hull_device()
            if hull is None:
                a.xeqs = a.yeqs = None
                a.nfx = a.nfy = 0
            else:
                a.xeqs, a.yeqs = hull[0].data_ptr(), hull[1].data_ptr()
                a.nfx, a.nfy = hull[0].shape[0], hull[1].shape[0]
            a.nlayer, a.log_mask = nl, lib.log_mask
        return arr

    def _tri_arms(self):
        """rvs_nm_tri_arm descriptors: the triangulation of every arm and its row
        buffers"""
        arr = (_lib.NmTriArm * len(self.arm_buf))()
        for ia, (arm, b) in enumerate(zip(self.batch.arms, self.arm_buf)):
            lib = self.libs[arm.name]
            a = arr[ia]
            a.dats, a.transform = lib.dats.data_ptr(), lib.tri_transform.data_ptr()
            a.extraflags = lib.tri_extraflags.data_ptr()
            a.simplices = lib.tri_simplices.data_ptr()
            a.templ, a.outside = b['templ'].data_ptr(), b['outside'].data_ptr()
            # (arms on ONE triangulation share the simplex ids: rvs_nm_run searches
            # once for all of them)
            first = [k for k in range(ia + 1) if self.libs[
                self.batch.arms[k].name].tri_transform.data_ptr() ==
                lib.tri_transform.data_ptr() and self.libs[
                self.batch.arms[k].name].log_mask == lib.log_mask][0]
            a.simplex = self.arm_buf[first]['sx'].data_ptr()
            a.buckets = lib._tri_bk
            a.ntp, a.nsimplex = lib.ntp, lib.tri_nsimplex
            a.exp_flag, a.log_mask = lib.exp_flag, lib.log_mask
        return arr

    def native_desc(self):
        """rvs_nm_objective: this objective for the C round driver"""
        o = _lib.NmObjective()
        # (the chain form has no one-kernel descriptors: rvs_bfgs_run_grad, which
        # reads the mapping alone, is its only caller there)
        oarr = getattr(self, 'oarr', None)
        o.arms = None if oarr is None else ctypes.addressof(oarr)
        for k, t in (('fixed', self.fixed), ('vsini_fixed', self.vsini_fixed),
                     ('safe', self.safe), ('prior_mean', self.prior_mean),
                     ('prior_isig', self.prior_isig), ('vel', self.vel),
                     ('vsini', self.vsini), ('params', self.params),
                     ('extra', self.extra), ('chi', self.chi),
                     ('job_spec', self.job_spec), ('bad', self.bad),
                     ('jstatus', self.jstatus), ('status', self.status),
                     ('scratch', self.scratch)):
            setattr(o, k, None if t is None else t.data_ptr())
        o.min_vel, o.max_vel = self.min_vel, self.max_vel
        o.max_vsini, o.badchi = self.max_vsini, self.badchi
        o.narm, o.npoly = len(self.arm_buf), self.npoly
        o.n, o.ndim, o.vsini_col = self.n, self.ndim, self.vsini_col
        for i in range(8):
            o.src[i] = self.src[i] if i < self.ndim else -1
        o.nn = None if self.nn_arr is None else ctypes.addressof(self.nn_arr)
        o.tri = None if self.tri_arr is None else ctypes.addressof(self.tri_arr)
        return o

    def eval(self, list_t, X, J, counts, cidx, F):
        """F[:J] = chisq_func(X[j]) for spectrum list_t[j]; rows >= the device
        count counts[cidx] are padding: the one-kernel objective skips them, F there
        is whatever it was."""
        L = self.L
        st = _lib.stream()
        narm = len(self.arm_buf)
        rc = L.rvs_proc_map(J, self.n, self.ndim, _p(X), _p(list_t), self.src,
                            self.vsini_col, _p(self.fixed),
                            _p(self.vsini_fixed), _p(self.safe),
                            _p(self.prior_mean), _p(self.prior_isig),
                            self.min_vel, self.max_vel, self.max_vsini,
                            _p(self.job_spec), _p(self.vel), _p(self.vsini),
                            _p(self.params), _p(self.extra), _p(self.bad), st)
        _lib.check(rc, 'rvs_proc_map')
        live = None if counts is None else counts.data_ptr() + 4 * int(cidx)
        # (the one-kernel forms -- 3 = 1 | RVS_OBJ_STATUS_STORE: outside penalty on,
        # jstatus is overwritten, no clearing launch)
        if self.form == 'fused':   # gather, FIR, spline solve, chi^2
            rc = L.rvs_objective_fused_n(
                ctypes.addressof(self.oarr), narm, self.npoly, _p(self.params),
                _p(self.vsini), _p(self.job_spec), J, live, _p(self.vel),
                self.badchi, 3, _p(self.scratch), _p(self.chi), _p(self.jstatus),
                st)
            _lib.check(rc, 'rvs_objective_fused')
        elif self.form == 'from_template':
            if self.nn_arr is not None:   # one grouped launch chain for all arms
                rc = L.rvs_template_nn_arms_n(
                    _p(self.params), J, live, self.ndim, narm,
                    ctypes.addressof(self.nn_arr), st)
                _lib.check(rc, 'rvs_template_nn_arms')
            else:
                self._rows_per_arm(J)
            tp = (ctypes.c_void_p * narm)(*[b['templ'].data_ptr()
                                            for b in self.arm_buf])
            op = (ctypes.c_void_p * narm)(*[b['outside'].data_ptr()
                                            for b in self.arm_buf])
            rc = L.rvs_objective_from_template_n(
                ctypes.addressof(self.oarr), narm, self.npoly,
                ctypes.cast(tp, ctypes.c_void_p),
                ctypes.cast(op, ctypes.c_void_p), _p(self.vsini),
                _p(self.job_spec), J, live, _p(self.vel), self.badchi, 3,
                _p(self.scratch), _p(self.chi), _p(self.jstatus), st)
            _lib.check(rc, 'rvs_objective_from_template')
        else:
            self._rows_per_arm(J)
            self._chisq_point(J, st)
        rc = L.rvs_proc_finish(J, _p(counts), cidx, _p(self.chi), _p(self.extra),
                               _p(self.bad), _p(self.job_spec), _p(self.jstatus),
                               _p(F), _p(self.status), st)
        _lib.check(rc, 'rvs_proc_finish')
        self.calls += 1
        self.jobs += J

    def _rows_per_arm(self, J):
        """the template rows of every arm from its evaluator and -- chain -- the
        broadening, spline records and penalties behind them: the arms are
        independent until the kernel that sums them, one stream each"""
        L = self.L
        main = torch.cuda.current_stream()
        self.ev_in.record(main)
        for arm, b, side, ev in zip(self.batch.arms, self.arm_buf, self.streams,
                                    self.ev_out):
            lib = self.libs[arm.name]
            side.wait_event(self.ev_in)
            ss = ctypes.c_void_p(side.cuda_stream)
            scr = b['sx']
            if b['nn'] is not None:
                scr = dict(b['nn'], torch_stream=side)
            lib.eval_into(self.params, J, b['templ'], b['outside'], ss,
                          scratch=scr)
            if self.form == 'chain':
                y = b['templ']
                if self.has_vsini:
                    rc = L.rvs_vsini_convolve(_p(y), _p(self.vsini),
                                              _p(b['outside']), lib.lnstep, 0.6,
                                              lib.ntp, J, _p(b['templ2']), ss)
                    _lib.check(rc, 'rvs_vsini_convolve')
                    y = b['templ2']
                rc = L.rvs_spline_construct(_p(lib.knots), _p(y), lib.ntp, J,
                                            lib.spline_form,
                                            _p(lib.spline_factors), _p(b['coef']),
                                            ss)
                _lib.check(rc, 'rvs_spline_construct')
                with torch.cuda.stream(side):
                    torch.mul(b['outside'], self.badchi, out=b['pen'])
                    if self.batch.pen_scale is not None:   # grid sets (SpecBatch)
                        b['pen'][:J] *= self.batch.pen_scale[self.job_spec[:J].long()]
            ev.record(side)
        for ev in self.ev_out:
            main.wait_event(ev)

    def _chisq_point(self, J, st):
        """chain: chi[:J], jstatus[:J] from the arms' spline records"""
        if self.npoly > engine.POINT_MAXP:
            # 17 ... 32 basis functions: beyond the point kernel's 16 per lane, the
            # arms' values come from rvs_chisq_full (engine.chisq_point)
            c, stj = engine.chisq_point(
                self.batch, self.libs, [b['coef'] for b in self.arm_buf],
                [b['outside'][:J] for b in self.arm_buf], self.vel[:J],
                npoly=self.npoly, rbf=self.rbf, job_spec=self.job_spec[:J],
                resols=self.resols)
            self.chi[:J] = c
            self.jstatus[:J] = stj
        else:
            self.jstatus.zero_()
            rc = self.L.rvs_chisq_point(
                ctypes.addressof(self.arr), len(self.arm_buf), self.npoly,
                _p(self.job_spec), None, J, _p(self.vel), self.badchi,
                _p(self.scratch), _p(self.chi), _p(self.jstatus), st)
            _lib.check(rc, 'rvs_chisq_point')


# bytes the row buffers of a GradChain may take (template rows, their tangents and the
# spline records of `cap` rows per arm: 48 (1 + ntan) ntp bytes per row and arm, 2.7 MB
# at ntan = 6 and 8000 template pixels); a round with more rows runs in chunks
GRAD_CHAIN_BUDGET = 4 << 30
# bytes the work rows of GradChain(fused_fisher=True) may take ((3 + ntan) npix doubles
# per row and arm: 0.55 MB per row on the three DESI arms); a chunk with more rows goes
# through rvs_objective_fisher in several launches, with the same bits
FISHER_FUSED_WORK_BUDGET = 512 << 20


class GradChain:
    """chisq_func_grad for the rows of a round: the rvs_grad_chain of
    rvs_bfgs_run_grad around a ProcessObjective (whose mapping tables and row
    buffers it uses), and the same evaluation driven from Python (`rows`).
    fisher=True: the Fisher form of the chain (rvs_lm_run: rvs_chisq_point_fisher and
    rvs_proc_finish_fisher as its last two calls) -- `rows` then returns
    [rows, 1 + n + n (n + 1) / 2] = (f, gradient, lower triangle of the Gauss-Newton
    Hessian), and the Fisher buffers are counted inside the same budget.
    fused=True (config['fused_gradient']): the rows' value and gradient come from ONE
    rvs_objective_grad call per chunk (rvs_bfgs_run_grad_fused; csrc/objective_grad.hip)
    -- the object then holds no template or record buffers, only the arm descriptors,
    the kernel's scratch and the chunk's chi / grad; `rows` goes through the same call.
    On MLP libraries (the objective's nn_gradient set; rvs_bfgs_run_grad_fused_nn, DESIGN
    4.25) it also holds a chunk's adjoint rows [cap, ntp] per arm and the work of the
    networks' reverse pass; on Delaunay libraries (the objective's tri_gradient set;
    rvs_bfgs_run_grad_fused_tri) the adjoint rows and the arms' parameter
    components.  Under resolution matrices (the objective's resol_gradient set; DESIGN
    4.27) the arm descriptors carry the taps and the runs are the _resol forms of the
    three (rvs_bfgs_run_grad_fused_resol, _nn_resol, _tri_resol): still no row buffers.
    What that kernel does not cover, fisher=True included, raises ValueError.
    fused_fisher=True (config['fused_fisher']): the Fisher form with the rows' value,
    gradient and matrix from ONE rvs_objective_fisher call per chunk (rvs_lm_run_fused;
    csrc/objective_fisher.hip) -- no row buffers either: the arm descriptors, the chunk's
    chi / grad and one buffer for the chunk's matrices and the kernel's work rows, at
    most FISHER_FUSED_WORK_BUDGET bytes of the latter (the call goes through a chunk's
    jobs in as many launches as that takes)."""

    def __init__(self, pobj, cap=None, budget=None, fisher=False, fused=False,
                 fused_fisher=False):
        L = _lib.lib()
        batch, libs = pobj.batch, pobj.libs
        fit = pobj.vsini_col >= 0
        self.fused = bool(fused)
        self.fused_fisher = bool(fused_fisher) and not self.fused
        if self.fused:
            self._init_fused(pobj, cap, fisher)
            return
        if self.fused_fisher:
            self._init_fused_fisher(pobj, cap)
            return
        # (refused before anything is built; nothing falls back to differences)
        engine.check_grad_scope(batch, libs, pobj.npoly, pobj.resols, False,
                                vsini_grad=fit,
                                nn_gradient=getattr(pobj, 'nn_gradient', False),
                                resol_gradient=getattr(pobj, 'resol_gradient', False))
        self.pobj = pobj
        self.fisher = bool(fisher)
        dev = pobj.dev
        narm = len(batch.arms)
        self.ntan = pobj.ndim + (1 if fit else 0)
        self.vsini_mode = 2 if fit else (1 if pobj.has_vsini else 0)
        ntps = [libs[a.name].ntp for a in batch.arms]
        cap = self.choose_cap(pobj.S, ntps, self.ntan, self.vsini_mode, cap=cap,
                              budget=budget, row_capacity=pobj.cap, fisher=self.fisher)
        ntp = (ctypes.c_int32 * narm)(*ntps)
        work_size = L.rvs_fisher_chain_work_size if self.fisher else \
            L.rvs_grad_chain_work_size
        size = lambda c: work_size(  # noqa: E731
            c, narm, self.ntan, ntp, self.vsini_mode)
        self.cap = cap
        self.nbytes = int(size(cap))
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        K, R = 1 + self.ntan, 1 + pobj.ndim
        self.arms = (_lib.GradArm * narm)()
        self.point = (_lib.PointArm * narm)()
        self.bconst = (ctypes.c_double * narm)()
        self._keep = []
        for ia, arm in enumerate(batch.arms):
            lib = libs[arm.name]
            b = dict(templ=torch.empty((cap, K, lib.ntp), **f64),
                     templ2=torch.empty((cap, K, lib.ntp), **f64)
                     if self.vsini_mode else None,
                     coef=torch.empty((cap, K, lib.ntp, 4), **f64),
                     outside=torch.empty(cap, **f64), penalty=torch.empty(cap, **f64),
                     simplex=torch.empty(cap, **i32),
                     vs_rows=torch.empty(cap * R, **f64)
                     if self.vsini_mode == 1 else None,
                     out_rows=torch.empty(cap * R, **f64)
                     if self.vsini_mode == 1 else None)
            a = self.arms[ia]
            for k, t in b.items():
                setattr(a, k, None if t is None else t.data_ptr())
            a.knots = lib.knots.data_ptr()
            if lib.kind != 'nn':
                a.dats = lib.dats.data_ptr()
            a.factors = None if lib.spline_factors is None else \
                lib.spline_factors.data_ptr()
            a.spline_form, a.lnstep = lib.spline_form, lib.lnstep
            a.ntp, a.log_mask = lib.ntp, lib.log_mask
            a.exp_flag = getattr(lib, 'exp_flag', 1)
            if lib.kind == 'nn':
                # tri == 2: dats is a HOST rvs_nm_nn_arm; its activation buffer
                # (act1: cap (1 + ndim) float32 rows of the widest layer; act0 is
                # not used) is this object's, outside rvs_grad_chain_work_size
                lib.check_nn_grad_scope()
                n = _lib.NmNNArm()
                nl = len(lib.nn_W)
                Wp = (ctypes.c_void_p * nl)(*[w.data_ptr() for w in lib.nn_W])
                bp = (ctypes.c_void_p * nl)(*[x.data_ptr() for x in lib.nn_b])
                b['a1'] = torch.empty((cap * R, lib.nn_width()),
                                      dtype=torch.float32, device=dev)
                b['a0'] = b['a1'][:1]
                n.M, n.S = lib.nn_M.data_ptr(), lib.nn_S.data_ptr()
                n.W = ctypes.cast(Wp, ctypes.c_void_p)
                n.b = ctypes.cast(bp, ctypes.c_void_p)
                n.dims = lib.nn_dims.ctypes.data
                n.act0, n.act1 = b['a0'].data_ptr(), b['a1'].data_ptr()
                n.templ = n.outside = None
                hull = lib.hull_device()
                if hull is None:
                    n.xeqs = n.yeqs = None
                    n.nfx = n.nfy = 0
                else:
                    n.xeqs, n.yeqs = hull[0].data_ptr(), hull[1].data_ptr()
                    n.nfx, n.nfy = hull[0].shape[0], hull[1].shape[0]
                n.nlayer, n.log_mask = nl, lib.log_mask
                a.tri, a.dats = 2, ctypes.addressof(n)
                self._keep += [n, Wp, bp, hull]
            elif lib.kind == 'triangulation':
                from . import library
                a.tri, a.nsimplex = 1, lib.tri_nsimplex
                a.transform = lib.tri_transform.data_ptr()
                a.extraflags = lib.tri_extraflags.data_ptr()
                a.simplices = lib.tri_simplices.data_ptr()
                # (the search TemplateLibrary._tri_call chooses)
                if lib._tri_bk is not None and library.TRI_BUCKETS:
                    a.buckets = lib._tri_bk
            else:
                a.tri, a.ngrid = 0, lib.ngrid
                a.idgrid, a.uvecs = lib.idgrid.data_ptr(), lib.uvecs.data_ptr()
                a.vecs_s = lib.vecs_s.data_ptr()
                a.lens, a.ptp = lib.lens.ctypes.data, lib.ptp.ctypes.data
            self._keep.append(b)
            # (the arm's resolution matrix: the chain then ends in the _resol calls)
            rs = engine._arm_resol(arm, ia, pobj.resols)
            if rs is not None:
                engine.check_grad_resol_lds(self.ntan, rs['nd'])
            self._keep.append(engine.fill_point_arm(
                self.point[ia], arm, lib, pobj.npoly, pobj.rbf, 0.0, rs, b['coef'],
                b['penalty']))
            # the orthonormal basis of the same space, as engine.chisq_point_grad
            qt, const = arm.basis_ortho(pobj.npoly, pobj.rbf)
            self.point[ia].polysT = qt.data_ptr()
            self.bconst[ia] = const
            self._keep.append(qt)
        nb = L.rvs_chisq_point_grad_work_size(cap, narm, self.ntan)
        self.point_work = torch.empty((nb + 7) // 8, **f64)
        self.chi = torch.empty(cap, **f64)
        self.grad = torch.empty((cap, K), **f64)
        self.njev = torch.zeros(pobj.S, **i32)
        if self.fisher:
            nb = L.rvs_chisq_point_fisher_work_size(cap, narm, self.ntan)
            self.fisher_work = torch.empty((nb + 7) // 8, **f64)
            self.fisher_buf = torch.empty((cap, K, K), **f64)

    def _init_fused_rows(self, pobj, cap, key, check_scope, fisher, **scope_kw):
        """What both fused forms begin with: `check_scope` (engine.check_fused_*_scope
        with its keywords; refused before anything is built), the tangents, the rows of a chunk (ValueError
        naming the config key `key` where MAX_CHUNKS chunks do not hold a row per run),
        the kernels' arm descriptors and the chunk's chi / grad.  Returns the library,
        the tensor keywords and the number of arms for the form's own buffers."""
        batch, libs = pobj.batch, pobj.libs
        fit = pobj.vsini_col >= 0
        check_scope(batch, libs, pobj.npoly, pobj.resols, False, vsini_grad=fit,
                    **scope_kw)
        self.pobj, self.fisher = pobj, fisher
        narm = len(batch.arms)
        self.ntan = pobj.ndim + (1 if fit else 0)
        self.vsini_mode = 2 if fit else (1 if pobj.has_vsini else 0)
        cap = int(min(pobj.S if cap is None else cap, pobj.cap))
        if cap < 1 or (pobj.S + cap - 1) // cap > GradChain.MAX_CHUNKS:
            raise ValueError('%s: a round holds at most %d chunks of '
                             '%d rows: %d spectra do not fit one call; pass them in '
                             'smaller batches' % (key, GradChain.MAX_CHUNKS, cap, pobj.S))
        self.cap = cap
        f64 = dict(dtype=torch.float64, device=pobj.dev)
        self.garms = (_lib.ObjectiveArm * narm)()
        self.bconst = (ctypes.c_double * narm)()
        self._keep = engine.fill_objective_grad_arms(self.garms, self.bconst, batch, libs,
                                                     pobj.npoly, pobj.rbf,
                                                     resols=pobj.resols)
        self.chi = torch.empty(cap, **f64)
        self.grad = torch.empty((cap, 1 + self.ntan), **f64)
        self.njev = torch.zeros(pobj.S, dtype=torch.int32, device=pobj.dev)
        return _lib.lib(), f64, narm

    def _init_fused(self, pobj, cap, fisher):
        batch, libs = pobj.batch, pobj.libs
        L, f64, narm = self._init_fused_rows(
            pobj, cap, 'second_minimizer_jac', engine.check_fused_grad_scope, False,
            what='the Fisher form of the chain (fisher=True)' if fisher else None,
            nn_gradient=getattr(pobj, 'nn_gradient', False),
            tri_gradient=getattr(pobj, 'tri_gradient', False),
            resol_gradient=getattr(pobj, 'resol_gradient', False))
        cap = self.cap
        # arms under a resolution matrix (admitted with resol_gradient): the _resol forms
        # of the three runs
        self.fused_resol = any(engine._arm_resol(arm, ia, pobj.resols) is not None
                               for ia, arm in enumerate(batch.arms))
        # MLP libraries (admitted with nn_gradient): rvs_bfgs_run_grad_fused_nn;
        # Delaunay libraries (with tri_gradient): rvs_bfgs_run_grad_fused_tri
        self.fused_nn = libs[batch.arms[0].name].kind == 'nn'
        self.fused_tri = libs[batch.arms[0].name].kind == 'triangulation'
        if self.fused_nn or self.fused_tri:
            # the adjoint rows and the reverse pass's work of a chunk are this object's
            # (library.TRI_BUCKETS = False: the exhaustive search, which the rounds in the
            # library do not take)
            from . import library
            if not pobj.native or (self.fused_tri and not library.TRI_BUCKETS):
                raise ValueError("config['fused_gradient'] on %s libraries needs the "
                                 'rounds inside the library (the from-template objective%s)'
                                 % (('MLP', '') if self.fused_nn else
                                    ('Delaunay', ' with a bucket grid on every arm')))
            vg = 1 if pobj.vsini_col >= 0 else 0
            ls = [libs[a.name] for a in batch.arms]
            self.nbytes = int(L.rvs_objective_grad_from_template_work_size(cap, narm, vg))
            self.tbar = [torch.empty((cap, lib.ntp), **f64) for lib in ls]
            self.gparams = [torch.empty((cap, pobj.ndim), **f64) for lib in ls]
            self.grad_vv = torch.empty((cap, 1 + vg), **f64)
            self.tbar_p = (ctypes.c_void_p * narm)(*[t.data_ptr() for t in self.tbar])
            self.gparams_p = (ctypes.c_void_p * narm)(*[t.data_ptr()
                                                        for t in self.gparams])
            self.gwork = torch.empty((self.nbytes + 7) // 8, **f64)
            self.nbytes += sum(t.numel() * 8 for t in self.tbar + self.gparams)
            if self.fused_nn:
                # (the contraction with a simplex's tangents needs no work buffer)
                self.vjp_work = [torch.empty(
                    (int(L.rvs_template_nn_vjp_work_size(cap, len(lib.nn_W),
                                                         _lib.ptr(lib.nn_dims))) + 7) // 8,
                    **f64) for lib in ls]
                self.vjp_work_p = (ctypes.c_void_p * narm)(*[t.data_ptr()
                                                             for t in self.vjp_work])
                self.nbytes += sum(t.numel() * 8 for t in self.vjp_work)
        else:
            self.nbytes = int(L.rvs_objective_grad_work_size(cap, narm, self.ntan))
            self.gwork = torch.empty((self.nbytes + 7) // 8, **f64)

    def _init_fused_fisher(self, pobj, cap):
        L, f64, narm = self._init_fused_rows(pobj, cap, 'second_minimizer_lm',
                                             engine.check_fused_fisher_scope, True)
        cap, K = self.cap, 1 + self.ntan
        npix_max = max(a.npix for a in pobj.batch.arms)
        one = int(L.rvs_objective_fisher_work_size(1, narm, self.ntan, npix_max))
        rows = max(1, min(cap, FISHER_FUSED_WORK_BUDGET // one))
        self.nbytes = cap * K * K * 8 + rows * one
        self.fwork = torch.empty(self.nbytes // 8, **f64)

    MAX_CHUNKS = 24     # the chunk counters of the scan kernel (rounds_dev.h: BF_NCHUNK)

    @staticmethod
    def choose_cap(S, ntps, ntan, vsini_mode, cap=None, budget=None,
                   row_capacity=None, fisher=False):
        """rows per chunk for S runs on arms of ntps template pixels: `cap`, or the
        most whose buffers (rvs_grad_chain_work_size) stay inside `budget`
        (GRAD_CHAIN_BUDGET).  ValueError where MAX_CHUNKS chunks of that many rows
        do not hold one row per run: at the default budget, three arms of 8000
        template pixels and ntan = 6 that is beyond ~12 000 spectra per call.
        fisher: the chain of second_minimizer_lm, whose Fisher scratch and matrices
        (rvs_fisher_chain_work_size) count inside the same budget."""
        L = _lib.lib()
        key = 'second_minimizer_lm' if fisher else 'second_minimizer_jac'
        work_size = L.rvs_fisher_chain_work_size if fisher else \
            L.rvs_grad_chain_work_size
        narm = len(ntps)
        ntp = (ctypes.c_int32 * narm)(*ntps)
        if cap is None:
            budget = GRAD_CHAIN_BUDGET if budget is None else budget
            one = work_size(1, narm, ntan, ntp, vsini_mode)
            if one <= 0:
                raise ValueError('%s: GradChain: %d arms / %d tangents are outside '
                                 'rvs_grad_chain_work_size' % (key, narm, ntan))
            cap = max(1, min(S, int(budget // one)))
        cap = int(cap if row_capacity is None else min(cap, row_capacity))
        if cap < 1 or (S + cap - 1) // cap > GradChain.MAX_CHUNKS:
            raise ValueError(
                '%s: the gradient chain holds %d rows per chunk '
                '(optimizer.GRAD_CHAIN_BUDGET = %d bytes) and a round at most %d '
                'chunks: %d spectra do not fit one call; pass them in smaller batches'
                % (key, cap, GRAD_CHAIN_BUDGET if budget is None else budget,
                   GradChain.MAX_CHUNKS, S))
        return cap

    def desc(self):
        g = _lib.GradChain()
        g.basis_const = ctypes.addressof(self.bconst)
        ps = self.pobj.batch.pen_scale
        g.pen_scale = None if ps is None else ps.data_ptr()
        if not (self.fused or self.fused_fisher):   # (the fused runs read none of the three)
            g.arms, g.point = ctypes.addressof(self.arms), ctypes.addressof(self.point)
            g.point_work = self.point_work.data_ptr()
        g.chi, g.grad = self.chi.data_ptr(), self.grad.data_ptr()
        g.njev = self.njev.data_ptr()
        g.narm, g.ntan = len(self.pobj.batch.arms), self.ntan
        g.cap, g.vsini_mode = self.cap, self.vsini_mode
        return g

    def fisher_desc(self):
        """rvs_fisher_chain: the Fisher buffers of a chain built with fisher=True"""
        fc = _lib.FisherChain()
        fc.fisher_work = self.fisher_work.data_ptr()
        fc.fisher = self.fisher_buf.data_ptr()
        return fc

    def rows(self, idx, X):
        """(chisq_func, its gradient) of the rows X [J, n] of spectra idx [J]: numpy
        in, numpy [J, 1 + n] out -- rvs_proc_map, spec_fit.chisq_grad_jobs' launches
        and rvs_proc_finish_grad, driven from Python.  The objective of
        bfgs.minimize_lockstep_native(jac=True), and what rvs_bfgs_run_grad's rounds
        are held against.  With fisher=True: [J, 1 + n + n (n + 1) / 2] through
        rvs_chisq_point_fisher and rvs_proc_finish_fisher, the objective of
        lm.minimize_lockstep_native and what rvs_lm_run's rounds are held against (with
        fused_fisher=True: through rvs_objective_fisher, against rvs_lm_run_fused's)."""
        from . import spec_fit
        p, L = self.pobj, _lib.lib()
        dev = p.dev
        idx_t = torch.as_tensor(idx, dtype=torch.int32).to(dev).contiguous()
        X_t = torch.as_tensor(X, dtype=torch.float64).to(dev).contiguous()
        J = X_t.shape[0]
        width = p.n + 1 + (p.n * (p.n + 1) // 2 if self.fisher else 0)
        F = torch.empty((J, width), dtype=torch.float64, device=dev)
        st = _lib.stream()
        for a in range(0, J, p.cap):
            n = min(J, a + p.cap) - a
            rc = L.rvs_proc_map(n, p.n, p.ndim, _p(X_t[a:]), _p(idx_t[a:]), p.src,
                                p.vsini_col, _p(p.fixed), _p(p.vsini_fixed),
                                _p(p.safe), _p(p.prior_mean), _p(p.prior_isig),
                                p.min_vel, p.max_vel, p.max_vsini, _p(p.job_spec),
                                _p(p.vel), _p(p.vsini), _p(p.params), _p(p.extra),
                                _p(p.bad), st)
            _lib.check(rc, 'rvs_proc_map')
            res = spec_fit._chisq_grad(
                p.batch, p.libs, p.job_spec[:n], p.vel[:n], p.params[:n],
                None if p.vsini is None else p.vsini[:n], p.npoly, p.rbf, 0.0, True,
                p.resols, False, p.vsini_col >= 0, self.fisher,
                nn_gradient=getattr(p, 'nn_gradient', False),
                tri_gradient=getattr(p, 'tri_gradient', False),
                resol_gradient=getattr(p, 'resol_gradient', False), fused=self.fused,
                fused_fisher=self.fused_fisher)
            chi, grad, status = res[0], res[1], res[-1]
            tail = (_p(X_t[a:]), _p(p.params), _p(p.extra), _p(p.bad), _p(p.job_spec),
                    _p(status), p.src, p.vsini_col, _p(p.prior_mean), _p(p.prior_isig),
                    p.max_vsini, _p(F[a:]), _p(p.status), st)
            head = (n, p.n, p.ndim, self.ntan, None, 0, _p(chi), _p(grad.contiguous()))
            if self.fisher:
                rc = L.rvs_proc_finish_fisher(*head, _p(res[2].contiguous()), *tail)
                _lib.check(rc, 'rvs_proc_finish_fisher')
            else:
                rc = L.rvs_proc_finish_grad(*head, *tail)
                _lib.check(rc, 'rvs_proc_finish_grad')
            p.calls += 1
            p.jobs += n
        return F.cpu().numpy()


# False: the rounds of a fused objective are driven from Python (one_round below,
# the loop every non-fused objective takes anyway) instead of rvs_nm_run; the
# two give the same simplices bit for bit
# (tests/test_gpu_parity.py::test_nm_round_drivers_agree).
# (Replaying the rounds from HIP graphs was measured in round 1: same wall time --
# the rounds are bound by the GPU-side chain of small dependent kernels, not by
# host launches -- and removed.)
NATIVE_ROUNDS = True


def _order(sim, fsim):
    """scipy: ind = np.argsort(fsim); sim = np.take(sim, ind, 0) -- stable, so
    that equal values keep their vertex order"""
    # (np.argsort on <= 16 elements is an insertion sort, i.e. stable; NaN last)
    key = torch.where(torch.isnan(fsim), torch.full_like(fsim, float('inf')),
                      fsim)
    ind = torch.sort(key, dim=1, stable=True)[1]
    fsim = torch.gather(fsim, 1, ind)
    sim = torch.gather(sim, 1, ind[:, :, None].expand_as(sim))
    return sim, fsim


class DeviceNelderMead:

    def __init__(self, S, N, dev):
        self.S, self.N, self.dev = S, N, dev
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        self.fsim = torch.empty((S, N + 1), **f64)
        self.nit = torch.ones(S, **i32)
        self.nfev = torch.full((S, ), N + 1, **i32)
        self.flags = torch.ones(S, **i32)
        self.list1 = torch.zeros(S, **i32)
        self.list2 = torch.zeros(S, **i32)
        self.list3 = torch.zeros(S, **i32)
        self.X1 = torch.zeros((S, N), **f64)
        self.X2 = torch.zeros((S, N), **f64)
        self.F1 = torch.zeros(S, **f64)
        self.F2 = torch.zeros(S, **f64)
        self.cases = torch.zeros(S, **i32)
        self.pos2 = torch.zeros(S, **i32)
        self.counts = torch.zeros(8, **i32)

    def minimize(self, objective, simplex, fatol=1e-3, xatol=1e-2,
                 maxiter=10000, sync_every=4, stats=None):
        L = _lib.lib()
        S, N = self.S, self.N
        sim = simplex.clone().to(torch.float64).contiguous()
        allidx = torch.arange(S, dtype=torch.int32, device=self.dev)
        for k in range(N + 1):
            self.X1.copy_(sim[:, k])
            objective.eval(allidx, self.X1, S, None, 0, self.F1)
            self.fsim[:, k] = self.F1
        sim, fsim = _order(sim, self.fsim)
        sim = sim.contiguous()
        self.fsim.copy_(fsim)
        fs = self.fsim
        if NATIVE_ROUNDS and isinstance(objective, ProcessObjective) and \
                objective.native:
            # the rounds in C (rvs_nm_run): same launches, no interpreter
            m = _lib.NmState()
            for k, t in (('sim', sim), ('fsim', fs), ('X1', self.X1),
                         ('X2', self.X2), ('F1', self.F1), ('F2', self.F2),
                         ('nit', self.nit), ('nfev', self.nfev),
                         ('flags', self.flags), ('list1', self.list1),
                         ('list2', self.list2), ('list3', self.list3),
                         ('cases', self.cases), ('pos2', self.pos2),
                         ('counts', self.counts)):
                setattr(m, k, t.data_ptr())
            m.S, m.N = S, N
            o = objective.native_desc()
            st3 = (ctypes.c_int64 * 3)()
            nfev0 = self.nfev.sum()
            rc = L.rvs_nm_run(ctypes.addressof(m), ctypes.addressof(o), float(xatol),
                              float(fatol), int(maxiter), int(sync_every), st3,
                              _lib.stream())
            _lib.check(rc, 'rvs_nm_run')
            objective.calls += int(st3[1])
            # evaluations performed = the function values scipy's algorithm counts
            # (rows of a launch behind the device count are skipped); `slots` =
            # rows launched
            objective.jobs += int((self.nfev.sum() - nfev0).item())
            objective.slots += int(st3[2])
            return self._result(sim, fs, int(st3[0]), stats)

        def begin(jb):
            rc = L.rvs_nm_begin(S, N, xatol, fatol, maxiter, _p(sim), _p(fs),
                                _p(self.nit), _p(self.flags), _p(self.list1),
                                _p(self.X1), _p(self.counts), jb, _lib.stream())
            _lib.check(rc, 'rvs_nm_begin')

        def one_round(jb):
            st = _lib.stream()
            begin(jb)
            objective.eval(self.list1, self.X1, jb, self.counts, 0, self.F1)
            rc = L.rvs_nm_decide(N, _p(sim), _p(fs), _p(self.list1),
                                 _p(self.F1), _p(self.cases), _p(self.pos2),
                                 _p(self.list2), _p(self.X2), _p(self.counts), jb,
                                 st)
            _lib.check(rc, 'rvs_nm_decide')
            objective.eval(self.list2, self.X2, jb, self.counts, 1, self.F2)
            rc = L.rvs_nm_update(N, _p(sim), _p(fs), _p(self.nit),
                                 _p(self.nfev), _p(self.list1), _p(self.X1),
                                 _p(self.F1), _p(self.cases), _p(self.pos2),
                                 _p(self.X2), _p(self.F2), _p(self.flags),
                                 _p(self.counts), jb, st)
            _lib.check(rc, 'rvs_nm_update')

        # launch bounds are quantised (1/8 steps of a power of two) so that a
        # handful of launch shapes serve the whole run
        def bucket(n):
            if n <= 64:
                return min(S, 64)
            p2 = 1 << (int(n - 1).bit_length())      # next power of two >= n
            stepq = max(p2 // 8, 1)
            return min(S, -(-n // stepq) * stepq)

        jb = S
        rounds = 0
        begin(jb)
        while True:
            # host look: counts of the most recent begin (an upper bound of what
            # is active now), parked shrinks
            c = self.counts.cpu().numpy()
            live, parked = int(c[0]), int(c[4])
            if parked > 0:
                self._shrink(objective, sim, parked)
                begin(S)
                continue
            if live == 0:
                break
            jb = bucket(live)
            for _ in range(sync_every):
                one_round(jb)
            rounds += sync_every
        return self._result(sim, fs, rounds, stats)

    def _result(self, sim, fs, rounds, stats):
        if stats is not None:
            stats['rounds'] = stats.get('rounds', 0) + rounds
        success = (self.flags & 2) != 0
        return dict(x=sim[:, 0].clone(), fun=fs.min(dim=1)[0],
                    nit=self.nit.long(), nfev=self.nfev.long(), success=success,
                    final_simplex=(sim, fs))

    def _shrink(self, objective, sim, parked):
        """scipy's shrink step for the parked simplices: N objective calls"""
        L = _lib.lib()
        N = self.N
        st = _lib.stream()
        rc = L.rvs_nm_collect(self.S, _p(self.flags), _p(self.list3),
                              _p(self.counts), st)
        _lib.check(rc, 'rvs_nm_collect')
        jb = parked
        for k in range(1, N + 1):
            rc = L.rvs_nm_shrink_point(N, k, _p(sim), _p(self.list3),
                                       _p(self.X2), _p(self.counts), jb, st)
            _lib.check(rc, 'rvs_nm_shrink_point')
            objective.eval(self.list3, self.X2, jb, self.counts, 2, self.F2)
            rc = L.rvs_nm_shrink_store(N, k, _p(sim), _p(self.fsim),
                                       _p(self.nit), _p(self.nfev),
                                       _p(self.flags), _p(self.list3),
                                       _p(self.F2), _p(self.counts), jb, st)
            _lib.check(rc, 'rvs_nm_shrink_store')


class TorchObjective:
    """adapter: a torch callable f(idx long [J], X [J,N]) -> [J] behind the
    ProcessObjective.eval interface (tests of DeviceNelderMead)"""

    def __init__(self, func):
        self.func = func

    def eval(self, list_t, X, J, counts, cidx, F):
        F[:J] = self.func(list_t[:J].long(), X[:J])


class EpochChain:
    """The joint objective of vel_fit.process_epochs: one set of stellar parameters (and
    one vsini) per star, one velocity per epoch.  GradChain(fisher=True) with two
    capacities -- `cap_star` rows for the template / FIR / spline stage, which runs ONCE
    per star, and `cap_epoch` jobs for the point stage, which reads a star's records
    through job_templ:

      rvs_epoch_map            theta [J, m], v -> per star params, vsini, prior / vsini
                               penalty, bad; per epoch vel and job_templ
      engine.build_templates   per arm: the star's template, its tangents, the
                               broadening, the spline records (cap_star rows)
      rvs_chisq_point_fisher   chi, grad, fisher of every epoch; the penalty of an epoch
                               is outside[star] x badchi of the epoch's spectrum
      rvs_epoch_finish         the star's arrow row (alm.row_size)

    `batch` holds the epochs sorted by star: star n owns the rows eoff[n] ..
    eoff[n + 1] - 1.  pd0 / priors / safe_params are per STAR ([N] / [N, ndim]).  theta's
    columns are ParamMapper.get_fitted_params() without 'vel': [vsini,] free stellar
    parameters.  A chunk holds whole stars.  The scope is engine.check_grad_scope's."""

    def __init__(self, batch, libs, names, pd0, fixParam, fitVsini, config, options,
                 priors, safe_params, eoff, resols=None, cap_star=None, cap_epoch=None):
        from . import alm
        self.batch, self.libs = batch, libs
        dev = batch.device
        self.dev = dev
        self.eoff = np.asarray(eoff, dtype=np.int64)
        self.nE = np.diff(self.eoff)
        N = len(self.nE)
        if N < 1 or self.eoff[0] != 0 or self.eoff[-1] != batch.S:
            raise ValueError('EpochChain: eoff does not cover the %d epochs of the batch'
                             % batch.S)
        if (self.nE < 1).any():
            raise ValueError('EpochChain: star %d has no epochs'
                             % int(np.nonzero(self.nE < 1)[0][0]))
        self.N = N
        self.npoly = options.get('npoly') or 5
        self.rbf = options.get('rbf_continuum', True)
        self.resols = resols
        self.nn_gradient = bool(config.get('nn_gradient'))
        self.resol_gradient = bool(config.get('resol_gradient'))
        engine.check_grad_scope(batch, libs, self.npoly, resols,
                                bool(options.get('fast_interp')), vsini_grad=fitVsini,
                                nn_gradient=self.nn_gradient,
                                resol_gradient=self.resol_gradient)
        self.ndim = len(names)
        f64 = dict(dtype=torch.float64, device=dev)
        self.has_vsini = 'vsini' in pd0
        k = 0
        self.vsini_col = -1
        if fitVsini:
            self.vsini_col = k
            k += 1
        src = []
        for x in names:
            if x in fixParam:
                src.append(-1)
            else:
                src.append(k)
                k += 1
        self.m = k
        if not 1 <= self.m <= alm.MAXM:
            raise ValueError('the joint fit takes 1 <= m <= %d shared parameters per '
                             'star, not m = %d' % (alm.MAXM, self.m))
        self.ntan = self.ndim + (1 if fitVsini else 0)
        self.src = (ctypes.c_int32 * self.ndim)(*src)
        self.fixed = torch.stack([pd0[_] for _ in names], dim=1).contiguous()
        self.vsini_fixed = pd0['vsini'].contiguous() if (
            self.has_vsini and not fitVsini) else None
        self.safe = safe_params.contiguous()
        assert self.fixed.shape == (N, self.ndim) and self.safe.shape == self.fixed.shape
        self.prior_mean = self.prior_isig = None
        if priors:
            pm = torch.zeros((N, self.ndim), **f64)
            ps = torch.zeros((N, self.ndim), **f64)
            for i, x in enumerate(names):
                if x in priors:
                    mu, sg = priors[x]
                    pm[:, i] = torch.as_tensor(mu, **f64)
                    ps[:, i] = 1.0 / torch.as_tensor(sg, **f64)
            self.prior_mean, self.prior_isig = pm, ps
        self.min_vel, self.max_vel = float(config['min_vel']), float(config['max_vel'])
        self.max_vsini = float(config['max_vsini'])
        # capacities: the template stage's buffers are the chain's big ones
        ntps = [libs[a.name].ntp for a in batch.arms]
        if cap_star is None:
            L = _lib.lib()
            ntp = (ctypes.c_int32 * len(ntps))(*ntps)
            one = L.rvs_fisher_chain_work_size(
                1, len(ntps), self.ntan, ntp,
                2 if fitVsini else (1 if self.has_vsini else 0))
            if one <= 0:
                raise ValueError('EpochChain: %d arms / %d tangents are outside '
                                 'rvs_fisher_chain_work_size' % (len(ntps), self.ntan))
            cap_star = max(1, min(N, int(GRAD_CHAIN_BUDGET // one)))
        self.cap_star = int(cap_star)
        self.cap_epoch = int(batch.S if cap_epoch is None else cap_epoch)
        if self.cap_star < 1 or int(self.nE.max()) > self.cap_epoch:
            raise ValueError('EpochChain: star %d has %d epochs, a chunk holds whole '
                             'stars and cap_epoch = %d epochs'
                             % (int(self.nE.argmax()), int(self.nE.max()),
                                self.cap_epoch))
        self.status = torch.zeros(N, dtype=torch.int32, device=dev)
        self.calls = 0          # chunks evaluated
        self.star_rows = 0      # template-stage rows (stars)
        self.epoch_jobs = 0     # point-stage jobs (epochs)
        self.keep_epochs = False
        self.epochs = None      # the epochs' chi, grad, fisher of the last rows() call

    def _chunk(self, ids, theta, vel):
        from . import alm
        L, dev, st = _lib.lib(), self.dev, _lib.stream()
        n, m, ndim = len(ids), self.m, self.ndim
        nE = self.nE[ids]
        leoff = np.concatenate([[0], np.cumsum(nE)])
        S = int(leoff[-1])
        ro = alm.offsets(m, leoff)[1]
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        # one upload of the chunk's integer tables (rowoff first: int64 at offset 0) and
        # one of its vectors, not six small copies per chunk and round
        ids = np.asarray(ids, dtype=np.int64)
        spec = np.repeat(self.eoff[ids] - leoff[:-1], nE) + np.arange(S)
        ints = torch.as_tensor(np.concatenate([
            ro[:-1].astype(np.int64).view(np.int32), leoff.astype(np.int32),
            ids.astype(np.int32), spec.astype(np.int32)])).to(dev)
        ro_t = ints[:2 * n].view(torch.int64)
        eoff_t = ints[2 * n:3 * n + 1]
        list_t = ints[3 * n + 1:4 * n + 1]
        job_spec = ints[4 * n + 1:]
        vecs = torch.as_tensor(np.concatenate([
            np.asarray(theta, dtype=np.float64).reshape(-1),
            np.asarray(vel, dtype=np.float64).reshape(-1)])).to(dev)
        theta_t, velin = vecs[:n * m].view(n, m), vecs[n * m:]
        assert theta_t.shape == (n, m) and velin.shape == (S, )
        star_id, bad = torch.empty(n, **i32), torch.empty(n, **i32)
        job_templ = torch.empty(S, **i32)
        velo, params = torch.empty(S, **f64), torch.empty((n, ndim), **f64)
        vsini = torch.empty(n, **f64) if self.has_vsini else None
        extra = torch.empty(n, **f64)
        rc = L.rvs_epoch_map(n, S, m, ndim, _p(theta_t), _p(velin), _p(eoff_t),
                             _p(list_t), self.src, self.vsini_col, _p(self.fixed),
                             _p(self.vsini_fixed), _p(self.safe), _p(self.prior_mean),
                             _p(self.prior_isig), self.min_vel, self.max_vel,
                             self.max_vsini, _p(star_id), _p(job_templ), _p(velo),
                             _p(vsini), _p(params), _p(extra), _p(bad), st)
        _lib.check(rc, 'rvs_epoch_map')
        coefs, outs = [], []
        for arm in self.batch.arms:
            c, o = engine.build_templates(self.libs[arm.name], params, vsini,
                                          tangents=True,
                                          vsini_tangent=self.vsini_col >= 0)
            coefs.append(c)
            outs.append(o)
        chi, grad, fisher, status = engine.chisq_point_fisher(
            self.batch, self.libs, coefs, outs, velo, npoly=self.npoly, rbf=self.rbf,
            job_spec=job_spec, job_templ=job_templ, resols=self.resols,
            nn_gradient=self.nn_gradient, resol_gradient=self.resol_gradient)
        F = torch.empty(int(ro[-1]), **f64)
        # (named before their pointers are taken: they outlive the launch)
        grad, fisher = grad.contiguous(), fisher.contiguous()
        rc = L.rvs_epoch_finish(n, m, ndim, self.ntan, None, 0, _p(eoff_t), _p(ro_t),
                                _p(chi), _p(grad), _p(fisher),
                                _p(theta_t), _p(params), _p(extra), _p(bad), _p(star_id),
                                _p(status), self.src, self.vsini_col,
                                _p(self.prior_mean), _p(self.prior_isig), self.max_vsini,
                                _p(F), _p(self.status), st)
        _lib.check(rc, 'rvs_epoch_finish')
        self.calls += 1
        self.star_rows += n
        self.epoch_jobs += S
        ep = None
        if self.keep_epochs == 'values':    # (what process_epochs reports, no more)
            ep = dict(chi=chi.cpu().numpy(), params=params.cpu().numpy(),
                      vsini=None if vsini is None else vsini.cpu().numpy())
        elif self.keep_epochs:
            ep = dict(chi=chi.cpu().numpy(), grad=grad.cpu().numpy(),
                      fisher=fisher.cpu().numpy(), status=status.cpu().numpy(),
                      params=params.cpu().numpy(), extra=extra.cpu().numpy(),
                      bad=bad.cpu().numpy(), vel=velo.cpu().numpy(),
                      vsini=None if vsini is None else vsini.cpu().numpy())
        return F.cpu().numpy(), ep

    def rows(self, star_idx, theta, vel):
        """the arrow rows of the stars star_idx [J] at theta [J, m] and the velocities
        `vel` (ragged: the stars' epochs one behind the other), numpy in, the ragged
        rows as numpy out -- the objective of alm.minimize_lockstep_native."""
        ids = np.asarray(star_idx, dtype=np.int64).reshape(-1)
        theta = np.asarray(theta, dtype=np.float64).reshape(len(ids), self.m)
        vel = np.asarray(vel, dtype=np.float64).reshape(-1)
        nE = self.nE[ids]
        if vel.shape[0] != nE.sum():
            raise ValueError('EpochChain.rows: %d velocities for %d epochs'
                             % (vel.shape[0], nE.sum()))
        out, eps = [], []
        a = va = 0
        one = len(ids) <= self.cap_star and nE.sum() <= self.cap_epoch
        while a < len(ids):
            b, ne = (len(ids), int(nE.sum())) if one else (a, 0)
            while b < len(ids) and b - a < self.cap_star and \
                    ne + nE[b] <= self.cap_epoch:
                ne += int(nE[b])
                b += 1
            F, ep = self._chunk(ids[a:b], theta[a:b], vel[va:va + ne])
            out.append(F)
            eps.append(ep)
            a, va = b, va + ne
        if self.keep_epochs:
            self.epochs = {k: (None if eps[0][k] is None else
                               np.concatenate([e[k] for e in eps])) for k in eps[0]}
        return np.concatenate(out)

    def objective(self, idx, X, xoff):
        """rows() in the calling convention of alm.minimize_lockstep_native: X holds
        the vectors (theta [m], v [E]) of the stars idx one behind the other"""
        m = self.m
        xoff = np.asarray(xoff, dtype=np.int64)
        X = np.asarray(X, dtype=np.float64)
        at = xoff[:-1, None] + np.arange(m)[None, :]
        isvel = np.ones(int(xoff[-1]), dtype=bool)
        isvel[at.reshape(-1)] = False
        return self.rows(idx, X[at], X[:int(xoff[-1])][isvel])

    def native_desc(self):
        """rvs_epoch_chain: this chain for the rounds inside the library (rvs_alm_run),
        built once: the arm descriptors of GradChain with the template stage's buffers
        for cap_star rows and the point stage's for cap_epoch jobs"""
        if getattr(self, '_native', None) is not None:
            return self._native
        L = _lib.lib()
        batch, libs, dev = self.batch, self.libs, self.dev
        narm = len(batch.arms)
        cs, ce = self.cap_star, self.cap_epoch
        fit = self.vsini_col >= 0
        mode = 2 if fit else (1 if self.has_vsini else 0)
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        K, R = 1 + self.ntan, 1 + self.ndim
        arms = (_lib.GradArm * narm)()
        point = (_lib.PointArm * narm)()
        bconst = (ctypes.c_double * narm)()
        keep = []
        for ia, arm in enumerate(batch.arms):
            lib = libs[arm.name]
            b = dict(templ=torch.empty((cs, K, lib.ntp), **f64),
                     templ2=torch.empty((cs, K, lib.ntp), **f64) if mode else None,
                     coef=torch.empty((cs, K, lib.ntp, 4), **f64),
                     outside=torch.empty(cs, **f64), penalty=torch.empty(ce, **f64),
                     simplex=torch.empty(cs, **i32),
                     vs_rows=torch.empty(cs * R, **f64) if mode == 1 else None,
                     out_rows=torch.empty(cs * R, **f64) if mode == 1 else None)
            a = arms[ia]
            for k, t in b.items():
                setattr(a, k, None if t is None else t.data_ptr())
            a.knots = lib.knots.data_ptr()
            if lib.kind != 'nn':
                a.dats = lib.dats.data_ptr()
            a.factors = None if lib.spline_factors is None else \
                lib.spline_factors.data_ptr()
            a.spline_form, a.lnstep = lib.spline_form, lib.lnstep
            a.ntp, a.log_mask = lib.ntp, lib.log_mask
            a.exp_flag = getattr(lib, 'exp_flag', 1)
            if lib.kind == 'nn':
                lib.check_nn_grad_scope()
                n = _lib.NmNNArm()
                nl = len(lib.nn_W)
                Wp = (ctypes.c_void_p * nl)(*[w.data_ptr() for w in lib.nn_W])
                bp = (ctypes.c_void_p * nl)(*[x.data_ptr() for x in lib.nn_b])
                b['a1'] = torch.empty((cs * R, lib.nn_width()), dtype=torch.float32,
                                      device=dev)
                b['a0'] = b['a1'][:1]
                n.M, n.S = lib.nn_M.data_ptr(), lib.nn_S.data_ptr()
                n.W = ctypes.cast(Wp, ctypes.c_void_p)
                n.b = ctypes.cast(bp, ctypes.c_void_p)
                n.dims = lib.nn_dims.ctypes.data
                n.act0, n.act1 = b['a0'].data_ptr(), b['a1'].data_ptr()
                n.templ = n.outside = None
                hull = lib.hull_device()
                if hull is None:
                    n.xeqs = n.yeqs = None
                    n.nfx = n.nfy = 0
                else:
                    n.xeqs, n.yeqs = hull[0].data_ptr(), hull[1].data_ptr()
                    n.nfx, n.nfy = hull[0].shape[0], hull[1].shape[0]
                n.nlayer, n.log_mask = nl, lib.log_mask
                a.tri, a.dats = 2, ctypes.addressof(n)
                keep += [n, Wp, bp, hull]
            elif lib.kind == 'triangulation':
                from . import library
                a.tri, a.nsimplex = 1, lib.tri_nsimplex
                a.transform = lib.tri_transform.data_ptr()
                a.extraflags = lib.tri_extraflags.data_ptr()
                a.simplices = lib.tri_simplices.data_ptr()
                if lib._tri_bk is not None and library.TRI_BUCKETS:
                    a.buckets = lib._tri_bk
            else:
                a.tri, a.ngrid = 0, lib.ngrid
                a.idgrid, a.uvecs = lib.idgrid.data_ptr(), lib.uvecs.data_ptr()
                a.vecs_s = lib.vecs_s.data_ptr()
                a.lens, a.ptp = lib.lens.ctypes.data, lib.ptp.ctypes.data
            keep.append(b)
            rs = engine._arm_resol(arm, ia, self.resols)
            if rs is not None:
                engine.check_grad_resol_lds(self.ntan, rs['nd'])
            keep.append(engine.fill_point_arm(point[ia], arm, lib, self.npoly, self.rbf,
                                              0.0, rs, b['coef'], b['penalty']))
            qt, const = arm.basis_ortho(self.npoly, self.rbf)
            point[ia].polysT = qt.data_ptr()
            bconst[ia] = const
            keep.append(qt)
        nb = L.rvs_chisq_point_fisher_work_size(ce, narm, self.ntan)
        bufs = dict(fisher_work=torch.empty((nb + 7) // 8, **f64),
                    chi=torch.empty(ce, **f64), grad=torch.empty((ce, K), **f64),
                    fisher=torch.empty((ce, K, K), **f64),
                    theta=torch.empty((cs, self.m), **f64),
                    vsini=torch.empty(cs, **f64) if self.has_vsini else None,
                    params=torch.empty((cs, self.ndim), **f64),
                    extra=torch.empty(cs, **f64), velin=torch.empty(ce, **f64),
                    vel=torch.empty(ce, **f64), star_id=torch.empty(cs, **i32),
                    bad=torch.empty(cs, **i32), job_templ=torch.empty(ce, **i32),
                    jstatus=torch.empty(ce, **i32))
        c = _lib.EpochChain()
        c.arms, c.point = ctypes.addressof(arms), ctypes.addressof(point)
        c.basis_const = ctypes.addressof(bconst)
        ps = batch.pen_scale
        c.pen_scale = None if ps is None else ps.data_ptr()
        for k, t in bufs.items():
            setattr(c, k, None if t is None else t.data_ptr())
        for k, t in (('fixed', self.fixed), ('vsini_fixed', self.vsini_fixed),
                     ('safe', self.safe), ('prior_mean', self.prior_mean),
                     ('prior_isig', self.prior_isig), ('status', self.status)):
            setattr(c, k, None if t is None else t.data_ptr())
        c.min_vel, c.max_vel = self.min_vel, self.max_vel
        c.max_vsini, c.badchi = self.max_vsini, float(batch.badchi)
        c.narm, c.npoly, c.ntan, c.vsini_mode = narm, self.npoly, self.ntan, mode
        c.m, c.ndim, c.vsini_col = self.m, self.ndim, self.vsini_col
        c.cap_star, c.cap_epoch = cs, ce
        for i in range(8):
            c.src[i] = self.src[i] if i < self.ndim else -1
        self._native_keep = (arms, point, bconst, keep, bufs)
        self._native = c
        return c
