"""B quasistatic iRS-LQR problems side by side: `IrsLqrQuasistaticBatch`.

An iteration of `IrsLqrQuasistatic` is a sample pass followed by one bounded descent -- two waves on one compute
unit for ~98 % of its time.  Users of a contact-rich optimiser run the same task from several initial guesses, start
states or goals anyway; as separate `IrsLqrQuasistatic` objects those descents queue behind each other on that one
unit.  Here the B descents of an iteration are ONE launch (`irs_quasistatic_box_descent_batch`: the same kernel with
a problem index, one workgroup per problem), their trust-region rows one more, and the B sample passes a third
(`irs_smooth_rng_batch`: the sample-pass kernel over B x T rows, every row with the launch geometry, the draws and the
summation order of the single call) -- each problem with its seed, its `std_u` schedule and the shared iteration
counter, so every problem sees the draws, and computes the bits, of an `IrsLqrQuasistatic` given the same parameters.
`batched_sample_pass=False` (or a model / mode the batched pass does not serve) sends the B sample passes through the
single-problem entry back to back on the stream instead: the same bits, B launches and B library calls.  Exact mode
linearises per problem either way.

The problems share the model, `T`, the cost dictionaries, `gradient_mode`, `num_samples`, `sampling`, the kind of
bound and the QP settings; they may differ in `x0`, `x_trj_d`, `u_trj_0`, the bound values, `std_u_initial` and
`device_rng_seed`.
"""
import numpy as np
import torch

from . import device as dev
from . import distributed as dist_util
from .batch_common import StackedResults, seed_bits
from .irs_lqr_quasistatic import QP_FIELDS, SAMPLED_MODE, decouple_AB_dev, descent_failure, qp_settings
from .quasistatic_base import COST_TERMS, QuasistaticOptimizerBase


def _same_function(f, g):
    """The same callable: one object, or two functions of the same code, defaults and closure values."""
    if f is g:
        return True
    try:
        cells = lambda h: [c.cell_contents for c in (h.__closure__ or ())]     # noqa: E731
        return f.__code__ is g.__code__ and f.__defaults__ == g.__defaults__ and cells(f) == cells(g)
    except (AttributeError, ValueError):
        return False


def _same_dict(a, b):
    return (a is None and b is None) or (a is not None and b is not None and set(a) == set(b) and all(
        np.array_equal(np.asarray(a[k], float), np.asarray(b[k], float)) for k in a))


def _bound_kind(p):
    return "abs" if p.u_bounds_abs is not None else ("rel" if p.u_bounds_rel is not None else "none")


class _Problem(QuasistaticOptimizerBase):
    """One problem's data, initial rollout, history lists and best-so-far: the bookkeeping of the single class."""

    def __init__(self, q_dynamics, params):
        self._setup(q_dynamics, params, params.x_trj_d)
        self.verbose = False


class IrsLqrQuasistaticBatch(StackedResults):
    def __init__(self, q_dynamics, params_list, batched_sample_pass=True):
        ps = list(params_list)
        if not ps:
            raise ValueError("params_list is empty")
        p0 = ps[0]
        # ---- what the one launch shares (no GPU is touched before all of this has passed) ----
        for b, p in enumerate(ps[1:], 1):
            for field in ("T", "gradient_mode", "decouple_AB", "num_samples"):
                if getattr(p, field) != getattr(p0, field):
                    raise ValueError("params_list[%d].%s differs from params_list[0].%s" % (b, field, field))
            for field in ("Q_dict", "Qd_dict", "R_dict"):
                if not _same_dict(getattr(p, field), getattr(p0, field)):
                    raise ValueError("params_list[%d].%s differs from params_list[0].%s" % (b, field, field))
            if not _same_function(p.sampling, p0.sampling):
                raise ValueError("params_list[%d].sampling differs from params_list[0].sampling" % b)
            for field in ("x_bounds_abs", "x_bounds_rel"):
                if (getattr(p, field) is None) != (getattr(p0, field) is None):
                    raise ValueError("params_list[%d].%s: the problems must have the same kind of bound" % (b, field))
            if (p.u_bounds_abs is None, p.u_bounds_rel is None) != (p0.u_bounds_abs is None, p0.u_bounds_rel is None):
                raise ValueError("params_list[%d].u_bounds_abs / u_bounds_rel: the problems must have the same kind of "
                                 "bound (abs or rel)" % b)
            for field, value, value0 in zip(QP_FIELDS, qp_settings(p), qp_settings(p0)):
                if value != value0:
                    raise ValueError("params_list[%d].%s differs from params_list[0].%s" % (b, field, field))
        # ---- what the batched path serves ----
        if p0.gradient_mode not in ("zero_order_B", "first_order", "exact"):
            raise NotImplementedError("gradient_mode %r: the batch runs zero_order_B, first_order and exact"
                                      % (p0.gradient_mode,))
        if not p0.decouple_AB:
            raise NotImplementedError("the batch needs decouple_AB = True")
        if p0.gradient_mode != "exact" and any(getattr(p, "device_rng_seed", None) is None for p in ps):
            raise NotImplementedError("the sampled gradient modes need params.device_rng_seed for every problem (host "
                                      "draws would serialise the B sample passes)")
        if p0.x_bounds_abs is not None or p0.x_bounds_rel is not None:
            raise NotImplementedError("state bounds are not served by the batched descent")
        if p0.u_bounds_abs is not None and p0.u_bounds_rel is not None:
            raise NotImplementedError("the batched descent takes ONE control box: u_bounds_abs or u_bounds_rel")
        if int(qp_settings(p0)[0]) not in (0, 3):
            raise NotImplementedError("the batched descent is solver 3's method (qp_solver 0 or 3)")
        if any(getattr(p, "qp_adaptive_rho", False) for p in ps):
            raise NotImplementedError("qp_adaptive_rho belongs to the ADMM (solver 1); the batched descent is solver "
                                      "3's method")
        if any(getattr(p, "qp_lazy_bounds", False) for p in ps):
            raise NotImplementedError("qp_lazy_bounds belongs to the ADMM (solver 1); the batched descent is solver "
                                      "3's method")
        dm = q_dynamics.dm()
        if not dm.quasistatic_descent_supported(p0.T, 3):
            raise NotImplementedError("the model does not fit the matrix-core tile of the batched descent")

        self.q_dynamics, self.params_list, self._dm = q_dynamics, ps, dm
        self.B, self.T, self.dim_x, self.dim_u = len(ps), p0.T, q_dynamics.dim_x, q_dynamics.dim_u
        self.gradient_mode, self.num_samples = p0.gradient_mode, p0.num_samples
        self._kind = _bound_kind(p0)
        self.problems = [_Problem(q_dynamics, p) for p in ps]
        self.status = [None] * self.B
        self.current_iter = 1
        self.verbose = False

        pr0 = self.problems[0]
        device = pr0._x0.device
        self._Q, self._Qd, self._R = pr0._Q, pr0._Qd, pr0._R
        self._xd = torch.stack([pr._xd for pr in self.problems]).contiguous()
        self._idx = torch.as_tensor(np.asarray(pr0.indices_u_into_x), device=device)          # int64: torch indexing
        self._idx32 = self._idx.to(torch.int32).contiguous()
        # trust-region offsets (B,2,m), or (B,2,T,m) as soon as one problem gives per-time rows; no bound: +-inf
        T, m = self.T, self.dim_u
        offs = [np.asarray(p.u_bounds_abs if self._kind == "abs" else p.u_bounds_rel, float) if self._kind != "none"
                else np.array([-np.ones(m) * np.inf, np.ones(m) * np.inf]) for p in ps]
        if any(o.ndim == 3 for o in offs):
            offs = [np.broadcast_to(o if o.ndim == 3 else o[:, None, :], (2, T, m)) for o in offs]
        self._offsets = dev.to_dev(np.ascontiguousarray(np.stack(offs)))
        self._rows = None
        self._act = None
        # the sample passes of an iteration as one launch, where the library serves the model and the mode
        mode = SAMPLED_MODE.get(self.gradient_mode)
        self.batched_sample_pass = bool(batched_sample_pass) and mode is not None and dm.smooth_batch_supported(mode)
        if self.batched_sample_pass:
            self._seeds = seed_bits([p.device_rng_seed for p in ps], device)    # uploaded once
        self._std_u = None

    # ---- results, per problem (x_trj, u_trj, cost: StackedResults) ---------------------------------
    @property
    def x_trj_best(self):
        return [pr.x_trj_best for pr in self.problems]

    @property
    def u_trj_best(self):
        return [pr.u_trj_best for pr in self.problems]

    @property
    def cost_best(self):
        return np.array([pr.cost_best for pr in self.problems])

    def __getattr__(self, name):
        # x_trj_list, u_trj_list, cost_all_list, cost_Qu_list, ...: one list per problem
        if name in ("x_trj_list", "u_trj_list", "cost_all_list") + tuple("cost_%s_list" % t for t in COST_TERMS):
            return [getattr(pr, name) for pr in self.problems]
        raise AttributeError(name)

    # ---- one descent of all problems ----------------------------------------------------------------
    def _std_u_schedule(self, it0, D):
        """(D, B, m): every problem's std_u at the iterations it0 .. it0 + D - 1, evaluated on the host."""
        return np.array([[np.broadcast_to(np.asarray(p.sampling(p.std_u_initial, it0 + d), float), (self.dim_u,))
                          for p in self.params_list] for d in range(D)], dtype=float)

    def _linearise(self, X, U, it, AT, BT, CT, sinfo, d=0):
        """The B sample passes: ONE launch over B x T rows (`batched_sample_pass`; `self._std_u[d]` holds the problems'
        std_u of this descent), or B calls of the single-problem entry back to back on the stream.  Either way problem
        b's pass takes its seed and the iteration counter -- the draws of its single twin."""
        mode = SAMPLED_MODE.get(self.gradient_mode)
        # (asked again per descent: IRS_UG is read per call, and IRS_UG=0 sends the planar hand to the general kernel)
        if self.batched_sample_pass and self._dm.smooth_batch_supported(mode):
            self._dm.smooth_rng_batch(mode, X, U, self.num_samples, self._std_u[d], self._seeds, it,
                                      out=dict(sums=self._sums, At=AT, Bt=BT, ct=CT, info=sinfo))
            return
        for b, p in enumerate(self.params_list):
            if self.gradient_mode == "exact":
                At, Bt, ct = self._dm.exact_linearize(X[b], U[b])
                At, Bt, ct = decouple_AB_dev(At, Bt, ct, X[b], U[b], self._idx, self.dim_x, self.dim_u)
                AT[b].copy_(At)
                BT[b].copy_(Bt)
                CT[b].copy_(ct)
                sinfo[b].zero_()
                continue
            std_u = np.broadcast_to(np.asarray(p.sampling(p.std_u_initial, it), float), (self.dim_u,))
            out = dict(sums=self._sums[b], At=AT[b], Bt=BT[b], ct=CT[b], info=sinfo[b])
            self._dm.smooth_rng(mode, X[b], U[b], self.num_samples, None, std_u, int(p.device_rng_seed), it, out=out)

    def iterate(self, max_iterations):
        """The quiet loop of `IrsLqrQuasistatic.iterate` over all problems: every descent is the B sample passes (one
        launch, or B with `batched_sample_pass=False`), one bound-rows launch and ONE batched descent that writes
        straight into its slot of the history; nothing waits for the device until the one read-back at the end, where
        each problem's bookkeeping (history lists, five cost terms, best-so-far) is replayed as the single class does.
        A problem whose smoothing solve or QP failed does not raise: it stops adopting at that descent, `status[b]`
        holds the message the single class raises, and the others finish.  Returns (x_trj (B,T+1,n), u_trj (B,T,m), cost (B))."""
        if dist_util.rank_world()[1] != 1:
            raise NotImplementedError("the batch runs on one GPU")
        B, T, n, m = self.B, self.T, self.dim_x, self.dim_u
        dm = self._dm
        _, _, qp_max_iter, qp_eps = qp_settings(self.params_list[0])
        it0 = self.current_iter
        D = max(1, max_iterations - it0 + 2)                 # the single loop: descents until current_iter > max
        X = dev.to_dev(self.x_trj)
        U = dev.to_dev(self.u_trj)
        device = X.device
        x0 = X[:, 0, :].contiguous()
        xs = torch.empty((D, B, T + 1, n), dtype=dev.F64, device=device)
        us = torch.empty((D, B, T, m), dtype=dev.F64, device=device)
        costs = torch.empty((D, B), dtype=dev.F64, device=device)
        infos = torch.empty((D, B, 3), dtype=torch.int32, device=device)
        sinfo = torch.empty((D, B, T), dtype=torch.int32, device=device)
        AT = torch.empty((B, T, n, n), dtype=dev.F64, device=device)
        BT = torch.empty((B, T, n, m), dtype=dev.F64, device=device)
        CT = torch.empty((B, T, n), dtype=dev.F64, device=device)
        if self.gradient_mode != "exact":
            P = dm.sums_len(SAMPLED_MODE[self.gradient_mode])
            self._sums = torch.empty((B, T, P), dtype=dev.F64, device=device)
        if self._act is None:
            # the first tail's active set of every problem, handed from one descent to the next (zeros: cold start)
            self._act = torch.zeros((B, T, m), dtype=dev.F64, device=device)
        if self._rows is None:
            self._rows = (torch.empty((B, T, m), dtype=dev.F64, device=device),
                          torch.empty((B, T, m), dtype=dev.F64, device=device))
            if self._kind == "rel":                          # bounds on u_t - u_{t-1}: the offsets, once
                dm.quasistatic_bound_rows_batch(X, self._idx32, self._offsets, rel=True, out=self._rows)
        if self.batched_sample_pass:                         # the std_u schedule of all D descents: one upload
            self._std_u = dev.to_dev(self._std_u_schedule(it0, D))
        it = it0
        for d in range(D):
            self._linearise(X, U, it, AT, BT, CT, sinfo[d], d)
            if self._kind != "rel":
                dm.quasistatic_bound_rows_batch(X, self._idx32, self._offsets, rel=False, out=self._rows)
            rows = dict(du_lo=self._rows[0], du_hi=self._rows[1]) if self._kind == "rel" else dict(
                u_lo=self._rows[0], u_hi=self._rows[1])
            dm.quasistatic_box_descent_batch(AT, BT, CT, self._Q, self._Qd, self._R, self._xd, x0,
                                             max_iter=qp_max_iter, eps=qp_eps,
                                             out=dict(x_new=xs[d], u_new=us[d], cost=costs[d], info=infos[d]),
                                             act=self._act, **rows)
            X, U = xs[d], us[d]
            it += 1
        xs_h, us_h = xs.cpu().numpy(), us.cpu().numpy()                     # the one read-back
        infos_h, sbad = infos.cpu().numpy(), (sinfo != 0).any(dim=2).cpu().numpy()
        self._last = dict(At=AT, Bt=BT, ct=CT, info=infos[D - 1], cost=costs)
        for b, pr in enumerate(self.problems):
            if self.status[b] is not None:
                continue                                     # failed in an earlier call: frozen at its last adopted state
            pr.current_iter = it0
            failures = [descent_failure(infos_h[i, b], sbad[i, b]) for i in range(D)]
            self.status[b] = pr._replay(xs_h[:, b], us_h[:, b], failures, max_iterations)
        self.current_iter = it0 + D - 1
        return self.x_trj, self.u_trj, self.cost
