"""B iRS-LQR problems of one analytic system side by side: `IrsLqrBatch`.

A descent of `IrsLqrZeroOrder` / `IrsLqrFirstOrder` / `IrsLqrExact` is one wave in one launch, and at the sizes the
example scripts use its sample pass is bound by launch latency.  Users of these models run many initial guesses, start
states or goals of the same system anyway (multi-start, a sweep over x0, a value-function grid); as separate objects
those descents queue on a single wave.  Here an iteration of all B problems is

    one linearisation    `irs_smooth_rng_general_batch` (the sample-pass kernel over B x T rows), or for "exact" one
                         `irs_exact_linearize` on the stacked (B T) nominal points,
    one descent launch   `irs_tvlqr_descent_batch` (the descent kernel with a problem index, one workgroup each),
    one plan-test launch `irs_tvlqr_plan_within_bounds_batch`, when any problem has a finite bound,
    (bounded=True)       one bounded-descent launch `irs_tvlqr_box_descent_batch` behind the plan test's flags: the
                         ADMM kernel of the single classes with a problem index, one workgroup each; a problem whose
                         plan stays inside its box, or that has stopped, returns at once,
    and the adoption     a masked copy,

enqueued back to back without a device synchronisation; the histories are read back once at the end.

The problems share the system, `T`, `Q`, `Qd`, `R`, and the sampling's `num_samples` and `power`; they may differ in
`x0`, `xd_trj`, `u_trj_initial`, the bounds, and their `GaussianSmoothing`'s seed, `std_x` and `std_u`.

bounded=False (the default): descents are the unbounded ones (Riccati): a problem whose plan leaves its box at some
descent -- a bound that is genuinely active -- stops adopting there and `status[b]` says how to run it.
bounded=True: that problem's descent is the single class's bounded one (T warm-started tail QPs by ADMM, fixed penalty;
`qp_rho`, `qp_max_iter`, `qp_eps` shared by the problems), it keeps `status[b] is None` and runs to the end; it stops
only where a bounded QP is not solved, with the single class's message.  Either way a problem whose Riccati pass or
smoothing solve failed stops with the message the single class raises, and the other problems finish.
"""
import numpy as np
import torch

from . import device as dev
from . import distributed as dist_util
from ._lib import SMOOTH_FIRST_ORDER, SMOOTH_ZERO_ORDER_AB
from .batch_common import StackedResults, seed_bits
from .irs_lqr import HORIZON_BEYOND_LIMIT, RICCATI_FAILED, SMOOTHING_FAILED, IrsLqr
from .sampling import GaussianSmoothing
from .torch_system import TorchDynamicalSystem

ORDERS = {"zero_order": (SMOOTH_ZERO_ORDER_AB, "IrsLqrZeroOrder"), "first_order": (SMOOTH_FIRST_ORDER, "IrsLqrFirstOrder"),
          "exact": (None, "IrsLqrExact")}


def _bound_active(single):
    return ("a box bound is active at this descent: the batch runs unbounded (Riccati) descents only; run this problem "
            "with %s, whose bounded descent (irs_tvlqr_box_descent) enforces it" % single)


# the bounded QPs' ADMM settings, shared by the problems of a launch: the field and the single class's default
QP_SETTINGS = (("qp_rho", 10.0), ("qp_max_iter", 5000), ("qp_eps", 1e-8))
QP_RELAX = 1.6


class IrsLqrBatch(StackedResults):
    def __init__(self, system, params_list, order, sampling_list=None, bounded=False):
        ps = list(params_list)
        if not ps:
            raise ValueError("params_list is empty")
        if order not in ORDERS:
            raise ValueError("order %r: one of %s" % (order, sorted(ORDERS)))
        # ---- what the batch serves (no GPU is touched before all of this has passed) ----
        if isinstance(system, TorchDynamicalSystem):
            raise NotImplementedError("a TorchDynamicalSystem has no device functor: the batched launches need a compiled "
                                      "analytic model")
        for flag in ("qp_adaptive_rho", "qp_lazy_bounds"):
            if any(bool(getattr(p, flag, False)) for p in ps):
                raise NotImplementedError("params.%s belongs to the bounded descent; the batch runs unbounded descents" % flag)
        if dist_util.rank_world()[1] != 1:
            raise NotImplementedError("the batch runs on one GPU (world > 1)")
        # ---- what the one launch shares ----
        p0 = ps[0]
        T = np.asarray(p0.u_trj_initial).shape[0]
        for b, p in enumerate(ps[1:], 1):
            if np.asarray(p.u_trj_initial).shape[0] != T:
                raise ValueError("params_list[%d]: T = %d differs from params_list[0]'s %d"
                                 % (b, np.asarray(p.u_trj_initial).shape[0], T))
            for field in ("Q", "Qd", "R"):
                if not np.array_equal(np.asarray(getattr(p, field), float), np.asarray(getattr(p0, field), float)):
                    raise ValueError("params_list[%d].%s differs from params_list[0].%s" % (b, field, field))
        self.bounded = bool(bounded)
        self._qp = {field: getattr(p0, field, default) for field, default in QP_SETTINGS}
        if self.bounded:
            for b, p in enumerate(ps[1:], 1):
                for field, default in QP_SETTINGS:
                    if getattr(p, field, default) != self._qp[field]:
                        raise ValueError("params_list[%d].%s differs from params_list[0].%s: the bounded descents of a "
                                         "launch share their ADMM settings" % (b, field, field))
        self.mode, self._single = ORDERS[order]
        if self.mode is None:
            if sampling_list is not None:
                raise ValueError("order 'exact' takes no sampling_list")
            smps = None
        else:
            smps = list(sampling_list) if sampling_list is not None else []
            if len(smps) != len(ps):
                raise ValueError("sampling_list: one GaussianSmoothing per problem (%d for %d problems)" % (len(smps), len(ps)))
            for b, s in enumerate(smps):
                if not isinstance(s, GaussianSmoothing) or not getattr(s, "on_device", True):
                    raise NotImplementedError("sampling_list[%d] is drawn on the host: the batch needs device-drawn samples "
                                              "(a GaussianSmoothing); host draws would serialise the B sample passes" % b)
                for field in ("num_samples", "power"):
                    if getattr(s, field) != getattr(smps[0], field):
                        raise ValueError("sampling_list[%d].%s differs from sampling_list[0].%s" % (b, field, field))

        self.system, self.params_list, self.order, self.sampling_list = system, ps, order, smps
        # one problem's data, initial rollout, cost and history lists: the single class's own
        self.problems = [IrsLqr(system, p) for p in ps]
        for pr in self.problems:
            pr.verbose = False
            if pr.T != T or pr.x_trj.shape != (T + 1, system.dim_x):
                raise ValueError("the problems' trajectories differ in shape")
        self._dm = self.problems[0]._dm
        self.B, self.T, self.dim_x, self.dim_u = len(ps), T, system.dim_x, system.dim_u
        if self.mode is not None and not self._dm.smooth_general_batch_supported(self.mode):
            raise NotImplementedError("the batched sample pass does not serve this model in order %r" % (order,))
        self.status = [None] * self.B
        self.iter = 1
        self.verbose = False
        pr0 = self.problems[0]
        self._Q, self._Qd, self._R = pr0._Q, pr0._Qd, pr0._R
        self._xd = torch.stack([pr._xd for pr in self.problems]).contiguous()
        # per-problem boxes, +-inf where a problem has no bound; tested only if some entry is finite
        boxes = []
        for pr in self.problems:
            pr._box_bounds()
            boxes.append(pr._box_host)
        self._box = None
        if any(np.isfinite(v).any() for box in boxes for v in box):
            if self.bounded and not self._dm.box_descent_supported(T):
                raise NotImplementedError(HORIZON_BEYOND_LIMIT % (T, self._dm.box_horizon_limit()))
            self._box = tuple(dev.to_dev(np.stack([box[i] for box in boxes])) for i in range(4))
        if smps is not None:
            self._seeds = seed_bits([s.seed for s in smps], self._Q.device)      # uploaded once

    # ---- results, per problem (x_trj, u_trj, cost: StackedResults) ---------------------------------
    @property
    def x_trj_lst(self):
        return [pr.x_trj_lst for pr in self.problems]

    @property
    def u_trj_lst(self):
        return [pr.u_trj_lst for pr in self.problems]

    @property
    def cost_lst(self):
        return [pr.cost_lst for pr in self.problems]

    def _linearise(self, X, U, d, it, o):
        """One linearisation of all problems around (X, U) into o = dict(At, Bt, ct, info[, sums])."""
        B, T, n, m = self.B, self.T, self.dim_x, self.dim_u
        if self.mode is None:
            # irs_exact_linearize reads rows of nominal points: B problems are one call on the stacked (B T) points
            At, Bt, ct = self._dm.exact_linearize(X[:, :T].reshape(B * T, n), U.reshape(B * T, m))
            o["At"], o["Bt"], o["ct"] = At.view(B, T, n, n), Bt.view(B, T, n, m), ct.view(B, T, n)
            return
        self._dm.smooth_rng_general_batch(self.mode, X, U, self.sampling_list[0].num_samples, self._std_x[d],
                                          self._std_u[d], self._seeds, it, out=o)

    def iterate(self, max_iterations):
        """`IrsLqr.iterate` over all problems: max_iterations - iter + 2 descents, the last one logged but not
        adopted, every descent four enqueues (see the module text) and nothing waiting for the device until the one
        read-back at the end, where each problem's bookkeeping (`x_trj_lst`, `u_trj_lst`, `cost_lst`, `x_trj`, `u_trj`,
        `cost`) is replayed as the single class does it.  A problem that stops (module text) keeps the trajectory it had
        adopted; `status[b]` holds the reason.  Returns (x_trj (B,T+1,n), u_trj (B,T,m), cost (B))."""
        B, T, n, m = self.B, self.T, self.dim_x, self.dim_u
        dm = self._dm
        it0 = self.iter
        D = max_iterations - it0 + 2
        if D <= 0:
            return self.x_trj, self.u_trj, self.cost
        X = dev.to_dev(self.x_trj)
        U = dev.to_dev(self.u_trj)
        device = X.device
        x0 = X[:, 0, :].contiguous()
        alive = torch.as_tensor([s is None for s in self.status], device=device)
        xs = torch.empty((D, B, T + 1, n), dtype=dev.F64, device=device)
        us = torch.empty((D, B, T, m), dtype=dev.F64, device=device)
        costs = torch.empty((D, B), dtype=dev.F64, device=device)
        dinfo = torch.empty((D, B), dtype=torch.int32, device=device)
        flags = torch.zeros((D, B), dtype=torch.int32, device=device)
        sinfo = torch.zeros((D, B, T), dtype=torch.int32, device=device)
        bounded = self.bounded and self._box is not None     # no finite bound anywhere: nothing more than the Riccati loop
        binfo = torch.zeros((D, B, 3), dtype=torch.int32, device=device)       # rows a bounded descent did not write: 0
        K = torch.empty((B, T, m, n), dtype=dev.F64, device=device)
        k = torch.empty((B, T, m), dtype=dev.F64, device=device)
        lin = {}
        if self.mode is not None:
            lin = dm._tv_alloc(dm._tv_shapes((B, T), self.mode), device)
            stds = [[s.stds(it0 + d) for s in self.sampling_list] for d in range(D)]       # the schedule: one upload
            self._std_x = dev.to_dev(np.array([[np.broadcast_to(sx, (n,)) for sx, _ in row] for row in stds], float))
            self._std_u = dev.to_dev(np.array([[np.broadcast_to(su, (m,)) for _, su in row] for row in stds], float))
        for d in range(D):
            if self.mode is not None:
                lin["info"] = sinfo[d]
            self._linearise(X, U, d, it0 + d, lin)
            dm.tvlqr_descent_batch(lin["At"], lin["Bt"], lin["ct"], self._Q, self._Qd, self._R, self._xd, x0, alpha_R=0.5,
                                   out=dict(K=K, k=k, x_new=xs[d], u_new=us[d], cost=costs[d], info=dinfo[d]))
            if self._box is not None:
                dm.plan_within_bounds_batch(lin["At"], lin["Bt"], lin["ct"], K, k, xs[d], *self._box, flag=flags[d])
            if not bounded and d + 1 == D:
                break                                        # the last descent is logged, not adopted
            # go: alive, and this descent's Riccati pass and smoothing solve succeeded
            go = alive & (dinfo[d] == 0) & ~(sinfo[d] != 0).any(dim=1)
            solved = flags[d] == 0
            if bounded:
                # the bounded descents of the problems whose plan leaves its box, behind their flags: they overwrite
                # this descent's rows of the histories; a stopped problem's workgroup returns at once
                dm.tvlqr_box_descent_batch(lin["At"], lin["Bt"], lin["ct"], self._Q, self._Qd, self._R, self._xd, x0,
                                           *self._box, alpha_R=0.5, rho=self._qp["qp_rho"], relax=QP_RELAX,
                                           max_iter=self._qp["qp_max_iter"], eps=self._qp["qp_eps"],
                                           run_flag=flags[d] * go.to(torch.int32),
                                           out=dict(x_new=xs[d], u_new=us[d], cost=costs[d], info=binfo[d]))
                solved = solved | ((binfo[d, :, 0] == 0) & (binfo[d, :, 2] == 0))
            if d + 1 < D:
                # adoption: a problem goes on from its new trajectory unless this descent, or an earlier one, stopped it
                alive = go & solved
                keep = alive[:, None, None]
                X, U = torch.where(keep, xs[d], X), torch.where(keep, us[d], U)
        xs_h, us_h, cs_h = xs.cpu().numpy(), us.cpu().numpy(), costs.cpu().numpy()        # the one read-back
        dinfo_h, flags_h, sbad_h = dinfo.cpu().numpy(), flags.cpu().numpy(), (sinfo != 0).any(dim=2).cpu().numpy()
        binfo_h = binfo.cpu().numpy()
        self._last = dict(At=lin["At"], Bt=lin["Bt"], ct=lin["ct"], K=K, k=k, info=dinfo[D - 1], flag=flags[D - 1],
                          box_info=binfo[D - 1])
        for b, pr in enumerate(self.problems):
            if self.status[b] is not None:
                continue                                     # stopped in an earlier call: frozen at its last adopted state
            pr.iter = it0
            failures = [None] * D
            for i in range(D):
                if dinfo_h[i, b] != 0:
                    failures[i] = RICCATI_FAILED
                elif sbad_h[i, b]:
                    failures[i] = SMOOTHING_FAILED
                elif flags_h[i, b] != 0 and not bounded:
                    failures[i] = _bound_active(self._single)
                elif flags_h[i, b] != 0 and (binfo_h[i, b, 0] != 0 or binfo_h[i, b, 2] != 0):
                    failures[i] = RICCATI_FAILED             # the single class's message for an unsolved bounded QP
            self.status[b] = pr._replay(xs_h[:, b], us_h[:, b], cs_h[:, b], failures, max_iterations)
        self.iter = it0 + D - 1
        return self.x_trj, self.u_trj, self.cost
