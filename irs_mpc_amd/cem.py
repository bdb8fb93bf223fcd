"""Host mirror of the reference's cross-entropy-method baseline (irs_lqr/cem.py:7-216):
`CemParameters`, `CrossEntropyMethod(system, params)` with rollout / evaluate_cost / local_descent /
iterate and the attributes x_trj, u_trj, cost, std_trj, iter, x_trj_lst, u_trj_lst, cost_lst.

`local_descent` draws the candidates on the host exactly as the reference does
(`np.random.normal(u_trj, std_trj, (batch_size, T, m))`, cem.py:159-161 -- identical seeds give
identical candidates); the B rollouts + costs, the elite selection and the refit run on the GPU
(csrc/cem.hip).  Construction-time validation is IrsLqr's (same checks, same messages:
cem.py:77-106 duplicates irs_lqr.py:73-103).

`params.device_seed` (optional, not a reference field; None = the host draw above): an int makes the
method device resident -- the candidates are a counter-based stream keyed by (device_seed, self.iter)
and drawn inside the rollout kernel, the refit regenerates the elites from their indices, no (B,T,m)
tensor exists on either side; `iterate` is then ONE library call (irs_cem_iterate) and one read-back.
"""
import time

import numpy as np

from . import device as dev
from .irs_lqr import IrsLqr


class CemParameters:
    """irs_lqr/cem.py:7-32 (same fields)."""

    def __init__(self):
        for name in ("Q", "Qd", "R", "x0", "xd_trj", "u_trj_initial", "n_elite", "batch_size", "elite_frac",
                     "initial_std"):
            setattr(self, name, None)
        self.device_seed = None     # int: draw the candidates on the device (not a reference field)


class CemDescent:
    """What CrossEntropyMethod and CrossEntropyMethodQuasistatic share: one descent and, with device_seed, the head
    of `iterate`.  The host class has batch_size, n_elite, T, dim_u, std_trj, device_seed, _dm and the device copies
    _x0, _Q, _R, _xd; `it` is its iteration counter, Qd (a device tensor) asks for the quasistatic cost."""

    def _cem_descent(self, u_trj, it, Qd=None):
        """Candidate source -> costs -> elites and refit -> the mean's rollout -> std_trj; returns (x_mean, u_mean).
        The source is the reference's host draw or, with device_seed, the stream of (device_seed, it): no candidate
        tensor.  cost_array and elite_idx stay behind as attributes."""
        if self.device_seed is None:
            src = dev.CemSource.supplied(dev.to_dev(np.random.normal(u_trj, self.std_trj,
                                                                     (self.batch_size, self.T, self.dim_u))))
        else:
            src = dev.CemSource.drawn(dev.to_dev(np.asarray(u_trj, float)), dev.to_dev(np.asarray(self.std_trj, float)),
                                      self.batch_size, self.device_seed, it)
        self.cost_array = self._dm.cem_costs(src, self._x0, self._Q, self._R, self._xd, Qd=Qd)
        self.elite_idx, u_mean, u_std = self._dm.cem_refit_from(src, self.cost_array, self.n_elite)
        x_mean, _ = self._dm.rollout_cost(self._x0, u_mean, self._Q, self._R, self._xd)
        self.std_trj = u_std.cpu().numpy()
        return x_mean.cpu().numpy(), u_mean.cpu().numpy()

    def _cem_iterate_histories(self, max_iterations, it, Qd=None):
        """The descents the host loop would run from iteration `it`, through ONE cem_iterate call and one read-back:
        (their number k, the histories of DeviceModel.cem_iterate as NumPy arrays)."""
        k = max(1, max_iterations - it + 2)
        o = self._dm.cem_iterate(dev.to_dev(np.asarray(self.u_trj, float)), dev.to_dev(np.asarray(self.std_trj, float)),
                                 self._x0, self._Q, Qd, self._R, self._xd, self.batch_size, self.n_elite, k,
                                 self.device_seed, it, quasistatic=Qd is not None)
        return k, {key: v.cpu().numpy() for key, v in o.items()}


class CrossEntropyMethod(CemDescent):
    check_valid_system = IrsLqr.check_valid_system
    check_valid_params = IrsLqr.check_valid_params

    def __init__(self, system, params):
        self.system, self.params = system, params
        self.check_valid_system(system)
        self.check_valid_params(params, system)
        for name in ("Q", "Qd", "R", "x0", "xd_trj", "n_elite", "batch_size", "elite_frac", "initial_std"):
            setattr(self, name, getattr(params, name))
        self.device_seed = getattr(params, "device_seed", None)
        self.u_trj = params.u_trj_initial
        self.T, self.dim_x, self.dim_u = self.u_trj.shape[0], system.dim_x, system.dim_u

        self._dm = system.dm()
        self._Q, self._R, self._x0, self._xd = (dev.to_dev(np.asarray(a, float))
                                                for a in (self.Q, self.R, self.x0, self.xd_trj))
        self.x_trj = self.rollout(self.x0, self.u_trj)
        self.cost = self.evaluate_cost(self.x_trj, self.u_trj)
        self.std_trj = np.tile(self.initial_std, (self.T, 1))
        self.x_trj_lst, self.u_trj_lst, self.cost_lst = [self.x_trj], [self.u_trj], [self.cost]
        self.start_time = time.time()
        self.iter = 1
        self.verbose = True

    def rollout(self, x0, u_trj):
        """cem.py:108-122."""
        x_trj, _ = self._dm.rollout_cost(dev.to_dev(np.asarray(x0, float)), dev.to_dev(np.asarray(u_trj, float)),
                                         self._Q, self._R, self._xd)
        return x_trj.cpu().numpy()

    def evaluate_cost(self, x_trj, u_trj):
        """cem.py:124-140 (terminal term with Q, like IrsLqr)."""
        return float(dev.evaluate_cost(dev.to_dev(np.asarray(x_trj, float)), dev.to_dev(np.asarray(u_trj, float)),
                                       self._Q, self._R, self._xd).item())

    def local_descent(self, x_trj, u_trj):
        """cem.py:151-184: sample, price, keep the elites, refit mean and std."""
        return self._cem_descent(u_trj, self.iter)

    def _iterate_drawn(self, max_iterations):
        """The loop below through ONE irs_cem_iterate call: every descent enqueued back to back, one read-back."""
        k, h = self._cem_iterate_histories(max_iterations, self.iter)
        for i in range(k):
            x_new, u_new, cost_new = h["x_hist"][i], h["u_hist"][i], float(h["cost_hist"][i])
            if self.verbose:
                print("Iteration: {:02d}  ||  Current Cost: {:05f}  ||  Elapsed time: {:05f} ".format(
                    self.iter, cost_new, time.time() - self.start_time))
            for log, item in ((self.x_trj_lst, x_new), (self.u_trj_lst, u_new), (self.cost_lst, cost_new)):
                log.append(item)
            self.std_trj = h["std_hist"][i]
            if i == k - 1:
                return self.x_trj, self.u_trj, self.cost
            self.cost, self.x_trj, self.u_trj = cost_new, x_new, u_new
            self.iter += 1

    def iterate(self, max_iterations):
        """cem.py:186-216: max_iterations + 1 descents, the last one logged but not adopted."""
        if self.device_seed is not None:
            return self._iterate_drawn(max_iterations)
        while True:
            x_new, u_new = self.local_descent(self.x_trj, self.u_trj)
            cost_new = self.evaluate_cost(x_new, u_new)
            if self.verbose:
                print("Iteration: {:02d}  ||  Current Cost: {:05f}  ||  Elapsed time: {:05f} ".format(
                    self.iter, cost_new, time.time() - self.start_time))
            for log, item in ((self.x_trj_lst, x_new), (self.u_trj_lst, u_new), (self.cost_lst, cost_new)):
                log.append(item)
            if self.iter > max_iterations:
                return self.x_trj, self.u_trj, self.cost
            self.cost, self.x_trj, self.u_trj = cost_new, x_new, u_new
            self.iter += 1
