"""Host mirror of the reference's quasistatic cross-entropy-method baseline
(irs_lqr/cem_quasistatic.py:10-258): `CemQuasistaticParameters`,
`CrossEntropyMethodQuasistatic(q_dynamics, params)` with rollout / eval_cost / calc_Q_cost /
local_descent / iterate and the reference's attribute names (quasistatic_base.py lists them) plus
`n_elite, batch_size, initial_std, std_trj`.

`local_descent` draws the candidates on the host exactly as the reference does
(`np.random.normal(u_trj, std_trj, (batch_size, T, m))`, :188-189 -- identical seeds give identical
candidates); the B contact rollouts, their quasistatic costs, the elite selection and the refit run
on the GPU (csrc/cem.hip).  The reference's parameter class declares `xd_trj` but its solver reads
`params.x_trj_d` (:62, a latent AttributeError there): either attribute is accepted here.

`params.device_seed` (optional, not a reference field; None = the host draw above): an int makes the
method device resident, as in cem.py of this package -- candidates drawn inside the rollout kernel from
the stream keyed by (device_seed, self.current_iter), elites regenerated from their indices, and
`iterate` ONE library call (irs_cem_iterate) with one read-back.
"""
import time

import numpy as np

from .cem import CemDescent
from .quasistatic_base import QuasistaticOptimizerBase


class CemQuasistaticParameters:
    """irs_lqr/cem_quasistatic.py:10-37 (same fields)."""

    def __init__(self):
        for name in ("Q_dict", "Qd_dict", "R_dict", "x0", "xd_trj", "u_trj_0", "n_elite", "batch_size",
                     "initial_std", "T"):
            setattr(self, name, None)       # initial_std: (dim_u,) array of initial stds
        self.publish_every_iteration = True
        self.device_seed = None     # int: draw the candidates on the device (not a reference field)


class CrossEntropyMethodQuasistatic(CemDescent, QuasistaticOptimizerBase):
    def __init__(self, q_dynamics, params):
        goal = getattr(params, "x_trj_d", None)
        self._setup(q_dynamics, params, params.xd_trj if goal is None else goal)
        self.n_elite, self.batch_size, self.initial_std = params.n_elite, params.batch_size, params.initial_std
        self.std_trj = np.tile(self.initial_std, (self.T, 1))
        self.device_seed = getattr(params, "device_seed", None)

    def local_descent(self, x_trj, u_trj):
        """cem_quasistatic.py:168-211: sample, price, keep the elites, refit mean and std."""
        return self._cem_descent(u_trj, self.current_iter, Qd=self._Qd)

    def iterate(self, max_iterations):
        """QuasistaticOptimizerBase.iterate; with device_seed set, through ONE irs_cem_iterate call: every descent
        enqueued back to back, one read-back, then the loop's bookkeeping (the five-term log, best-so-far, the last
        descent logged but not adopted)."""
        if self.device_seed is None:
            return super().iterate(max_iterations)
        k, h = self._cem_iterate_histories(max_iterations, self.current_iter, Qd=self._Qd)
        for i in range(k):
            if self.verbose:
                print("Iter {:02d}, cost: {:0.4f}. time: {:0.2f}.".format(self.current_iter, self.cost,
                                                                        time.time() - self.start_time))
            x_new, u_new = h["x_hist"][i], h["u_hist"][i]
            cost_new = self._log(x_new, u_new)
            self.std_trj = h["std_hist"][i]
            if self.publish_every_iteration:
                self.q_dynamics.publish_trajectory(x_new)
            if i == k - 1:
                return self.x_trj, self.u_trj, self.cost
            self.cost, self.x_trj, self.u_trj = cost_new, x_new, u_new
            self.current_iter += 1

    # outer loop: QuasistaticOptimizerBase.iterate
    def _start(self):
        return None

    def _descend(self, state):
        return self.local_descent(self.x_trj, self.u_trj) + (None,)
