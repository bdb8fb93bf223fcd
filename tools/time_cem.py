#!/usr/bin/env python3
"""Times one CEM iteration (ms) four ways, at the sizes the project compares at:

    python tools/time_cem.py [--reps 5] [--host-reps 3] [--B 50000] [--T 80]

  (a) host_draw   the public class with device_seed = None: np.random.normal on the host, the f64 upload, three kernels,
                  the read-back (CrossEntropyMethod[Quasistatic].local_descent)
  (b) supplied    the same kernels on a candidate tensor that is already on the device
  (c) drawn       the drawn kernels (candidates generated in the rollout lane, elites regenerated in the refit)
  (d) iterate     irs_cem_iterate: all descents in one call, per descent

on the pendulum (T = 80, B = 5e4) and box pivoting with the exact step QP (T = 80, B = 5e4, n_elite = B / 20).  One
process, device events around every window (a window ends with the iteration's last kernel or read-back), one warm-up
of every shape excluded.  Prints one JSON line; asserts nothing."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import irs_mpc_amd as amd  # noqa: E402
from irs_mpc_amd import device as dev  # noqa: E402


def timed(fn, reps):
    """ms per call of fn over `reps` calls after one warm-up, by device events."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def pendulum(T, B):
    p = amd.CemParameters()
    p.Q, p.Qd, p.R = np.diag([1., 1.]), np.diag([20., 20.]), np.diag([1.])
    p.x0, p.xd_trj = np.array([0., 0.]), np.tile(np.array([np.pi, 0.]), (T + 1, 1))
    p.u_trj_initial, p.initial_std = np.tile(np.array([0.1]), (T, 1)), np.array([1.0])
    p.batch_size, p.n_elite = B, B // 20
    sol = amd.CrossEntropyMethod(amd.PendulumDynamics(0.05), p)
    return sol, sol._dm, (sol._x0, sol._Q, None, sol._R, sol._xd), p.u_trj_initial, False


def box_pivoting(T, B):
    from examples.run_quasistatic import box_problem
    sd, x0, u0, Q_dict, Qd_dict, R_dict, xd = box_problem(T)
    p = amd.CemQuasistaticParameters()
    p.Q_dict, p.Qd_dict, p.R_dict = Q_dict, Qd_dict, R_dict
    p.x0, p.xd_trj, p.u_trj_0, p.T = x0, xd, u0, T
    p.n_elite, p.batch_size, p.initial_std = B // 20, B, 0.2 * np.ones(2)
    p.publish_every_iteration = False
    sol = amd.CrossEntropyMethodQuasistatic(sd, p)
    return sol, sol._dm, (sol._x0, sol._Q, sol._Qd, sol._R, sol._xd), u0, True


def measure(make, T, B, reps, host_reps):
    sol, dm, (x0, Q, Qd, R, xd), u0, qs = make(T, B)
    sol.verbose = False
    n_elite, seed = sol.n_elite, 1
    mean, std = dev.to_dev(np.asarray(u0, float)), dev.to_dev(np.asarray(sol.std_trj, float))
    cand = dm.cem_candidates(mean, std, B, seed, 1)

    def price(c):
        return dm.cem_rollout_costs_quasistatic(c, x0, Q, Qd, R, xd) if qs else dm.cem_rollout_costs(c, x0, Q, R, xd)

    def price_drawn():
        if qs:
            return dm.cem_rollout_costs_quasistatic_drawn(mean, std, B, seed, 1, x0, Q, Qd, R, xd)
        return dm.cem_rollout_costs_drawn(mean, std, B, seed, 1, x0, Q, R, xd)

    def host_draw():
        np.random.seed(0)
        sol.std_trj = np.tile(sol.initial_std, (T, 1))
        sol.local_descent(sol.x_trj, sol.u_trj)

    def supplied():
        _, u_new, _ = dm.cem_refit(cand, price(cand), n_elite)
        dm.rollout_cost(x0, u_new, Q, R, xd)

    def drawn():
        _, u_new, _ = dm.cem_refit_drawn(mean, std, seed, 1, price_drawn(), n_elite)
        dm.rollout_cost(x0, u_new, Q, R, xd)

    def iterate():
        o = dm.cem_iterate(mean, std, x0, Q, Qd, R, xd, B, n_elite, reps, seed, 1, quasistatic=qs)
        o["cost_hist"].cpu()                 # the one read-back

    out = {"T": T, "B": B, "n_elite": n_elite,
           "host_draw_ms": timed(host_draw, host_reps), "supplied_ms": timed(supplied, reps),
           "drawn_ms": timed(drawn, reps), "iterate_ms_per_descent": timed(iterate, 1) / reps,
           "rollout_supplied_ms": timed(lambda: price(cand), reps), "rollout_drawn_ms": timed(price_drawn, reps)}
    return {k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--B", type=int, default=50000)
    ap.add_argument("--T", type=int, default=80)
    ap.add_argument("--only", choices=["pendulum", "box_pivoting"], default=None)
    a = ap.parse_args()
    dev.require_gpu()
    res = {"tool": "time_cem", "device": torch.cuda.get_device_name(0), "reps": a.reps, "host_reps": a.host_reps}
    for name, make in (("pendulum", pendulum), ("box_pivoting", box_pivoting)):
        if a.only in (None, name):
            res[name] = measure(make, a.T, a.B, a.reps, a.host_reps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
