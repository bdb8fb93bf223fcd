#!/usr/bin/env python3
"""Times one CEM descent (ms) of a system written as a torch callable beside its compiled twin:

    python tools/time_cem_values.py [--reps 5] [--T 30] [--B 5000 50000]

on the pendulum problem of the CEM tests (n_elite = B / 20), candidates drawn on the device, per batch size

  torch      TorchPendulum: T + 1 stage launches (csrc/cem.hip, cem_values_stage_kernel) with the callable between them
  compiled   PendulumDynamics: one launch of cem_rollout_kernel (irs_cem_rollout_costs[_drawn])
  copy       the stages with the callable replaced by a copy of x: the launches the design adds, without any dynamics

each as `rollout_ms` (the B candidate rollouts alone, drawn; `rollout_supplied_ms` on a (B,T,m) tensor already on the
device) and `descent_ms` (rollouts + selection + refit + the mean's rollout: local_descent without its read-back).  One
process, device events around every window, one warm-up of every shape excluded.  Prints one JSON line; asserts nothing."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import irs_mpc_amd as amd  # noqa: E402
from irs_mpc_amd import device as dev  # noqa: E402
from examples.torch_systems import TorchPendulum  # noqa: E402


class CopyPlant(amd.TorchDynamicalSystem):
    """x+ = x, by one device copy: what a stage-by-stage rollout costs before any dynamics."""

    def __init__(self):
        super().__init__()
        self.dim_x, self.dim_u = 2, 1

    def dynamics_batch_torch(self, x, u):
        return x.clone()


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


def measure(system, T, B, reps):
    dm, n_elite, seed = system.dm(), B // 20, 1
    x0, Q, R = dev.to_dev(np.zeros(2)), dev.to_dev(np.eye(2)), dev.to_dev(np.eye(1))
    xd = dev.to_dev(np.tile(np.array([np.pi, 0.]), (T + 1, 1)))
    mean, std = dev.to_dev(np.full((T, 1), 0.1)), dev.to_dev(np.ones((T, 1)))
    cand = dm.cem_candidates(mean, std, B, seed, 1)

    def rollout():
        return dm.cem_rollout_costs_drawn(mean, std, B, seed, 1, x0, Q, R, xd)

    def descent():
        _, u_new, _ = dm.cem_refit_drawn(mean, std, seed, 1, rollout(), n_elite)
        dm.rollout_cost(x0, u_new, Q, R, xd)

    out = {"rollout_ms": timed(rollout, reps), "descent_ms": timed(descent, reps),
           "rollout_supplied_ms": timed(lambda: dm.cem_rollout_costs(cand, x0, Q, R, xd), reps)}
    return {k: round(v, 4) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--T", type=int, default=30)
    ap.add_argument("--B", type=int, nargs="+", default=[5000, 50000])
    a = ap.parse_args()
    dev.require_gpu()
    res = {"tool": "time_cem_values", "device": torch.cuda.get_device_name(0), "reps": a.reps, "T": a.T}
    for B in a.B:
        res["B=%d" % B] = {name: measure(system, a.T, B, a.reps)
                           for name, system in (("torch", TorchPendulum(0.05)), ("compiled", amd.PendulumDynamics(0.05)),
                                                ("copy", CopyPlant()))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
