#!/usr/bin/env python3
"""Runs one of the reference's analytic examples on the GPU:

    python examples/run.py pendulum zero_order            # examples/pendulum/pendulum_zero_order.py
    python examples/run.py quadrotor first_order --device-rng
    python examples/run.py bicycle exact --csv bicycle_easy_exact.csv
    python examples/run.py pendulum cem
    python examples/run.py pendulum cem --device-rng

method = zero_order | first_order | exact | cem.  The sampling closure is the scripts'
(host NumPy RNG, `--seed`) unless --device-rng draws on the GPU.  Prints the cost history
(the reference saves it with np.savetxt, e.g. examples/quadrotor/quadrotor_cem.py:60-61).
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import irs_mpc_amd as amd  # noqa: E402
from examples.problems import PROBLEMS  # noqa: E402


def run_batch(sysd, params, sm, N, iters, a):
    """--batch B: B copies of the script's problem that differ in the initial guess (u_trj_initial + a fixed
    perturbation drawn with seed + b; problem 0 keeps the script's) and in the seed of their sample draws."""
    import copy
    plist, smps = [], []
    for b in range(a.batch):
        p = copy.copy(params)
        if b > 0:
            p.u_trj_initial = params.u_trj_initial + 0.01 * np.random.default_rng(a.seed + b).normal(
                size=params.u_trj_initial.shape)
        plist.append(p)
        smps.append(amd.GaussianSmoothing(sm["std_x"], sm["std_u"], N, power=sm["power"], seed=a.seed + b))
    # bounded=True: a problem whose box bound binds takes the bounded descent, as the single class does
    solver = amd.IrsLqrBatch(sysd, plist, a.method, None if a.method == "exact" else smps, bounded=True)
    t0 = time.time()
    solver.iterate(iters)
    for b in range(a.batch):
        print("problem %d final cost: %.6f  %s" % (b, solver.cost[b], solver.status[b] or "ok"))
    print("Elapsed time: " + str(time.time() - t0))
    if a.csv:
        np.savetxt(a.csv, np.array([c for c, s in zip(solver.cost_lst, solver.status) if s is None]).T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("system", choices=sorted(PROBLEMS))
    ap.add_argument("method", choices=["zero_order", "first_order", "exact", "cem"])
    ap.add_argument("--iters", type=int, default=None)
    ap.add_argument("--T", type=int, default=None)
    ap.add_argument("--N", type=int, default=None, help="samples per timestep (overrides the script's num_samples)")
    ap.add_argument("--device-rng", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--csv", default=None)
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--lazy-bounds", action="store_true",
                    help="irs-lqr methods: params.qp_lazy_bounds = True -- the bounded QPs put their penalty only on the "
                         "bounds a plan would break (the scripts' +-1e4 / +-1e5 'no bound' entries then cost nothing)")
    ap.add_argument("--batch", type=int, default=0,
                    help="irs-lqr methods: B problems in one IrsLqrBatch -- problem b starts from the script's "
                         "u_trj_initial plus a fixed, seeded perturbation and draws with seed + b (device RNG)")
    a = ap.parse_args()

    sysd, params, sm, cem, iters = PROBLEMS[a.system](*([a.T] if a.T else []))
    iters = a.iters if a.iters is not None else iters
    N = a.N or sm["N"]
    if a.lazy_bounds:
        params.qp_lazy_bounds = True
    np.random.seed(a.seed)
    if a.batch > 0:
        if a.method == "cem":
            ap.error("--batch runs the irs-lqr methods")
        return run_batch(sysd, params, sm, N, iters, a)
    if a.method == "cem":
        cp = amd.CemParameters()
        for k in ("Q", "Qd", "R", "x0", "xd_trj", "u_trj_initial"):
            setattr(cp, k, getattr(params, k))
        cp.initial_std, cp.batch_size, cp.n_elite = cem["initial_std"], cem["batch_size"], cem["n_elite"]
        if a.device_rng:        # candidates drawn inside the rollout kernel, iterate in one library call
            cp.device_seed = a.seed
        solver = amd.CrossEntropyMethod(sysd, cp)
    elif a.method == "exact":
        solver = amd.IrsLqrExact(sysd, params)
    else:
        sx, su, pw = np.asarray(sm["std_x"], float), np.asarray(sm["std_u"], float), sm["power"]
        if a.device_rng:
            sampling = amd.GaussianSmoothing(sx, su, N, power=pw, seed=a.seed)
        else:
            def sampling(xbar, ubar, it):       # the scripts' closure, e.g. pendulum_zero_order.py:38-43
                dx = np.random.normal(0.0, sx / (it ** pw), size=(N, len(sx)))
                du = np.random.normal(0.0, su / (it ** pw), size=(N, len(su)))
                return dx, du
        cls = amd.IrsLqrZeroOrder if a.method == "zero_order" else amd.IrsLqrFirstOrder
        solver = cls(sysd, params, sampling)
    solver.verbose = not a.quiet
    t0 = time.time()
    solver.iterate(iters)
    print("Final cost: " + str(solver.cost))
    print("Elapsed time: " + str(time.time() - t0))
    print("cost history:", " ".join("%.6f" % c for c in solver.cost_lst))
    if a.csv:
        np.savetxt(a.csv, np.array(solver.cost_lst))


if __name__ == "__main__":
    main()
