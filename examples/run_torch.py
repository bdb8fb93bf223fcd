#!/usr/bin/env python3
"""iRS-LQR on a system that exists only as a torch callable: the cart-pole of examples/torch_systems.py (n = 4, m = 1,
no compiled functor -- the values pass and the generic Riccati kernel run) through the three optimiser classes.

    python examples/run_torch.py                       # zero_order, first_order and exact, one after the other
    python examples/run_torch.py zero_order --iters 20 --N 2000
    python examples/run_torch.py exact --ubound 4      # |force| <= 4: bounded descents through the any-size box-QP kernel
    python examples/run_torch.py cem [--device-rng]    # the cross-entropy baseline beside exact iRS-LQR

The task is a crane's: the load starts swinging 0.5 rad off the vertical; move the cart one metre and bring the load to
rest under it (T = 100 steps of 0.02 s).  Samples are drawn on the GPU (GaussianSmoothing, Philox).

`cem` runs CrossEntropyMethod on the same problem -- the candidate rollouts are stage launches of csrc/cem.hip with the
callable stepping all candidates between them; --device-rng draws the candidates inside the stages and enqueues every
descent before reading anything back -- and prints its cost beside IrsLqrExact's, the way the reference's *_cem.py
scripts sit beside its iRS-LQR ones.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import irs_mpc_amd as amd  # noqa: E402
from examples.torch_systems import TorchCartPole  # noqa: E402


def cartpole_problem(T):
    p = amd.IrsLqrParameters()
    p.Q = np.diag([1.0, 1.0, 0.1, 0.1])
    p.Qd = np.diag([20.0, 20.0, 2.0, 2.0])
    p.R = np.diag([0.1])
    p.x0 = np.array([0.0, 0.5, 0.0, 0.0])
    p.xd_trj = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (T + 1, 1))
    p.u_trj_initial = np.zeros((T, 1))
    return p


def run_cem(a):
    """CrossEntropyMethod on the cart-pole, then IrsLqrExact on the same problem for comparison."""
    params = cartpole_problem(a.T)
    cp = amd.CemParameters()
    for k in ("Q", "Qd", "R", "x0", "xd_trj", "u_trj_initial"):
        setattr(cp, k, getattr(params, k))
    cp.initial_std, cp.batch_size, cp.n_elite = np.array([a.std]), a.batch, a.elite
    if a.device_rng:
        cp.device_seed = a.seed
    np.random.seed(a.seed)
    solver = amd.CrossEntropyMethod(TorchCartPole(a.h), cp)
    solver.verbose = not a.quiet
    t0 = time.time()
    solver.iterate(a.iters)
    t_cem = time.time() - t0
    lqr = amd.IrsLqrExact(TorchCartPole(a.h), params)
    lqr.verbose = False
    t0 = time.time()
    lqr.iterate(a.iters)
    print("cem: final cost %.6f after %d iterations, %.2f s" % (solver.cost, a.iters, t_cem))
    print("exact iRS-LQR: final cost %.6f after %d iterations, %.2f s" % (lqr.cost, a.iters, time.time() - t0))
    print("cost history:", " ".join("%.6f" % c for c in solver.cost_lst))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("method", nargs="?", default="all", choices=["all", "zero_order", "first_order", "exact", "cem"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--N", type=int, default=1000)
    ap.add_argument("--h", type=float, default=0.02)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--ubound", type=float, default=None, metavar="V",
                    help="bound the force on the cart, |u| <= V: where it binds, the stepped bounded descent runs "
                         "(IrsLqrParameters.qp_model_free)")
    ap.add_argument("--batch", type=int, default=2000, help="cem: candidates per descent")
    ap.add_argument("--elite", type=int, default=40, help="cem: elites kept per descent")
    ap.add_argument("--std", type=float, default=2.0, help="cem: initial standard deviation of the force")
    ap.add_argument("--device-rng", action="store_true",
                    help="cem: draw the candidates on the GPU (CemParameters.device_seed = --seed)")
    a = ap.parse_args()
    if a.method == "cem":
        return run_cem(a)
    for method in (["zero_order", "first_order", "exact"] if a.method == "all" else [a.method]):
        system, params = TorchCartPole(a.h), cartpole_problem(a.T)
        if a.ubound is not None:
            params.ubound = np.array([[-a.ubound], [a.ubound]])
            params.qp_model_free = True
        if method == "exact":
            solver = amd.IrsLqrExact(system, params)
        else:
            sampling = amd.GaussianSmoothing([0.05, 0.05, 0.1, 0.1], [0.5], a.N, seed=a.seed)
            solver = (amd.IrsLqrZeroOrder if method == "zero_order" else amd.IrsLqrFirstOrder)(system, params, sampling)
        solver.verbose = not a.quiet
        t0 = time.time()
        solver.iterate(a.iters)
        print("%s: final cost %.6f after %d iterations, %.2f s" % (method, solver.cost, a.iters, time.time() - t0))
        print("cost history:", " ".join("%.6f" % c for c in solver.cost_lst))


if __name__ == "__main__":
    main()
