#!/usr/bin/env python3
"""Cost of the bounded TV-LQR kernel's factor records in HBM (csrc/boxqp.hip) against records on chip.

    python tools/time_box_horizon.py

Per sweep step: ONE tail QP (irs_tvlqr_box_solve_wsx) run for a fixed number of ADMM iterations (eps far below
reach, so every iteration runs; info[1] reports how many did), at two iteration counts; the difference over the
extra backward + forward sweep steps (2 T per iteration) is the cost of one sweep step, the factorisation and the
launch cancel.  Each at the same T with the records on chip (no workspace) and in HBM (a workspace forces them
there): bicycle T = 100 (steer limit), quadrotor T = 40 (body-rate limits).  Then whole bounded descents (T
warm-started tail QPs) of the quadrotor at T = 50 (on chip), 100, 200 (HBM)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import irs_mpc_amd as amd                                      # noqa: E402
from irs_mpc_amd import _lib, device as dev                    # noqa: E402
from examples.problems import bicycle, quadrotor               # noqa: E402

REPS = 5


def problem(name, T):
    if name == "bicycle":
        sysd, p, _, _, _ = bicycle(T)
    else:
        sysd, p, _, _, _ = quadrotor(T)
        big = np.array([1e5, 1e5, 1e5, 2 * np.pi, np.pi / 2, 2 * np.pi, 1e5, 1e5, 1e5, 7.0, 7.0, 1e5])
        p.xbound = [-big, big]
    sol = amd.IrsLqrExact(sysd, p)
    sol.verbose = False
    x, u = dev.to_dev(sol.x_trj), dev.to_dev(sol.u_trj)
    At, Bt, ct = sol._get_TV_matrices_dev(x, u)
    return sol, (At, Bt, ct, sol._Q, sol._Qd, sol._R, sol._xd, x[0].contiguous()), sol._box_bounds()


def time_solve(sol, prob, box, T, hbm, iters):
    """ms per single-tail solve of exactly `iters` ADMM iterations (median of REPS) and the iterations run."""
    dm, lib = sol._dm, _lib.load()
    xs = torch.empty((T + 1, dm.n), dtype=dev.F64, device="cuda")
    us = torch.empty((T, dm.m), dtype=dev.F64, device="cuda")
    info = torch.empty((3,), dtype=torch.int32, device="cuda")
    ws = dm._box_workspace(T, False, xs.device, force=True) if hbm else None
    xlo, xhi, ulo, uhi = (b.expand(T + 1 if i < 2 else T, -1).contiguous() for i, b in enumerate(box))
    args = [a.data_ptr() for a in prob[:6]]

    def run():
        _lib.check(lib.irs_tvlqr_box_solve_wsx(dm.model_id, dm._p, dm._np, T, *args, 0.5, prob[6].data_ptr(),
                                               prob[7].data_ptr(), 0, xlo.data_ptr(), xhi.data_ptr(), ulo.data_ptr(),
                                               uhi.data_ptr(), None, None, 10.0, 1.6, iters, 1e-300, xs.data_ptr(),
                                               us.data_ptr(), info.data_ptr(), ws.data_ptr() if hbm else None,
                                               ws.numel() if hbm else 0, dev._stream()), "irs_tvlqr_box_solve_wsx")
    run()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), int(info[1].item())


def ns_per_sweep_step(sol, prob, box, T, hbm, i1=200, i2=1200):
    t1, n1 = time_solve(sol, prob, box, T, hbm, i1)
    t2, n2 = time_solve(sol, prob, box, T, hbm, i2)
    return (t2 - t1) * 1e6 / ((n2 - n1) * 2 * T)


def main():
    for name, T in (("bicycle", 100), ("quadrotor", 40)):
        sol, prob, box = problem(name, T)
        chip = ns_per_sweep_step(sol, prob, box, T, False)
        hbm = ns_per_sweep_step(sol, prob, box, T, True)
        print("%-9s T=%3d  ns per sweep step: on chip %7.1f   HBM %7.1f   ratio HBM / on chip %.3f"
              % (name, T, chip, hbm, hbm / chip))
    for T in (50, 100, 200):
        sol, prob, box = problem("quadrotor", T)
        dm = sol._dm
        step = ns_per_sweep_step(sol, prob, box, T, T > 50)
        o = dm.tvlqr_box_descent(*prob, *box, alpha_R=0.5, rho=1.0, max_iter=20000)        # warm up (workspace allocation)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o = dm.tvlqr_box_descent(*prob, *box, alpha_R=0.5, rho=1.0, max_iter=20000)
        e1.record()
        e1.synchronize()
        info = o["info"].cpu().numpy()
        print("quadrotor T=%3d  records %-7s  bounded descent %9.1f ms  (most ADMM iterations of a tail %d, tails "
              "at max_iter %d)  ns per sweep step %.1f"
              % (T, "on chip" if T <= 50 else "in HBM", e0.elapsed_time(e1), info[1], info[2], step))


if __name__ == "__main__":
    main()
