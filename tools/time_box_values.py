#!/usr/bin/env python3
"""What the stepped bounded descent of a torch-defined system (csrc/boxqp_values.hip) costs beside the compiled
one-launch descent (irs_tvlqr_box_descent) on the same problem and the same linearisation.

    python tools/time_box_values.py [--quick]

The pendulum and the quadrotor of the reference's scripts (examples/problems.py, T = 200; --quick: T = 40) written as
torch callables (examples/torch_systems.py), linearised exactly about the initial rollout by the compiled functor, with
|u| bounded at 0.6 of the unbounded descent's peak and no x bound (the scripts' +-1e5 "none" would put the penalty
term on every state component: what qp_lazy_bounds is for, and that form is compiled-only).  Device events, median
[min .. max] of 5 timings after a warm-up, taken in turn:

  compiled   DeviceModel.tvlqr_box_descent: factorisation, T tails and T plant steps in ONE launch -- the yardstick;
  stepped    TorchDeviceModel.tvlqr_box_descent: begin + T x (tail launch + one float64 step of the callable);
  tails      begin + the T tail launches alone, from the states the stepped descent realised (the same ADMM work);
  steps      the T float64 steps of the callable alone.
Also printed: the ADMM iterations (most of any tail, tails at the cap) of both, and the largest difference between the
two descents.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from irs_mpc_amd import device as dev                          # noqa: E402
from examples import problems                                  # noqa: E402
from examples.torch_systems import TorchPendulum, TorchQuadrotor   # noqa: E402

TIMINGS = 5
QP = dict(rho=10.0, relax=1.6, max_iter=5000, eps=1e-8)


def timed(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def fmt(us):
    return "%10.1f us [%.1f .. %.1f]" % (float(np.median(us)), min(us), max(us))


def one(name, make, torch_sys, T):
    compiled_sys, p, _, _, _ = make(T)
    dm_c, dm_t = compiled_sys.dm(), torch_sys.dm()
    Q, Qd, R, xd, x0 = (dev.to_dev(np.asarray(a, float)) for a in (p.Q, p.Qd, p.R, p.xd_trj, p.x0))
    u0 = dev.to_dev(p.u_trj_initial)
    x_trj, _ = dm_c.rollout_cost(x0, u0, Q, R, xd)
    At, Bt, ct = dm_c.exact_linearize(x_trj, u0)
    free = dm_c.tvlqr_descent(At, Bt, ct, Q, Qd, R, xd, x0)
    ub = 0.6 * float(free["u_new"].abs().max().item())
    m = u0.shape[1]
    n = At.shape[1]
    box = [dev.to_dev(np.full(n, -np.inf)), dev.to_dev(np.full(n, np.inf)), dev.to_dev(np.full(m, -ub)),
           dev.to_dev(np.full(m, ub))]
    prob = (At, Bt, ct, Q, Qd, R, xd)

    def compiled():
        return dm_c.tvlqr_box_descent(*prob, x0, *box, **QP)

    def stepped():
        return dm_t.tvlqr_box_descent(*prob, x0, *box, **QP)

    oc, ot = compiled(), stepped()
    torch.cuda.synchronize()
    xs, us = ot["x_new"].clone(), ot["u_new"].clone()
    u_t = torch.empty((m,), dtype=dev.F64, device="cuda")

    def tails():
        h = dev.box_values_begin(*prob, *box, rho=QP["rho"], relax=QP["relax"])
        for t in range(T):
            dev.box_values_tail(h, t, xs[t], QP["max_iter"], QP["eps"], u_t=u_t)
        return h["info"]

    def steps():
        for t in range(T):
            dm_t._step(xs[t], us[t])

    runs = dict(compiled=compiled, stepped=stepped, tails=tails, steps=steps)
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    us_ = {k: [] for k in runs}
    for _ in range(TIMINGS):                                    # in turn, so drift hits all alike
        for k, run in runs.items():
            us_[k].append(timed(run)[0])
    ic, it_ = oc["info"].cpu().numpy(), ot["info"].cpu().numpy()
    gap = max((oc["x_new"] - ot["x_new"]).abs().max().item(), (oc["u_new"] - ot["u_new"]).abs().max().item())
    print("%s (n,m,T)=(%d,%d,%d) |u| <= %.4g (unbounded peak %.4g)" % (name, At.shape[1], m, T, ub, ub / 0.6), flush=True)
    for k in runs:
        print("  %-9s %s" % (k, fmt(us_[k])), flush=True)
    med = {k: float(np.median(v)) for k, v in us_.items()}
    print("  stepped / compiled %.2f; tails %.0f %%, steps %.0f %% of stepped; info compiled %s stepped %s; "
          "max |compiled - stepped| %.2e" % (med["stepped"] / med["compiled"], 100 * med["tails"] / med["stepped"],
                                             100 * med["steps"] / med["stepped"], ic.tolist(), it_.tolist(), gap), flush=True)


def main():
    dev.require_gpu()
    T = 40 if "--quick" in sys.argv else 200
    one("pendulum", problems.pendulum, TorchPendulum(0.05), T)
    one("quadrotor", problems.quadrotor, TorchQuadrotor(0.05), T)
    return 0


if __name__ == "__main__":
    sys.exit(main())
