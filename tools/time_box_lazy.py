#!/usr/bin/env python3
"""The bounded TV-LQR descent with every finite bound penalised and with lazily enforced bounds (csrc/boxqp.hip,
irs_tvlqr_box_descent_lazy), each with the fixed and with the adaptive ADMM penalty.

    python tools/time_box_lazy.py [descents]

The first `descents` (default 1) bounded descents of IrsLqrExact on the hard bicycle problem (examples/problems.py
bicycle_hard: T = 100, steer bound pi / 4, every other bound the script's finite +-1e4; the class's defaults rho = 10,
max_iter = 5000, eps = 1e-8), each a launch of T warm-started tail QPs on the trajectory the lazy + adaptive form
produced before it.  Per form (fixed / adaptive: the kernels as they were, every finite bound carries a rho term;
lazy / lazy + adaptive): median, minimum and maximum ms of 3 launches in this process after a warm-up launch, taken in
turn, most iterations of a tail, tails at the limit, and where the kernel reports them ADMM iterations of all tails,
factorisations, activations, the final set and rho, and the distance of u_new from the fixed form's."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import irs_mpc_amd as amd                                      # noqa: E402
from irs_mpc_amd import device as dev                          # noqa: E402
from examples.problems import bicycle_hard                     # noqa: E402

REPS = 3
FORMS = (("fixed", {}), ("adaptive", dict(adaptive_rho=True)), ("lazy", dict(lazy_bounds=True)),
         ("lazy+adaptive", dict(lazy_bounds=True, adaptive_rho=True)))


def timed_once(run):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    o = run()
    e1.record()
    e1.synchronize()
    return o, e0.elapsed_time(e1)


def main():
    descents = int(sys.argv[1]) if len(sys.argv) > 1 else 1
    sysd, p, _, _, _ = bicycle_hard()
    sol = amd.IrsLqrExact(sysd, p)
    sol.verbose = False
    dm, T = sol._dm, sol.T
    x, u = dev.to_dev(sol.x_trj), dev.to_dev(sol.u_trj)
    enforced = None
    for d in range(1, descents + 1):
        At, Bt, ct = sol._get_TV_matrices_dev(x, u)
        prob = (At, Bt, ct, sol._Q, sol._Qd, sol._R, sol._xd, x[0].contiguous())
        kw = dict(alpha_R=0.5, rho=10.0, max_iter=5000, eps=1e-8)
        runs = {}
        for name, extra in FORMS:
            if extra.get("lazy_bounds"):
                extra = dict(extra, enforced=enforced)
            runs[name] = (lambda extra=extra: dm.tvlqr_box_descent(*prob, *sol._box_bounds(), **kw, **extra))
            runs[name]()                                        # warm up (code object, workspace)
        torch.cuda.synchronize()
        ms, out = {name: [] for name in runs}, {}
        for _ in range(REPS):                                   # the forms in turn, so drift hits all alike
            for name, run in runs.items():
                out[name], t = timed_once(run)
                ms[name].append(t)
        for name, _ in FORMS:
            o = out[name]
            info = o["info"].cpu().numpy()
            line = "descent %d T=%d %-14s %9.2f ms (min %.2f, max %.2f)  most iterations %5d, tails at the limit %3d" % (
                d, T, name, float(np.median(ms[name])), min(ms[name]), max(ms[name]), info[1], info[2])
            if "adapt" in o:
                adapt = o["adapt"].cpu().numpy()
                line += ", iterations %7d, factorisations %2d, final rho %.4g" % (adapt[2], adapt[0], adapt[1])
            if "lazy" in o:
                lazy = o["lazy"].cpu().numpy()
                line += ", activations %d (last at tail %d), set %s (from %s)" % (
                    lazy[0], lazy[1], o["enforced"].cpu().numpy(), None if enforced is None else enforced.cpu().numpy())
            line += "; max |u - u_fixed| %.2e" % (o["u_new"] - out["fixed"]["u_new"]).abs().max().item()
            print(line, flush=True)
        best = out["lazy+adaptive"]
        x, u, enforced = best["x_new"], best["u_new"], best["enforced"]


if __name__ == "__main__":
    main()
