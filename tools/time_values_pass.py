#!/usr/bin/env python3
"""What the values pass (csrc/smooth_values.hip) costs, and what it replaces.

    python tools/time_values_pass.py [--quick]

Device events, median [min .. max] of 5 timings after a warm-up, at (n, m, T, N) = (2,1,30,1e4), (12,4,50,1e4),
(12,4,50,1e5), (32,16,50,1e4) (--quick: N / 10, for a rehearsal):

  (a) irs_smooth_values alone (both launches: statistics + reduction and solve), the mean of REPS_A back-to-back
      calls per timing; the bytes the pass has to read, 4 T N (d + n), over that time as a share of 8 TB/s; and its two
      halves as entries of their own: irs_smooth_values_accumulate (statistics + reduction), ..._finalize (the solve);
  (b) the only model-free route without it: T calls of irs_least_squares on f64 copies of the same data, one pass of
      T calls per timing.  (a) and (b) are timed in turn in the same process;
  (c) one whole get_TV_matrices (T = 50, N = 1e4) of the pendulum and the quadrotor written as torch callables
      (examples/torch_systems.py) -- draw, evaluate, values pass -- beside the compiled functors' one-launch smooth_rng.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import irs_mpc_amd as amd                                      # noqa: E402
from irs_mpc_amd import _lib, device as dev                    # noqa: E402
from irs_mpc_amd._lib import SMOOTH_ZERO_ORDER_AB              # noqa: E402
from examples.torch_systems import TorchPendulum, TorchQuadrotor   # noqa: E402

SIZES = [(2, 1, 30, 10000), (12, 4, 50, 10000), (12, 4, 50, 100000), (32, 16, 50, 10000)]
TIMINGS, REPS_A = 5, 20
PEAK_BYTES_PER_S = 8e12


def timed(run, reps=1):
    """Microseconds per call of `run`, device events around `reps` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        run()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def fmt(us):
    return "%10.1f us [%.1f .. %.1f]" % (float(np.median(us)), min(us), max(us))


def inputs(n, m, T, N):
    g = torch.Generator(device="cuda").manual_seed(1000 * n + m)
    d = n + m
    z = torch.randn((T, N, d), generator=g, device="cuda", dtype=torch.float32)
    W = torch.randn((d, n), generator=g, device="cuda", dtype=torch.float32) / d ** 0.5
    f0 = torch.randn((T, n), generator=g, device="cuda", dtype=torch.float32)
    fz = f0[:, None, :] + z @ W + 1e-3 * torch.randn((T, N, n), generator=g, device="cuda", dtype=torch.float32)
    x = torch.randn((T + 1, n), generator=g, device="cuda", dtype=torch.float64)
    u = torch.randn((T, m), generator=g, device="cuda", dtype=torch.float64)
    return z[:, :, :n].contiguous(), z[:, :, n:].contiguous(), fz.contiguous(), f0, x, u, f0.double()


def values_vs_least_squares(n, m, T, N):
    lib = _lib.load()
    dx, du, fz, f0, x, u, fnom = inputs(n, m, T, N)
    out = dev.smooth_values(x, u, dx, du, fz, f0, fnom)

    def run_a():
        dev.smooth_values(x, u, dx, du, fz, f0, fnom, out=out)

    Z64 = torch.cat([dx, du], dim=2).double().contiguous()
    dF64 = (fz - f0[:, None, :]).double().contiguous()
    A = torch.empty((T, n, n), dtype=dev.F64, device="cuda")
    B = torch.empty((T, n, m), dtype=dev.F64, device="cuda")
    info = torch.empty((T,), dtype=torch.int32, device="cuda")
    st = dev._stream()

    def run_b():
        for t in range(T):
            _lib.check(lib.irs_least_squares(n, m, N, Z64[t].data_ptr(), dF64[t].data_ptr(), A[t].data_ptr(),
                                             B[t].data_ptr(), info[t:].data_ptr(), st), "irs_least_squares")

    for _ in range(3):
        run_a()
    run_b()
    torch.cuda.synchronize()
    assert int(out["info"].abs().sum().item()) == 0 and int(info.abs().sum().item()) == 0
    gap = max((out["At"] - A).abs().max().item(), (out["Bt"] - B).abs().max().item())
    sums = out["sums"].clone()
    fin = dict(At=out["At"], Bt=out["Bt"], ct=out["ct"], info=out["info"])
    parts = dict(acc=lambda: dev.smooth_values_accumulate(dx, du, fz, f0, sums=sums),
                 fin=lambda: dev.smooth_values_finalize(N, x, u, fnom, sums, out=fin))
    ta, tb, tp = [], [], dict(acc=[], fin=[])
    for _ in range(TIMINGS):                                    # in turn, so drift hits both alike
        ta.append(timed(run_a, REPS_A))
        tb.append(timed(run_b))
        for k, run in parts.items():                            # where (a) goes: statistics + reduction | solve alone
            tp[k].append(timed(run, REPS_A))
    geo = dev.smooth_values_geometry(T, N)
    nbytes = 4.0 * T * N * (n + m + n)
    share = nbytes / (float(np.median(ta)) * 1e-6) / PEAK_BYTES_PER_S
    print("(n,m,T,N)=(%d,%d,%d,%d) nblk %d" % (n, m, T, N, geo["nblk"]), flush=True)
    print("  (a) values pass        %s   %.1f MB read, %.1f %% of 8 TB/s" % (fmt(ta), nbytes / 1e6, 100 * share), flush=True)
    print("      accumulate entry   %s   finalize entry %s" % (fmt(tp["acc"]), fmt(tp["fin"])), flush=True)
    print("  (b) T x least_squares  %s   ranges %s; max |AB(a) - AB(b)| %.2e"
          % (fmt(tb), "apart, (a) below (b)" if max(ta) < min(tb) else "TOUCH", gap), flush=True)
    return max(ta) < min(tb)


def callable_vs_functor(name, torch_sys, compiled_sys, T, N, std_x, std_u):
    xs = [np.zeros(torch_sys.dim_x)]
    u_trj = np.tile(np.full(torch_sys.dim_u, 2.0 if name == "quadrotor" else 0.1), (T, 1))
    for t in range(T):
        xs.append(compiled_sys.dynamics(xs[-1], u_trj[t]))
    x, u = dev.to_dev(np.stack(xs)), dev.to_dev(u_trj)
    dm_t, dm_c = torch_sys.dm(), compiled_sys.dm()
    runs = dict(torch=lambda: dm_t.smooth_rng(SMOOTH_ZERO_ORDER_AB, x, u, N, std_x, std_u, 1, 1),
                compiled=lambda: dm_c.smooth_rng(SMOOTH_ZERO_ORDER_AB, x, u, N, std_x, std_u, 1, 1))
    outs = {k: run() for k, run in runs.items()}
    for run in runs.values():
        run()
    torch.cuda.synchronize()
    us = {k: [] for k in runs}
    for _ in range(TIMINGS):
        for k, run in runs.items():
            us[k].append(timed(run, 5))
    gap = max((outs["torch"][k] - outs["compiled"][k]).abs().max().item() for k in ("At", "Bt", "ct"))
    print("(c) %s get_TV_matrices T=%d N=%d: torch callable %s | compiled functor %s | max difference %.2e"
          % (name, T, N, fmt(us["torch"]), fmt(us["compiled"]), gap), flush=True)


def main():
    quick = "--quick" in sys.argv
    dev.require_gpu()
    ok = True
    for n, m, T, N in SIZES:
        ok = values_vs_least_squares(n, m, T, N // 10 if quick else N) and ok
    N = 1000 if quick else 10000
    callable_vs_functor("pendulum", TorchPendulum(0.05), amd.PendulumDynamics(0.05), 50, N, [1.0, 1.0], [1.0])
    callable_vs_functor("quadrotor", TorchQuadrotor(0.05), amd.QuadrotorDynamics(0.05), 50, N, [0.1] * 12, [0.1] * 4)
    print("acceptance (a) below (b) with ranges apart at every size: %s" % ("yes" if ok else "NO"), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
