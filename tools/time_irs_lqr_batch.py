"""Times the batched launches of the analytic models -- B descents (irs_tvlqr_descent_batch), B sample passes
(irs_smooth_rng_general_batch) and a whole IrsLqrBatch iteration (sample pass + descent + plan test + adoption) -- for
B = 1 ... 512 beside B x the single-problem calls measured in the same run, at the sizes of DESIGN 4: pendulum T=30
N=1e4, quadrotor T=50 N=1e4.

    python tools/time_irs_lqr_batch.py [pendulum|quadrotor] [--B 1,8,64,256,512] [--order zero_order|first_order]

What is timed: a window of back-to-back enqueues between two device events, long enough to last some tens of
milliseconds (the count comes from a pilot window), after a warm-up of the same calls; the figure is the median of 5
windows divided by the count, in microseconds per launch (per iteration).  The single-problem figure is the same
measurement of the single entry: calls queued back to back on one stream, which is what B separate solver objects do, so
"B x single" is B times that figure.  The B problems differ in start state, initial guess, seed and standard deviations.
Needs no oracle; on a shared GPU box run each model as a step of its own, under its own time limit."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from irs_mpc_amd import _lib, device as dev  # noqa: E402
from examples.problems import PROBLEMS  # noqa: E402

WINDOWS, WINDOW_MS = 5, 30.0
SIZES = {"pendulum": (30, 10000), "quadrotor": (50, 10000)}
MODES = {"zero_order": _lib.SMOOTH_ZERO_ORDER_AB, "first_order": _lib.SMOOTH_FIRST_ORDER}


def window_ms(fn, count):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(count):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def per_call_us(fn):
    """[us] per fn(): WINDOWS windows of `count` back-to-back calls, count sized by a pilot so a window lasts WINDOW_MS."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    pilot = window_ms(fn, 10) / 10
    count = int(min(2000, max(3, np.ceil(WINDOW_MS / max(pilot, 1e-3)))))
    us = [1e3 * window_ms(fn, count) / count for _ in range(WINDOWS)]
    return float(np.median(us)), min(us), max(us)


def fmt(v):
    return "%9.1f [%8.1f .. %8.1f]" % v


class Batch:
    """B problems of the model on the device: trajectories, goal, boxes, seeds, standard deviations, output buffers."""

    def __init__(self, name, B, mode):
        T, N = SIZES[name]
        system, p, sm, _, _ = PROBLEMS[name](T)
        self.dm, self.B, self.T, self.N, self.mode = system.dm(), B, T, N, mode
        dm, n, m = self.dm, system.dim_x, system.dim_u
        self.n, self.m = n, m
        rng = np.random.default_rng(B)
        self.Q, self.Qd, self.R = (dev.to_dev(np.asarray(a, float)) for a in (p.Q, p.Qd, p.R))
        x0 = np.asarray(p.x0, float) + 0.01 * rng.normal(size=(B, n))
        U = np.asarray(p.u_trj_initial, float) + 0.01 * rng.normal(size=(B, T, m))
        self.xd = dev.to_dev(np.tile(np.asarray(p.xd_trj, float), (B, 1, 1)))
        self.x0, self.U = dev.to_dev(x0), dev.to_dev(U)
        self.X = torch.stack([dm.rollout_cost(self.x0[b], self.U[b], self.Q, self.R, self.xd[b])[0] for b in range(B)])
        self.std_x = np.asarray(sm["std_x"], float) * (1.0 + 0.1 * rng.uniform(size=(B, 1)))
        self.std_u = np.asarray(sm["std_u"], float) * (1.0 + 0.1 * rng.uniform(size=(B, 1)))
        self.sx, self.su = dev.to_dev(self.std_x), dev.to_dev(self.std_u)
        self.seeds = torch.arange(1, B + 1, dtype=torch.int64, device="cuda")
        box = [np.broadcast_to(np.asarray(v, float), (B, d)).copy()
               for v, d in ((p.xbound[0], n), (p.xbound[1], n), (p.ubound[0], m), (p.ubound[1], m))]
        self.box = [dev.to_dev(v) for v in box]
        self.lin = dm._tv_alloc(dm._tv_shapes((B, T), mode), "cuda")
        self.out = dm._tv_alloc(dict(K=(B, T, m, n), k=(B, T, m), x_new=(B, T + 1, n), u_new=(B, T, m), cost=(B,),
                                     info=(B,)), "cuda")
        self.flag = torch.zeros((B,), dtype=torch.int32, device="cuda")
        self.alive = torch.ones((B,), dtype=torch.bool, device="cuda")

    # ---- the batched launches
    def smooth(self):
        self.dm.smooth_rng_general_batch(self.mode, self.X, self.U, self.N, self.sx, self.su, self.seeds, 1, out=self.lin)

    def descent(self):
        o = self.lin
        self.dm.tvlqr_descent_batch(o["At"], o["Bt"], o["ct"], self.Q, self.Qd, self.R, self.xd, self.x0, out=self.out)

    def iteration(self):
        self.smooth()
        self.descent()
        o, d = self.lin, self.out
        self.dm.plan_within_bounds_batch(o["At"], o["Bt"], o["ct"], d["K"], d["k"], d["x_new"], *self.box, flag=self.flag)
        alive = self.alive & (d["info"] == 0) & (self.flag == 0) & ~(o["info"] != 0).any(dim=1)
        keep = alive[:, None, None]
        # (the timing keeps linearising around the same trajectories: the adopted ones are computed and dropped)
        torch.where(keep, d["x_new"], self.X), torch.where(keep, d["u_new"], self.U)

    # ---- problem 0 through the single-problem entries
    def single_setup(self):
        self.lin1 = {k: v[0] for k, v in self.lin.items()}
        self.out1 = {k: v[0:1] if k in ("cost", "info") else v[0] for k, v in self.out.items()}
        self.x00 = self.x0[0].contiguous()

    def single_smooth(self):
        self.dm.smooth_rng(self.mode, self.X[0], self.U[0], self.N, self.std_x[0], self.std_u[0], 1, 1, out=self.lin1)

    def single_descent(self):
        o = self.lin1
        self.dm.tvlqr_descent(o["At"], o["Bt"], o["ct"], self.Q, self.Qd, self.R, self.xd[0], self.x00, out=self.out1)

    def single_iteration(self):
        self.single_smooth()
        self.single_descent()
        o, d, b = self.lin1, self.out1, self.box
        _lib.check(self.dm.lib.irs_tvlqr_plan_within_bounds(
            self.n, self.m, self.T, o["At"].data_ptr(), o["Bt"].data_ptr(), o["ct"].data_ptr(), d["K"].data_ptr(),
            d["k"].data_ptr(), d["x_new"].data_ptr(), b[0].data_ptr(), b[1].data_ptr(), b[2].data_ptr(), b[3].data_ptr(),
            self.flag.data_ptr(), dev._stream()), "irs_tvlqr_plan_within_bounds")


def main():
    argv = sys.argv[1:]

    def option(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    names = [v for v in argv if v in SIZES] or list(SIZES)
    Bs = [int(v) for v in option("--B", "1,8,64,256,512").split(",")]
    order = option("--order", "zero_order")
    for name in names:
        T, N = SIZES[name]
        one = Batch(name, 1, MODES[order])
        one.single_setup()
        sp, sd, si = per_call_us(one.single_smooth), per_call_us(one.single_descent), per_call_us(one.single_iteration)
        print("%s %s T=%d N=%d; us per launch as median [min .. max] of %d windows" % (name, order, T, N, WINDOWS))
        print("single  sample pass %s   descent %s   iteration %s" % (fmt(sp), fmt(sd), fmt(si)), flush=True)
        for B in Bs:
            b = Batch(name, B, MODES[order])
            p, d, i = per_call_us(b.smooth), per_call_us(b.descent), per_call_us(b.iteration)
            failed = int((b.out["info"] != 0).sum().item() + (b.lin["info"] != 0).any(dim=1).sum().item())
            print("B=%-4d sample pass %s (B x single %10.1f)   descent %s (B x single %10.1f)   iteration %s "
                  "(B x single %10.1f)   %9.0f problem-iterations/s   failed %d"
                  % (B, fmt(p), B * sp[0], fmt(d), B * sd[0], fmt(i), B * si[0], B / (i[0] * 1e-6), failed), flush=True)
            del b
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
