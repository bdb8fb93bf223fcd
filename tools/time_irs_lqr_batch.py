"""Times the batched launches of the analytic models -- B descents (irs_tvlqr_descent_batch), B sample passes
(irs_smooth_rng_general_batch) and a whole IrsLqrBatch iteration (sample pass + descent + plan test + adoption) -- for
B = 1 ... 512 beside B x the single-problem calls measured in the same run, at the sizes of DESIGN 4: pendulum T=30
N=1e4, quadrotor T=50 N=1e4.

    python tools/time_irs_lqr_batch.py [pendulum|quadrotor] [--B 1,8,64,256,512] [--order zero_order|first_order]
    python tools/time_irs_lqr_batch.py bounded [--B 1,8,64,256,512] [--max-singles K] [--reps 3]

`bounded`: B bounded descents in one launch (irs_tvlqr_box_descent_batch, records on chip and forced to HBM) beside
the single entry (irs_tvlqr_box_descent_if) on the same inputs, on the example script's bicycle problem (T = 100).

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


class Bounded:
    """B copies of the example script's bicycle problem (T = 100, steer bound; examples/run.py --batch: problem b starts
    from u_trj_initial + 0.01 N(0,1) drawn with seed b, problem 0 from the script's), linearised exactly along the
    rollout of their guesses: the inputs of the first bounded descent of `examples/run.py bicycle exact --batch B`."""

    def __init__(self, B, T=100):
        system, p, _, _, _ = PROBLEMS["bicycle"](T)
        self.dm, self.B, self.T = system.dm(), B, T
        dm, n, m = self.dm, system.dim_x, system.dim_u
        U = np.stack([np.asarray(p.u_trj_initial, float)
                      + (0.01 * np.random.default_rng(b).normal(size=(T, m)) if b > 0 else 0.0) for b in range(B)])
        self.Q, self.Qd, self.R = (dev.to_dev(np.asarray(a, float)) for a in (p.Q, p.Qd, p.R))
        self.xd = dev.to_dev(np.tile(np.asarray(p.xd_trj, float), (B, 1, 1)))
        self.x0 = dev.to_dev(np.tile(np.asarray(p.x0, float), (B, 1)))
        Ud = dev.to_dev(U)
        X = torch.stack([dm.rollout_cost(self.x0[b], Ud[b], self.Q, self.R, self.xd[b])[0] for b in range(B)])
        At, Bt, ct = dm.exact_linearize(X[:, :T].reshape(B * T, n), Ud.reshape(B * T, m))
        self.lin = (At.view(B, T, n, n).contiguous(), Bt.view(B, T, n, m).contiguous(), ct.view(B, T, n).contiguous())
        self.box = [dev.to_dev(np.broadcast_to(np.asarray(v, float), (B, d)).copy())
                    for v, d in ((p.xbound[0], n), (p.xbound[1], n), (p.ubound[0], m), (p.ubound[1], m))]
        self.out = dm._tv_alloc(dict(x_new=(B, T + 1, n), u_new=(B, T, m), cost=(B,), info=(B, 3)), "cuda")

    def batch(self, hbm):
        self.dm.tvlqr_box_descent_batch(*self.lin, self.Q, self.Qd, self.R, self.xd, self.x0, *self.box,
                                        records_in_hbm=hbm, out=self.out)

    def single(self, b):
        """irs_tvlqr_box_descent_if on problem b's blocks, into problem b's rows of the outputs."""
        dm, o = self.dm, self.out
        ptr = [t[b].data_ptr() for t in self.lin] + [t.data_ptr() for t in (self.Q, self.Qd, self.R)]
        _lib.check(dm.lib.irs_tvlqr_box_descent_if(
            dm.model_id, dm._p, dm._np, self.T, *ptr, 0.5, self.xd[b].data_ptr(), self.x0[b].data_ptr(),
            *[t[b].data_ptr() for t in self.box], 10.0, 1.6, 5000, 1e-8, o["x_new"][b].data_ptr(), o["u_new"][b].data_ptr(),
            o["cost"][b:b + 1].data_ptr(), o["info"][b].data_ptr(), None, dev._stream()), "irs_tvlqr_box_descent_if")


def launch_us(fn, reps=3):
    """[us] of one fn() between two device events: median, min, max of `reps` after one warm-up.  A bounded descent lasts
    milliseconds to seconds, far above the event resolution, so every launch is a window of its own."""
    fn()
    torch.cuda.synchronize()
    us = [1e3 * window_ms(fn, 1) for _ in range(reps)]
    return float(np.median(us)), min(us), max(us)


def bounded_rows(Bs, max_singles, reps=3):
    """Per B: the batched launch with its records on chip and forced to HBM, beside the single entry on the same inputs
    -- every problem alone, once, between its own events after a warm-up (`singles`: their sum, i.e. the calls back to
    back without the launch gaps; the slowest one is what the batch has to wait for).  Beyond max_singles problems only
    the first max_singles are run alone, and the row says so."""
    print("bicycle T=100 bounded descent (steer bound); us per launch as median [min .. max] of %d launches" % reps,
          flush=True)
    for B in Bs:
        b = Bounded(B)
        K = min(B, max_singles)
        b.single(0)
        each = [1e3 * window_ms(lambda q=q: b.single(q), 1) for q in range(K)]
        info1 = b.out["info"].cpu().numpy()[:K].copy()
        lds, hbm = launch_us(lambda: b.batch(False), reps), launch_us(lambda: b.batch(True), reps)
        info = b.out["info"].cpu().numpy()
        assert np.array_equal(info[:K], info1), "the batch and the singles disagree on info"
        print("B=%-4d on chip %s   in HBM %s   %d singles: sum %11.1f  slowest %9.1f  fastest %9.1f"
              "   most ADMM iterations %d   unsolved %d"
              % (B, fmt(lds), fmt(hbm), K, sum(each), max(each), min(each), int(info[:, 1].max()),
                 int(((info[:, 2] != 0) | (info[:, 0] != 0)).sum())), flush=True)
        del b
        torch.cuda.empty_cache()


def main():
    argv = sys.argv[1:]

    def option(name, default):
        return argv[argv.index(name) + 1] if name in argv else default

    if "bounded" in argv:
        return bounded_rows([int(v) for v in option("--B", "1,8,64,256,512").split(",")],
                            int(option("--max-singles", "512")), int(option("--reps", "3")))
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
