"""Times B quasistatic descents in one launch (irs_quasistatic_box_descent_batch), the B sample passes -- as B calls
of the single-problem entry and, where it is served (the planar hand), as ONE batched launch (irs_smooth_rng_batch) --
and a whole batched iteration (sample passes + one bound-rows launch + the batched descent, for both settings of
`batched_sample_pass`) beside B x the single-problem call, at the benchmark's sizes: planar hand T=50 N=1e4, box
pivoting T=80 N=6250.  Device-event times, 5 repetitions after a warm-up.

    python tools/time_quasistatic_batch.py [planar_hand|box_pivoting] [--B 1,8,64,256,512] [--distinct] [--single-only]

The B problems are copies of one problem (so the launch time shows what the hardware does with B equal workgroups);
--distinct linearises every problem on its own draws instead (the launch then lasts as long as its slowest problem).
--single-only times the single-problem descent alone (also runs against a library without the batched entries).
Needs no oracle; on a shared GPU box run each B as a step of its own, under its own time limit."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from irs_mpc_amd import device as dev  # noqa: E402
import bench  # noqa: E402

REPS = 5


def event_ms(fn, reps=REPS):
    """[ms] of `reps` runs of fn(), each between two device events, after one warm-up run."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def fmt(ms):
    return "%8.3f [%7.3f .. %7.3f]" % (float(np.median(ms)), min(ms), max(ms))


class Problem:
    """One problem of the workload on the device: nominal trajectory, weights, bound offsets, sample-pass settings."""

    def __init__(self, name, N=None):
        w = bench.Workload(name)
        self.w, self.name, self.T = w, name, w.T
        self.N = N or (10000 if name == "planar_hand" else 6250)
        self.dm = w.system.dm()
        self.m, self.n = self.dm.m, self.dm.n
        self.Q, self.Qd, self.R = dev.to_dev(w.Q), dev.to_dev(w.Qd), dev.to_dev(w.R)
        self.xd, self.x0, self.u_trj = dev.to_dev(w.xd), dev.to_dev(w.x0), dev.to_dev(w.u_trj)
        self.x_trj, _ = self.dm.rollout_cost(self.x0, self.u_trj, self.Q, self.R, self.xd)
        self.idx = torch.as_tensor(np.asarray(w.idx), device="cuda")
        self.kind, width = w.bounds
        self.off = torch.tensor([[-width] * self.m, [width] * self.m], dtype=torch.float64, device="cuda")
        self.std_u = [float(w.std_schedule(1))] * self.m

    def smooth(self, seed, out=None):
        return self.dm.smooth_rng(self.w.mode, self.x_trj, self.u_trj, self.N, None, self.std_u, seed, 1, out=out)

    def rows(self):
        """The torch expression of IrsLqrQuasistatic._bounds_dev."""
        center = (self.x_trj[:-1].index_select(1, self.idx) if self.kind == "abs"
                  else torch.zeros((self.T, self.m), dtype=torch.float64, device="cuda"))
        lo, hi = (center + self.off[0]).contiguous(), (center + self.off[1]).contiguous()
        return dict(u_lo=lo, u_hi=hi) if self.kind == "abs" else dict(du_lo=lo, du_hi=hi)


def time_single(p):
    """(descent ms, iteration ms) of the single-problem path: 5 repetitions each, cold active set every time."""
    o = p.smooth(0)
    act = torch.zeros((p.T, p.m), dtype=torch.float64, device="cuda")
    out = {}

    def descent(lin=o):
        act.zero_()
        out.update(p.dm.quasistatic_box_descent(lin["At"], lin["Bt"], lin["ct"], p.Q, p.Qd, p.R, p.xd, p.x0, solver=3,
                                                max_iter=2000, eps=1e-9, act=act, out=out or None, **p.rows()))

    def iteration():
        descent(p.smooth(0, out=o))

    d, i = event_ms(descent), event_ms(iteration)
    info = out["info"].cpu().numpy().tolist()
    return d, i, info, float(out["cost"].item())


def time_batch(p, B, distinct):
    T, n, m, dm = p.T, p.n, p.m, p.dm
    AT = torch.empty((B, T, n, n), dtype=torch.float64, device="cuda")
    BT = torch.empty((B, T, n, m), dtype=torch.float64, device="cuda")
    CT = torch.empty((B, T, n), dtype=torch.float64, device="cuda")
    info = torch.empty((B, T), dtype=torch.int32, device="cuda")
    sums = torch.empty((B, T, dm.sums_len(p.w.mode)), dtype=torch.float64, device="cuda")
    outs = [dict(sums=sums[b], At=AT[b], Bt=BT[b], ct=CT[b], info=info[b]) for b in range(B)]
    X = p.x_trj.unsqueeze(0).repeat(B, 1, 1).contiguous()
    XD = p.xd.unsqueeze(0).repeat(B, 1, 1).contiguous()
    X0 = p.x0.unsqueeze(0).repeat(B, 1).contiguous()
    off = p.off.unsqueeze(0).repeat(B, 1, 1).contiguous()
    idx32 = p.idx.to(torch.int32)
    lo, hi = dm.quasistatic_bound_rows_batch(X, idx32, off, rel=p.kind == "rel")
    rows = dict(u_lo=lo, u_hi=hi) if p.kind == "abs" else dict(du_lo=lo, du_hi=hi)
    act = torch.zeros((B, T, m), dtype=torch.float64, device="cuda")
    out = {}

    def passes():
        for b in range(B):
            p.smooth(b if distinct else 0, out=outs[b])

    # the same passes as one launch: problem b's trajectory, seed and std_u from device tensors
    U = p.u_trj.unsqueeze(0).repeat(B, 1, 1).contiguous()
    std_dev = dev.to_dev(np.tile(np.asarray(p.std_u, float), (B, 1)))
    seed_dev = torch.as_tensor(np.array([b if distinct else 0 for b in range(B)], dtype=np.int64)).cuda()
    bout = dict(sums=sums, At=AT, Bt=BT, ct=CT, info=info)

    def batched_pass():
        dm.smooth_rng_batch(p.w.mode, X, U, p.N, std_dev, seed_dev, 1, out=bout)

    def descent():
        act.zero_()
        out.update(dm.quasistatic_box_descent_batch(AT, BT, CT, p.Q, p.Qd, p.R, XD, X0, max_iter=2000, eps=1e-9, act=act,
                                                    out=out or None, **rows))

    def iteration(linearise=passes):
        linearise()
        dm.quasistatic_bound_rows_batch(X, idx32, off, rel=p.kind == "rel", out=(lo, hi))
        descent()

    passes()
    want = {k: v.clone() for k, v in bout.items()}
    d, s, i = event_ms(descent), event_ms(passes), event_ms(iteration)
    if not dm.smooth_batch_supported(p.w.mode):          # the general kernel has no batched sample pass
        sb = ib = same = None
    else:
        sb, ib = event_ms(batched_pass), event_ms(lambda: iteration(batched_pass))
        same = all(torch.equal(bout[k], want[k]) for k in bout)    # the one launch wrote the bits of the B calls
    bad = int((out["info"][:, 0] != 0).sum().item() + (out["info"][:, 2] != 0).sum().item())
    return d, s, i, bad, int(out["info"][:, 1].max().item()), sb, ib, same


def main():
    args = [v for v in sys.argv[1:] if not v.startswith("--")]
    name = args[0] if args else "planar_hand"
    Bs = [1, 8, 64, 256, 512]
    if "--B" in sys.argv:
        Bs = [int(v) for v in sys.argv[sys.argv.index("--B") + 1].split(",")]
        args = [v for v in args if v != sys.argv[sys.argv.index("--B") + 1]]
        name = args[0] if args else "planar_hand"
    p = Problem(name)
    sd, si, info, cost = time_single(p)
    print("%s T=%d N=%d %s bounds; ms as median [min .. max] of %d" % (name, p.T, p.N, p.kind, REPS))
    print("single   descent %s   iteration %s   info %s cost %.6f" % (fmt(sd), fmt(si), info, cost), flush=True)
    if "--single-only" in sys.argv:
        return
    md, mi = float(np.median(sd)), float(np.median(si))
    for B in Bs:
        d, s, i, bad, itmax, sb, ib, same = time_batch(p, B, "--distinct" in sys.argv)
        print("B=%-4d descent %s (B x single %9.3f)   sample passes %s   iteration %s (B x single %9.3f)   "
              "%8.0f problem-iterations/s   failed %d, most iterations %d"
              % (B, fmt(d), B * md, fmt(s), fmt(i), B * mi, B / (float(np.median(i)) * 1e-3), bad, itmax), flush=True)
        if sb is None:
            print("       batched sample pass: not served for this model (general kernel)", flush=True)
            continue
        print("       batched sample pass %s   iteration with it %s   %8.0f problem-iterations/s   bits equal: %s"
              % (fmt(sb), fmt(ib), B / (float(np.median(ib)) * 1e-3), same), flush=True)


if __name__ == "__main__":
    main()
