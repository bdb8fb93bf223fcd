#!/usr/bin/env python3
"""The bounded TV-LQR descent with a fixed and with the adaptive ADMM penalty (csrc/boxqp.hip, irs_admm_settings).

    python tools/time_box_adaptive.py

Two whole descents (T warm-started tail QPs, one launch each): the easy bicycle at T = 100 (steer limit, the
class's defaults rho = 10, max_iter = 5000) and the quadrotor at T = 100 with body-rate limits (rho = 1,
max_iter = 20000: the settings of tests/test_box_horizon_gpu.py; records in HBM).  Per form: median, minimum and
maximum ms of 5 launches in this process, most iterations of a tail, tails at the limit, ADMM iterations of all
tails, factorisations, final rho.  The fixed form's iteration total comes from the adaptive kernel with a trigger
no ratio reaches (its rho never moves: the same iterates); its time from the fixed kernel itself."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from irs_mpc_amd import _lib, device as dev                    # noqa: E402
from time_box_horizon import problem                           # noqa: E402

REPS = 5


def timed(run):
    run()                                                       # warm up (workspace allocation)
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o = run()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return o, float(np.median(ms)), min(ms), max(ms)


def counted_fixed(dm, prob, box, rho, max_iter):
    """The fixed penalty through the adaptive kernel (trigger out of reach), for its iteration total."""
    T = prob[0].shape[0]
    x_new = torch.empty((T + 1, dm.n), dtype=dev.F64, device="cuda")
    u_new = torch.empty((T, dm.m), dtype=dev.F64, device="cuda")
    info = torch.empty((3,), dtype=torch.int32, device="cuda")
    adapt = torch.empty((3,), dtype=dev.F64, device="cuda")
    ws = dm._box_workspace(T, False, x_new.device)
    st = _lib.admm_settings(rho, 1.6, max_iter, 1e-8, adaptive=True, trigger=1e300)
    _lib.check(dm.lib.irs_tvlqr_box_descent_set(dm.model_id, dm._p, dm._np, T, *[a.data_ptr() for a in prob[:6]], 0.5,
                                                prob[6].data_ptr(), prob[7].data_ptr(), *[b.data_ptr() for b in box],
                                                ctypes.byref(st), x_new.data_ptr(), u_new.data_ptr(), info.data_ptr(),
                                                adapt.data_ptr(), *dev._ws_args(ws), dev._stream()),
               "irs_tvlqr_box_descent_set")
    return info.cpu().numpy(), adapt.cpu().numpy()


def main():
    for name, T, rho, max_iter in (("bicycle", 100, 10.0, 5000), ("quadrotor", 100, 1.0, 20000)):
        sol, prob, box = problem(name, T)
        dm = sol._dm
        kw = dict(alpha_R=0.5, rho=rho, max_iter=max_iter, eps=1e-8)
        of, med, lo, hi = timed(lambda: dm.tvlqr_box_descent(*prob, *box, **kw))
        info, adapt = counted_fixed(dm, prob, box, rho, max_iter)
        assert np.array_equal(info, of["info"].cpu().numpy()), (info, of["info"])
        print("%-9s T=%d fixed rho=%-4g  %8.2f ms (min %.2f, max %.2f)  most iterations %5d, tails at the limit %d, "
              "iterations %7d, factorisations %2d" % (name, T, rho, med, lo, hi, info[1], info[2], adapt[2], adapt[0]))
        oa, med, lo, hi = timed(lambda: dm.tvlqr_box_descent(*prob, *box, adaptive_rho=True, **kw))
        info, adapt = oa["info"].cpu().numpy(), oa["adapt"].cpu().numpy()
        print("%-9s T=%d adaptive from %-4g %7.2f ms (min %.2f, max %.2f)  most iterations %5d, tails at the limit %d, "
              "iterations %7d, factorisations %2d, final rho %.4g; max |u - u_fixed| %.2e"
              % (name, T, rho, med, lo, hi, info[1], info[2], adapt[2], adapt[0], adapt[1],
                 (oa["u_new"] - of["u_new"]).abs().max().item()))


if __name__ == "__main__":
    main()
