#!/usr/bin/env python3
"""Sample counts of the uniform-geometry kernel (a -DIRS_UG_STAMPS build of csrc/smooth_ug.hip, tools/ug_variants.sh),
on the launch tests/tools/ug_stamps.py times: per launch, the samples that park after the first attempt, that the
flush's iterations settle, and that enter the dual steps (irs_debug_ug_counts).  python tests/tools/ug_counts.py [N]"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import irs_mpc_amd as amd  # noqa: E402
from irs_mpc_amd import _lib, device as dev  # noqa: E402
from irs_mpc_amd._lib import SMOOTH_ZERO_ORDER_B  # noqa: E402
from oracle import irs_oracle as orc  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
RUNS = 20           # every launch sees the same samples: the counts are the sum over RUNS launches, divided
HAND = orc.PlanarHandOracle
sys_o = HAND(0.1)
x0 = HAND.pack([0.0, 0.35, 0.0], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])
T = 50
u_trj = np.tile(x0[sys_o.indices_u_into_x], (T, 1))
x_trj = orc.rollout(sys_o, x0, u_trj)
xd, ud = dev.to_dev(x_trj), dev.to_dev(u_trj)
g = torch.Generator(device="cuda").manual_seed(1234)
du = 0.3 * torch.randn((T, N, 4), generator=g, device="cuda", dtype=torch.float32)
dm = amd.PlanarHandDynamics(0.1).dm()
plan = dev.SmoothPlan(dm, SMOOTH_ZERO_ORDER_B, xd, ud, dx=None, du=du, fuse=True)
lib = ctypes.CDLL(_lib.LIB_PATH)
cnt = (ctypes.c_uint * 3)()
plan.run()
torch.cuda.synchronize()
lib.irs_debug_ug_counts(cnt, 1)         # read and reset
for _ in range(RUNS):
    plan.run()
torch.cuda.synchronize()
rc = lib.irs_debug_ug_counts(cnt, 0)
per = [c / RUNS for c in cnt]
print("rc %d  per launch of %d samples: parked %.0f (%.2f %%), settled by the flush's iterations %.0f, entered the dual steps %.0f (%.3f %%)" % (
    rc, T * N, per[0], 100.0 * per[0] / (T * N), per[1], per[2], 100.0 * per[2] / (T * N)))
