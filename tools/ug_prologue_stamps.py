#!/usr/bin/env python3
"""Phase stamps of the uniform-geometry kernel's prologue (a -DIRS_UG_STAMPS build of csrc/smooth_ug.hip named by
IRS_HIP_LIB; the workload of tests/tools/ug_stamps.py): per workgroup, s_memtime ticks since its own start at

    geometry done (the barrier behind the f32 and f64 geometry) / table done / wave 0's first fresh trip done /
    the nominal wave's f64 geometry done / end,

and the time from "table done" to the end of wave 0's first trip.  python tools/ug_prologue_stamps.py [N]"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import irs_mpc_amd as amd  # noqa: E402
from irs_mpc_amd import _lib, device as dev  # noqa: E402
from irs_mpc_amd._lib import SMOOTH_ZERO_ORDER_B  # noqa: E402
from oracle import irs_oracle as orc  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
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
for _ in range(20):
    plan.run()
torch.cuda.synchronize()
lib = ctypes.CDLL(_lib.LIB_PATH)
nwg = 250
buf = (ctypes.c_ulonglong * (nwg * 12))()
rc = lib.irs_debug_ug_stamps(buf, nwg)
st = np.array(buf, dtype=np.uint64).reshape(nwg, 12).astype(np.int64)
print("rc", rc, " N", N, " ticks since the workgroup's own start; median / min / max")


def row(name, v):
    if len(v):
        print("%-34s median %7d  min %7d  max %7d  (n=%d)" % (name, np.median(v), v.min(), v.max(), len(v)))


for k, name in ((1, "geometry done"), (2, "table done"), (6, "wave 0 first trip done"),
                (10, "nominal wave f64 geometry done"), (5, "end")):
    ok = st[:, k] > 0
    row(name, (st[:, k] - st[:, 0])[ok])
ok = (st[:, 6] > 0) & (st[:, 2] > 0)
row("table done -> first trip done", (st[:, 6] - st[:, 2])[ok])
