"""Every way into the sample pass launches the same kernel on the same arguments (csrc/smooth_api.hip: one call
record, one checked path): per kernel family, the positional entries, irs_smooth_run, the two-step form and the Python
wrappers are compared with each other.

Shapes: the families of oracle/smooth_cases.py (CASES) at their smallest listed N with T = 2, plus -- where the family
has that form -- an N that is no multiple of 64 planned on two or more workgroups per time step.

How equal.  Forms that reach one launch are compared BIT FOR BIT (two calls of one entry are bit-identical in every
family, on this library and on the one before the entries moved: the sums are added in a fixed order, without float
atomics).  The fused launch against accumulate + finalize is two instantiations of one template, which the compiler
may contract differently: the tolerance of test_gpu_parity.py::test_fused_launch_equals_two_stage (rtol 1e-5, atol
1e-6, for the sums 1e-6 of their largest entry), with `info` equal and (A, B, c) compared where info == 0 -- a failed
solve (N = 1: the Gram matrix is singular) defines no outputs.  The batched entry against the single one is
tests/test_smooth_batch_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import smooth_cases as sc

pytestmark = pytest.mark.gpu

SEED, ITER, STD = 11, 2, 0.05
OUTS = ("sums", "At", "Bt", "ct", "info")

# (family, model, mode, N, sources, general kernel, at least this many workgroups per time step)
SHAPES = [
    (sc.LIGHT, "pendulum", sc.ZERO_ORDER_AB, 1, "s", False, 1),            # the single 1024-thread workgroup
    (sc.LIGHT, "pendulum", sc.ZERO_ORDER_AB, 1025, "s", False, 1),
    (sc.LIGHT, "pendulum", sc.ZERO_ORDER_B, 257, "r", False, 1),           # 256-thread workgroups: device-drawn
    (sc.LIGHT, "pendulum", sc.ZERO_ORDER_AB, 1025, "r", False, 2),
    (sc.HEAVY, "bicycle", sc.ZERO_ORDER_AB, 1, "sr", False, 1),
    (sc.HEAVY, "quadrotor", sc.FIRST_ORDER, 2049, "sr", False, 3),
    (sc.GRAM, "quadrotor", sc.ZERO_ORDER_AB, 1, "sr", False, 1),
    (sc.GRAM, "three_cart", sc.ZERO_ORDER_AB, 1025, "sr", False, 2),
    (sc.WAVE_DEALT, "box_pivot", sc.ZERO_ORDER_B, 1, "sr", False, 1),
    (sc.WAVE_DEALT, "box_pivot", sc.FIRST_ORDER, 257, "sr", False, 2),
    (sc.PARKED, "planar_hand", sc.ZERO_ORDER_B, 1, "sr", True, 1),         # the exact hand with IRS_UG=0, read per call
    (sc.PARKED, "planar_hand", sc.FIRST_ORDER, 449, "sr", True, 2),
    (sc.UG, "planar_hand", sc.ZERO_ORDER_B, 1, "sr", False, 1),
    (sc.UG, "planar_hand", sc.FIRST_ORDER, 513, "sr", False, 2),
]
T = 2


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


_dm = {}


def device_model(amd, model):
    if model not in _dm:
        cls, args, kw, _ = sc.SYSTEMS[model]
        _dm[model] = getattr(amd, cls)(*args, **kw).dm()
    return _dm[model]


class general_kernel:
    """IRS_UG=0 for the calls inside (read per call by the planner and by the launch)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.before = os.environ.get("IRS_UG")
        if self.on:
            os.environ["IRS_UG"] = "0"

    def __exit__(self, *a):
        if self.on:
            if self.before is None:
                os.environ.pop("IRS_UG", None)
            else:
                os.environ["IRS_UG"] = self.before


def same_bits(a, b):
    """Bit for bit (NaNs included): the bytes of two tensors of one shape and type."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                                                      b.contiguous().view(torch.uint8))


class Problem:
    """One shape's inputs, a workspace of its own for the raw entries, and the raw entries themselves."""

    def __init__(self, amd, model, mode, N):
        from irs_mpc_amd import device as dev
        self.dev, self.dm, self.mode, self.N = dev, device_model(amd, model), mode, N
        self.lib = self.dm.lib
        _, self.n, self.m, contact = sc.MODELS[model]
        self.u_only = mode == sc.ZERO_ORDER_B or (mode == sc.FIRST_ORDER and contact)
        x, u = sc.nominal(model, T)
        self.x, self.u = dev.to_dev(x), dev.to_dev(u)
        g = np.random.default_rng(1000 * N + mode)
        self.dx = None if self.u_only else dev.to_dev(STD * g.standard_normal((T, N, self.n)), dev.F32)
        self.du = dev.to_dev(STD * g.standard_normal((T, N, self.m)), dev.F32)
        self.std_x = None if self.u_only else [STD] * self.n
        self.std_u = [STD * (1 + 0.1 * j) for j in range(self.m)]
        self.P = self.dm.sums_len(mode)
        self.ws = torch.empty((self.lib.irs_smooth_workspace_bytes(self.dm.model_id, mode, T, N),), dtype=torch.uint8,
                              device="cuda")
        dev.check(self.lib.irs_workspace_init(self.ws.data_ptr(), self.ws.numel(), dev._stream()), "irs_workspace_init")
        self.head = (self.dm.model_id, self.dm._p, self.dm._np, mode, T, N, self.x.data_ptr(), self.u.data_ptr())

    def outputs(self, fused=True):
        o = dict(sums=torch.full((T, self.P), np.nan, dtype=torch.float64, device="cuda"))
        if fused:
            n, m = self.n, self.m
            o.update(At=torch.full((T, n, n), np.nan, dtype=torch.float64, device="cuda"),
                     Bt=torch.full((T, n, m), np.nan, dtype=torch.float64, device="cuda"),
                     ct=torch.full((T, n), np.nan, dtype=torch.float64, device="cuda"),
                     info=torch.full((T,), -7, dtype=torch.int32, device="cuda"))
        return o

    def counters_are_zero(self, ws=None):
        ws = self.ws if ws is None else ws
        return int(ws[:4 * T].view(torch.int32).abs().sum().item()) == 0

    def finish(self, rc, what, o):
        self.dev.check(rc, what)
        torch.cuda.synchronize()
        assert self.counters_are_zero(), what
        return o

    def samples(self, drawn):
        if drawn:
            sx = None if self.std_x is None else self.dev.dbl_array(self.std_x)
            return (sx, self.dev.dbl_array(self.std_u), SEED, ITER)
        return (None if self.dx is None else self.dx.data_ptr(), self.du.data_ptr())

    def positional(self, drawn, fused):
        o = self.outputs(fused)
        name = "irs_smooth" + ("" if fused else "_accumulate") + ("_rng" if drawn else "")
        args = self.head + self.samples(drawn) + ((0,) if drawn and not fused else ()) + tuple(o[k].data_ptr() for k in o)
        rc = getattr(self.lib, name)(*args, self.ws.data_ptr(), self.ws.numel(), self.dev._stream())
        return self.finish(rc, name, o)

    def by_struct(self, drawn, fused):
        from irs_mpc_amd import _lib
        o = self.outputs(fused)
        c = _lib.SmoothCall()
        self.dm.fill_call(c)
        c.mode, c.T, c.N, c.n_total = self.mode, T, self.N, self.N
        c.x_trj, c.u_trj = self.x.data_ptr(), self.u.data_ptr()
        if drawn:
            c.use_rng, c.seed, c.iter = 1, SEED, ITER
            for i, v in enumerate(self.std_x or []):
                c.std_x[i] = v
            for i, v in enumerate(self.std_u):
                c.std_u[i] = v
        else:
            c.dx, c.du = (None if self.dx is None else self.dx.data_ptr()), self.du.data_ptr()
        for k in o:
            setattr(c, k, o[k].data_ptr())
        c.workspace, c.workspace_bytes = self.ws.data_ptr(), self.ws.numel()
        return self.finish(self.lib.irs_smooth_run(ctypes.byref(c), self.dev._stream()), "irs_smooth_run", o)

    def finalize(self, sums, with_workspace):
        o = self.outputs()
        o["sums"] = sums
        args = self.head[:5] + (self.N, self.x.data_ptr(), self.u.data_ptr()) + tuple(o[k].data_ptr() for k in OUTS)
        if with_workspace:
            rc = self.lib.irs_smooth_finalize_ws(*args, self.ws.data_ptr(), self.ws.numel(), self.dev._stream())
        else:
            rc = self.lib.irs_smooth_finalize(*args, self.dev._stream())
        return self.finish(rc, "irs_smooth_finalize", o)

    def wrappers(self, drawn):
        """(fused, sums alone) of DeviceModel.smooth* and of SmoothPlan, each checked to leave the counters zero."""
        dm, mode, x, u = self.dm, self.mode, self.x, self.u
        if drawn:
            fused = dm.smooth_rng(mode, x, u, self.N, self.std_x, self.std_u, SEED, ITER)
            alone = dm.smooth_accumulate_rng(mode, x, u, self.N, self.std_x, self.std_u, SEED, ITER)
            kw = dict(rng=dict(N=self.N, std_x=self.std_x, std_u=self.std_u, seed=SEED, iter=ITER))
        else:
            fused = dm.smooth(mode, x, u, self.dx, self.du)
            alone = dm.smooth_accumulate(mode, x, u, self.dx, self.du)
            kw = dict(dx=self.dx, du=self.du)
        plan, plan_alone = self.dev.SmoothPlan(dm, mode, x, u, **kw), self.dev.SmoothPlan(dm, mode, x, u, fuse=False, **kw)
        got = [fused, dict(sums=alone), plan.run(), dict(sums=plan_alone.run())]
        torch.cuda.synchronize()
        assert self.counters_are_zero(plan.ws) and self.counters_are_zero(plan_alone.ws)
        return got


@pytest.mark.parametrize("family,model,mode,N,sources,general,min_nblk", SHAPES,
                         ids=["%s-%s-m%d-N%d-%s" % (s[0], s[1], s[2], s[3], s[4]) for s in SHAPES])
def test_every_entry_form_gives_the_same_results(amd, family, model, mode, N, sources, general, min_nblk):
    with general_kernel(general):
        p = Problem(amd, model, mode, N)
        for drawn in [src == "r" for src in sources]:
            geom = p.dm.smooth_geometry(mode, T, N, drawn)
            assert geom["family"] == family and geom["nblk"] >= min_nblk, geom
            assert family != sc.LIGHT or geom["block"] == (256 if drawn else 1024)
            run = p.by_struct(drawn, True)
            # two calls of one entry; the positional entry; the Python wrappers: one launch, bit for bit
            again, pos = p.by_struct(drawn, True), p.positional(drawn, True)
            alone, pos_alone = p.by_struct(drawn, False), p.positional(drawn, False)
            fused_w, alone_w, plan, plan_alone = p.wrappers(drawn)
            for k in OUTS:
                assert same_bits(again[k], run[k]), ("irs_smooth_run twice", k)
                assert same_bits(pos[k], run[k]), ("positional", k)
                assert same_bits(fused_w[k], run[k]), ("DeviceModel", k)
                assert same_bits(plan[k], run[k]), ("SmoothPlan", k)
            for name, got in (("positional", pos_alone), ("DeviceModel", alone_w), ("SmoothPlan", plan_alone)):
                assert same_bits(got["sums"], alone["sums"]), (name, "sums alone")
            # accumulate, then the solve -- reading the nominal steps the accumulate left in the workspace, and without
            two = [p.finalize(alone["sums"], True), p.finalize(alone["sums"], False)]
            ok = run["info"] == 0
            scale = float(run["sums"].abs().max().item())
            for t in two:
                worst = {k: float((t[k][ok] - run[k][ok]).abs().max().item()) if bool(ok.any()) else 0.0
                         for k in ("At", "Bt", "ct")}
                worst["sums"] = float((alone["sums"] - run["sums"]).abs().max().item()) / max(scale, 1e-300)
                print("%s %s drawn=%d: fused vs two-step, max |difference| %s (sums: of their largest entry); %d of %d "
                      "steps solved" % (family, model, drawn, worst, int(ok.sum().item()), T))
                assert torch.equal(t["info"], run["info"])
                np.testing.assert_allclose(alone["sums"].cpu().numpy(), run["sums"].cpu().numpy(), rtol=1e-5,
                                           atol=1e-6 * scale)
                for k in ("At", "Bt", "ct"):
                    np.testing.assert_allclose(t[k][ok].cpu().numpy(), run[k][ok].cpu().numpy(), rtol=1e-5, atol=1e-6)
        ws = p.dm._ws.get((mode, p.x.device))
        assert ws is not None and p.counters_are_zero(ws)
