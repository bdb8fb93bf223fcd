"""irs_tvlqr_plan_within_bounds (csrc/iterate.hip: plan_check16_kernel<NN> for every NN = 1 .. 16, plan_check_kernel
for n > 16, for closed loops beyond LDS and with more tails than one pass holds) on the cases of oracle/plan_cases.py,
admitted by tests/test_plan_check_cpu.py: the flag equals the statement's answer on bounds that exactly one tail, one
step or one ulp violates.  The entry's argument checks, and the info row of the fused loop around the flag.

The tests launch the entry and read the flag, nothing else.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import plan_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


def device_flags(cs):
    """The flag of every case of one problem: the problem's arrays go up once, a case's own array and its four bound
    vectors per case; every flag word is pre-set to -7 and all are read back together."""
    from irs_mpc_amd import _lib, device as dev
    lib = _lib.load()
    c0 = cs[0]
    n, m, T = c0["n"], c0["m"], c0["T"]
    base = {k: dev.to_dev(np.array(v)) for k, v in pc.problem(n, m, T, c0["family"], c0["seed"]).items()}
    flags = torch.full((len(cs),), -7, dtype=torch.int32, device="cuda")
    keep = []
    for q, c in enumerate(cs):
        d = dict(base)
        d.update({k: dev.to_dev(np.array(v)) for k, v in c["override"].items()})
        b = [dev.to_dev(np.array(v)) for v in c["bounds"]]
        keep.append((d, b))
        _lib.check(lib.irs_tvlqr_plan_within_bounds(n, m, T, *[d[k].data_ptr() for k in pc.DATA_KEYS],
                                                    *[v.data_ptr() for v in b], flags[q:].data_ptr(), dev._stream()),
                   "irs_tvlqr_plan_within_bounds")
    return flags.cpu().numpy()


@pytest.mark.parametrize("key", list(pc.SHAPES), ids=["%d-%d-%d" % key for key in pc.SHAPES])
def test_flag_equals_the_statement(amd, key):
    n, m, T = key
    wrong = []
    for fam in pc.FAMILIES:
        cs = pc.cases(n, m, T, fam)
        got = device_flags(cs)
        print("%s %s: %d cases on the %s kernel, %d with flag 1" % (key, fam, len(cs), pc.SHAPES[key],
                                                                   int((got == 1).sum())))
        wrong += ["flag %d: %s" % (g, pc.describe(c)) for g, c in zip(got, cs) if g != c["want"]]
    assert not wrong, "\n".join(wrong)


def test_argument_checks_leave_the_flag_alone(amd):
    """n = 33, m = 17, T = 0 and a null bound pointer: an error code each, and the flag still -7."""
    from irs_mpc_amd import _lib, device as dev
    lib = _lib.load()
    n, m, T = 2, 1, 5
    d = {k: dev.to_dev(np.array(v)) for k, v in pc.problem(n, m, T, "exact").items()}
    # bound vectors long enough for any size the entry might read before it refuses
    b = [dev.to_dev(np.full(64, v)) for v in (-np.inf, np.inf, -np.inf, np.inf)]
    flag = torch.full((1,), -7, dtype=torch.int32, device="cuda")

    def call(n_, m_, T_, bounds):
        return lib.irs_tvlqr_plan_within_bounds(n_, m_, T_, *[d[k].data_ptr() for k in pc.DATA_KEYS], *bounds,
                                                flag.data_ptr(), dev._stream())

    ptrs = [v.data_ptr() for v in b]
    assert call(33, m, T, ptrs) != 0
    assert call(n, 17, T, ptrs) != 0
    assert call(n, m, 0, ptrs) != 0
    for q in range(4):
        assert call(n, m, T, ptrs[:q] + [None] + ptrs[q + 1:]) != 0, q
    torch.cuda.synchronize()
    assert int(flag.item()) == -7
    assert call(n, m, T, ptrs) == 0                         # and the same call with everything in place runs
    torch.cuda.synchronize()
    assert int(flag.item()) == 0


# the steer limits of the fused-loop test: the problem's own, which the first unbounded descent's plans exceed by a
# factor of several hundred (the oracle: |steer| up to 381 against 0.785), and 1e4, which none of the three descents'
# plans reaches (the oracle: 548 at most, and no other state or input above 1735)
STEER_LIMITS = (np.pi / 4, 1e4)


def test_fused_loop_info_row_follows_the_flag(amd):
    """irs_iterate driven directly (IterateCall filled as IrsLqr._iterate_fused fills it) on the exact bicycle, T = 40,
    3 descents, once per steer limit.  Where row[2] == 0 the bounded kernel behind the run flag touched nothing:
    row[3:8] == 0 and the descent equals dm.tvlqr_descent on the exact linearisation around the previous history
    entry, bit for bit.  Where row[2] == 1: it ran on chip (row[6] == 0), converged (row[5] == 0), and the realised
    steer keeps the limit to 1e-6.  Both values of row[2] occur."""
    from irs_mpc_amd import _lib, device as dev
    from examples.problems import bicycle
    T, n_desc = 40, 3
    seen = set()
    for steer in STEER_LIMITS:
        sysd, params, _, _, _ = bicycle(T)
        params.xbound = [-np.array([1e4, 1e4, 1e4, 1e4, steer]), np.array([1e4, 1e4, 1e4, 1e4, steer])]
        sol = amd.IrsLqrExact(sysd, params)
        sol.verbose = False
        n, m, dm = sol.dim_x, sol.dim_u, sol._dm
        c = _lib.IterateCall()
        dm.fill_call(c)
        c.mode, c.T, c.N, c.n_descents = _lib.ITERATE_EXACT, T, 0, n_desc
        c.Q, c.Qd, c.R, c.xd_trj = (t_.data_ptr() for t_ in (sol._Q, sol._Qd, sol._R, sol._xd))
        c.alpha_R = 0.5
        box = sol._box_bounds()
        c.xlo, c.xhi, c.ulo, c.uhi = (b.data_ptr() for b in box)
        c.qp_rho, c.qp_max_iter, c.qp_eps = 10.0, 5000, 1e-8
        x0d, u0d = dev.to_dev(np.asarray(sol.x_trj, float)), dev.to_dev(np.asarray(sol.u_trj, float))
        c.x_trj0, c.u_trj0 = x0d.data_ptr(), u0d.data_ptr()
        xh = torch.empty((n_desc, T + 1, n), dtype=dev.F64, device="cuda")
        uh = torch.empty((n_desc, T, m), dtype=dev.F64, device="cuda")
        ch = torch.empty((n_desc,), dtype=dev.F64, device="cuda")
        ih = torch.zeros((n_desc, 8), dtype=torch.int32, device="cuda")
        c.x_hist, c.u_hist, c.cost_hist, c.info_hist = xh.data_ptr(), uh.data_ptr(), ch.data_ptr(), ih.data_ptr()
        need = dm.lib.irs_iterate_scratch_bytes(dm.model_id, _lib.ITERATE_EXACT, T, 0)
        scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
        c.scratch, c.scratch_bytes = scratch.data_ptr(), scratch.numel()
        _lib.check(dm.lib.irs_iterate(ctypes.byref(c), None, dev._stream()), "irs_iterate")
        rows = ih.cpu().numpy()
        print("steer limit %g: info rows\n%s" % (steer, rows))
        for i in range(n_desc):
            row = rows[i]
            assert row[0] == 0 and row[1] == 0, row
            seen.add(int(row[2]))
            if row[2] == 0:
                assert (row[3:8] == 0).all(), row
                xp, up = (x0d, u0d) if i == 0 else (xh[i - 1], uh[i - 1])
                At, Bt, ct = sol._get_TV_matrices_dev(xp.contiguous(), up.contiguous())
                o = dm.tvlqr_descent(At, Bt, ct, sol._Q, sol._Qd, sol._R, sol._xd, xp[0].contiguous(), alpha_R=0.5)
                assert torch.equal(o["x_new"], xh[i]) and torch.equal(o["u_new"], uh[i]), i
            else:
                assert row[2] == 1 and row[6] == 0 and row[5] == 0, row
                worst = float(xh[i, 1:, 4].abs().max().item())
                print("descent %d: realised |steer| %.9g against %.9g" % (i, worst, steer))
                assert worst <= steer + 1e-6
    assert seen == {0, 1}, seen
