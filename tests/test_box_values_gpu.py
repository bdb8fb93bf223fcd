"""The any-size bounded TV-LQR kernels (csrc/boxqp_values.hip): the cases of tests/helpers/box_values_cases.py, admitted
by tests/test_box_values_cpu.py, through the public solve_tvlqr; resumed tails against the oracle's MPC loop; the stepped
bounded descent of a TorchDynamicalSystem (IrsLqrParameters.qp_model_free) on a system with no compiled size and beside
a compiled one; reproducibility, stale workspaces, the header guard, the iteration limit and the flags.

The figures are the suite's own for the compiled kernel (tests/test_boxqp_cases_gpu.py): KKT certificate below 1e-5
and the oracle's ADMM solution at atol 1e-7 for a single QP; rtol 1e-5 / atol 1e-6 against orc.local_descent_box for a
descent (test_three_cart_box_descent_vs_oracle).
"""
import numpy as np
import pytest
import torch

from oracle import boxqp_cases as bc
from oracle import irs_oracle as orc
from tests.helpers import box_values_cases as vc

pytestmark = pytest.mark.gpu

DESCENT_TOL = dict(rtol=1e-5, atol=1e-6)


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()     # fails loudly if the HIP library is missing
    return irs_mpc_amd


def report(what, got, want, **tol):
    """Print the figure, then assert it."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    err = np.abs(got - want)
    print("%s: max abs err %.3g, worst err / (atol + rtol |want|) %.3g" % (
        what, err.max(), (err / np.maximum(tol.get("atol", 0) + tol["rtol"] * np.abs(want), 1e-300)).max()))
    np.testing.assert_allclose(got, want, err_msg=what, **tol)


def certify(c, xs, us, xo, uo):
    res = bc.kkt(c, xs, us)
    print("%s KKT residuals (dynamics, box, stationarity, multiplier sign):" % c["id"], res)
    assert max(res) < 1e-5, res
    report("u* vs oracle ADMM", us, uo, rtol=0, atol=1e-7)
    report("x* vs oracle ADMM", xs, xo, rtol=0, atol=1e-7)


def dev_problem(c):
    from irs_mpc_amd import device as dev
    return [dev.to_dev(c[k]) for k in ("At", "Bt", "ct", "Q", "Qd", "R", "xd")]


# ------------------------------------------------------------------------------------------------ 1, 2: one QP
@pytest.mark.parametrize("cid", list(vc.CASES))
def test_case_through_solve_tvlqr(amd, cid):
    """Sizes with no compiled kernel through the public solve_tvlqr (which raises unless info[0] == 0 and
    info[2] == 0)."""
    c = vc.case(cid)
    xo, uo, it = vc.reference(cid)
    assert it < 40000
    xs, us = amd.solve_tvlqr(c["At"], c["Bt"], c["ct"], c["Q"], c["Qd"], c["R"], c["x0"], c["xd"], None,
                             x_bound_abs=np.stack([c["x_lo"], c["x_hi"]]), u_bound_abs=np.stack([c["u_lo"], c["u_hi"]]),
                             rho=c["rho"], eps=1e-10, max_iter=40000)
    certify(c, xs, us, xo, uo)


def test_compiled_size_through_the_any_size_kernel(amd):
    """p62-B2, which solve_tvlqr hands to the compiled (6, 2) kernel, through device.box_values_solve: both are held
    to the oracle at 1e-7, hence lie within 2e-7 of each other.  No bit equality is claimed."""
    from irs_mpc_amd import device as dev
    c = bc.case("p62-B2")
    xo, uo, it = bc.reference("p62-B2")
    assert it < 40000
    o = dev.box_values_solve(*dev_problem(c), dev.to_dev(c["x0"]), *[dev.to_dev(c[k]) for k in ("x_lo", "x_hi", "u_lo", "u_hi")],
                             rho=c["rho"], relax=bc.RELAX, max_iter=40000, eps=1e-10)
    info = o["info"].cpu().numpy()
    assert info[0] == 0 and info[2] == 0, info
    certify(c, o["x_star"].cpu().numpy(), o["u_star"].cpu().numpy(), xo, uo)


# ------------------------------------------------------------------------------------------------ 3, 6: resumed tails
def resumed_descent(c, bounds, workspace=None, max_iter=None):
    """begin, then T tails with the linear model as the plant: torch matmuls between the launches, no host read."""
    from irs_mpc_amd import device as dev
    At, Bt, ct = (dev.to_dev(c[k]) for k in ("At", "Bt", "ct"))
    T, n, m = c["T"], At.shape[1], Bt.shape[2]
    h = dev.box_values_begin(*dev_problem(c), *[dev.to_dev(b) for b in bounds], rho=vc.QP["rho"], workspace=workspace)
    x = torch.empty((T + 1, n), dtype=dev.F64, device="cuda")
    u = torch.empty((T, m), dtype=dev.F64, device="cuda")
    x[0] = dev.to_dev(c["x0"])
    for t in range(T):
        dev.box_values_tail(h, t, x[t], max_iter or vc.QP["max_iter"], vc.QP["eps"], u_t=u[t])
        x[t + 1] = At[t] @ x[t] + Bt[t] @ u[t] + ct[t]
    return x.cpu().numpy(), u.cpu().numpy(), h["info"].cpu().numpy()


@pytest.mark.parametrize("cid", vc.RESUMED)
def test_resumed_tails_vs_oracle_descent(amd, cid):
    c = vc.case(cid)
    bounds, xo, uo, iters = vc.resumed_reference(cid)
    assert max(iters) < vc.QP["max_iter"], iters
    x, u, info = resumed_descent(c, bounds)
    assert info[0] == 0 and info[2] == 0 and 0 < info[1] < vc.QP["max_iter"], info
    report("u_new vs oracle", u, uo, **DESCENT_TOL)
    report("x_new vs oracle", x, xo, **DESCENT_TOL)
    lo, hi = bounds[2], bounds[3]
    assert (u >= lo - 1e-9).all() and (u <= hi + 1e-9).all()
    assert min(np.abs(u - lo).min(), np.abs(u - hi).min()) < 1e-9                  # the u bound is active
    # the same descent again: identical bits
    x2, u2, info2 = resumed_descent(c, bounds)
    np.testing.assert_array_equal(x, x2)
    np.testing.assert_array_equal(u, u2)
    np.testing.assert_array_equal(info, info2)


def test_stale_workspace_is_not_read(amd):
    """A (3, 2) problem in a workspace the (32, 16) one used last == the same in a freshly zeroed buffer, bit for bit."""
    from irs_mpc_amd import _lib
    lib = _lib.load()
    big, small = vc.case("s32x16-B2"), vc.case("s3x2-B2")
    nbytes = lib.irs_box_values_workspace_bytes(32, 16, 12)
    assert nbytes >= lib.irs_box_values_workspace_bytes(3, 2, 12)
    used = torch.empty((nbytes,), dtype=torch.uint8, device="cuda")
    resumed_descent(big, vc.constant_bounds(big), workspace=used)
    b = vc.constant_bounds(small)
    xa, ua, ia = resumed_descent(small, b, workspace=used)
    xb, ub, ib = resumed_descent(small, b, workspace=torch.zeros((nbytes,), dtype=torch.uint8, device="cuda"))
    assert ia[0] == 0 and ia[2] == 0, ia
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(ua, ub)
    np.testing.assert_array_equal(ia, ib)


# ------------------------------------------------------------------------------------------------ 7: the guard
def test_tail_refuses_a_workspace_that_was_not_begun(amd):
    from irs_mpc_amd import _lib, device as dev
    c = vc.case("s3x2-B2")
    T, n, m = c["T"], 3, 2
    b = [dev.to_dev(v) for v in vc.constant_bounds(c)]
    ws = torch.zeros((_lib.load().irs_box_values_workspace_bytes(n, m, T),), dtype=torch.uint8, device="cuda")
    h = dev.box_values_handle(*dev_problem(c), *b, rho=10.0, workspace=ws)
    x0 = dev.to_dev(c["x0"])
    u_t = torch.full((m,), 7.0, dtype=dev.F64, device="cuda")
    xp = torch.full((T + 1, n), 7.0, dtype=dev.F64, device="cuda")
    up = torch.full((T, m), 7.0, dtype=dev.F64, device="cuda")
    dev.box_values_tail(h, 0, x0, 100, 1e-8, u_t=u_t, x_plan=xp, u_plan=up)
    assert h["info"].cpu().numpy().tolist() == [-1, 0, 0]
    assert bool((u_t == 7.0).all()) and bool((xp == 7.0).all()) and bool((up == 7.0).all())
    assert not bool(ws.any())                                  # and nothing written to the workspace
    # a header of another size is refused too
    dev.box_values_begin(*dev_problem(c), *b, rho=10.0, workspace=ws)
    c1 = vc.case("s1x1-B2")
    h1 = dev.box_values_handle(*dev_problem(c1), rho=10.0, workspace=ws)
    u1 = torch.full((1,), 7.0, dtype=dev.F64, device="cuda")
    dev.box_values_tail(h1, 0, dev.to_dev(c1["x0"]), 100, 1e-8, u_t=u1)
    assert int(h1["info"][0].item()) == -1 and float(u1.item()) == 7.0
    # the next correct begin + tail succeeds
    o = dev.box_values_solve(*dev_problem(c), x0, *b, rho=10.0, max_iter=40000, eps=1e-10, workspace=ws)
    info = o["info"].cpu().numpy()
    assert info[0] == 0 and info[2] == 0 and info[1] > 0, info
    assert bool(torch.isfinite(o["u_star"]).all())


# ------------------------------------------------------------------------------------------------ 4, 8, 9: torch systems
class Replay:
    """sampling closure that replays recorded draws (one (N,n),(N,m) pair per call)."""

    def __init__(self, dx, du):
        self.dx, self.du, self.i = dx, du, 0

    def __call__(self, x, u, it):
        i = self.i % len(self.dx)
        self.i += 1
        return self.dx[i], self.du[i]


def cartpole_solver(amd, xhi=None, uhi=None, **flags):
    from examples.torch_systems import TorchCartPole
    s = vc.cartpole_setup()
    p = amd.IrsLqrParameters()
    p.Q, p.Qd, p.R, p.x0, p.xd_trj, p.u_trj_initial = s["Q"], s["Qd"], s["R"], s["x0"], s["xd"], s["u0"]
    if xhi is not None:
        p.xbound, p.ubound = [-xhi, xhi], np.array([-uhi, uhi])
    p.qp_rho, p.qp_max_iter, p.qp_eps = vc.QP["rho"], vc.QP["max_iter"], vc.QP["eps"]
    for k, v in flags.items():
        setattr(p, k, v)
    sol = amd.IrsLqrZeroOrder(TorchCartPole(s["h"]), p, Replay(s["dx"], s["du"]))
    sol.verbose = False
    return sol, s


def test_system_with_no_compiled_size_takes_the_stepped_descent(amd):
    """TorchCartPole (4, 1): both bounds bind on the oracle's own linearisation (tests/test_box_values_cpu.py); here the
    device's descent against the oracle's on the device's own At, Bt, ct."""
    r = vc.cartpole_bounds()
    vel = vc.CARTPOLE_VELOCITY
    sol, s = cartpole_solver(amd, r["xhi"], r["uhi"], qp_model_free=True)
    x_new, u_new = sol.local_descent(sol.x_trj, sol.u_trj)
    info = sol._last["box_info"].cpu().numpy() if sol._box_used else None
    assert sol._box_used and info[0] == 0 and info[2] == 0, info
    At, Bt, ct = (sol._last[k].cpu().numpy() for k in ("At", "Bt", "ct"))
    xo, uo, iters = vc.cartpole_bounded_descent(At, Bt, ct)
    assert max(iters) < vc.QP["max_iter"], iters
    report("u_new vs oracle", u_new, uo, **DESCENT_TOL)
    report("x_new vs oracle", x_new, xo, **DESCENT_TOL)
    assert np.abs(u_new).max() == pytest.approx(r["uhi"][0], abs=1e-9)             # the u bound is met
    assert np.abs(x_new[:, vel]).max() > r["xhi"][vel] - 1e-3                       # and the velocity bound
    xn, un, _, _ = orc.local_descent(vc.NumpyCartPole(s["h"]), At, Bt, ct, s["Q"], s["Qd"], s["R"], s["x0"], s["xd"])
    assert np.abs(u_new - un).max() > 1e-2
    sol2, _ = cartpole_solver(amd, r["xhi"], r["uhi"], qp_model_free=True)
    sol2.iterate(1)
    assert len(sol2.cost_lst) == 3 and np.isfinite(sol2.cost_lst).all(), sol2.cost_lst


def test_iteration_limit_is_a_failure(amd):
    r = vc.cartpole_bounds()
    sol, _ = cartpole_solver(amd, r["xhi"], r["uhi"], qp_model_free=True, qp_max_iter=3)
    sol.local_descent(sol.x_trj, sol.u_trj)
    info = sol._last["box_info"].cpu().numpy()
    assert sol._box_used and info[1] == 3 and info[2] > 0, info
    sol, _ = cartpole_solver(amd, r["xhi"], r["uhi"], qp_model_free=True, qp_max_iter=3)
    with pytest.raises(ValueError, match="TV_LQR failed"):
        sol.iterate(1)


def test_flags(amd):
    r = vc.cartpole_bounds()
    for flag in ("qp_adaptive_rho", "qp_lazy_bounds"):
        sol, _ = cartpole_solver(amd, r["xhi"], r["uhi"], qp_model_free=True, **{flag: True})
        with pytest.raises(NotImplementedError, match=flag):
            sol.local_descent(sol.x_trj, sol.u_trj)
    sol, _ = cartpole_solver(amd, r["xhi"], r["uhi"])                               # without the flag: as before
    with pytest.raises(NotImplementedError, match="compiled"):
        sol.local_descent(sol.x_trj, sol.u_trj)
    # the position-controlled form has no any-size kernel
    c = vc.case("s3x2-B2")
    with pytest.raises(NotImplementedError, match="no compiled kernel"):
        amd.solve_tvlqr(c["At"], c["Bt"], c["ct"], c["Q"], c["Qd"], c["R"], c["x0"], c["xd"], None,
                        indices_u_into_x=[0, 2], u_bound_abs=np.stack([c["u_lo"], c["u_hi"]]))
    # beyond the horizon limit: the limit is named
    from irs_mpc_amd import device as dev
    n, m = 32, 16
    T = dev.box_values_horizon_limit(n, m) + 1
    rng = np.random.default_rng(0)
    with pytest.raises(NotImplementedError, match="T <= %d" % (T - 1)):
        amd.solve_tvlqr(np.tile(np.eye(n), (T, 1, 1)), rng.normal(size=(T, n, m)), np.zeros((T, n)), np.eye(n), np.eye(n),
                        np.eye(m), np.ones(n), np.zeros((T + 1, n)), None,
                        u_bound_abs=np.stack([-1e-3 * np.ones(m), 1e-3 * np.ones(m)]))


# ------------------------------------------------------------------------------------------------ 5: beside a compiled model
def test_torch_pendulum_beside_the_compiled_pendulum(amd):
    from examples.torch_systems import TorchPendulum
    T, N = 30, 100
    rng = np.random.default_rng(2)
    dx = rng.normal(size=(T, N, 2)).astype(np.float32)
    du = rng.normal(size=(T, N, 1)).astype(np.float32)
    so = orc.PendulumOracle(0.05)

    def params():
        p = amd.IrsLqrParameters()
        p.Q, p.Qd, p.R = np.diag([1., 1.]), np.diag([20., 20.]), np.diag([1.])
        p.x0 = np.array([0., 0.])
        p.xd_trj = np.tile(np.array([np.pi, 0.]), (T + 1, 1))
        p.u_trj_initial = np.tile(np.array([0.1]), (T, 1))
        p.xbound = [-np.array([1e4, 1e4]), np.array([1e4, 1e4])]
        p.ubound = np.array([[-0.05], [0.05]])
        p.qp_rho, p.qp_max_iter, p.qp_eps = vc.QP["rho"], vc.QP["max_iter"], vc.QP["eps"]
        return p

    for name, system, flag in (("torch", TorchPendulum(0.05), True), ("compiled", amd.PendulumDynamics(0.05), False)):
        p = params()
        p.qp_model_free = flag
        sol = amd.IrsLqrZeroOrder(system, p, Replay(dx, du))
        x_new, u_new = sol.local_descent(sol.x_trj, sol.u_trj)
        info = sol._last["box_info"].cpu().numpy() if sol._box_used else None
        assert sol._box_used and info[0] == 0 and info[2] == 0, (name, info)
        At, Bt, ct = (sol._last[k].cpu().numpy() for k in ("At", "Bt", "ct"))
        xo, uo, iters = orc.local_descent_box(so, At, Bt, ct, p.Q, p.Qd, p.R, p.x0, p.xd_trj, *[np.asarray(b, float) for b in p.xbound],
                                              p.ubound[0], p.ubound[1], **vc.QP)
        assert max(iters) < vc.QP["max_iter"], iters
        report("%s: u_new vs oracle" % name, u_new, uo, **DESCENT_TOL)
        report("%s: x_new vs oracle" % name, x_new, xo, **DESCENT_TOL)
        assert np.abs(u_new).max() == pytest.approx(0.05, abs=1e-9)
