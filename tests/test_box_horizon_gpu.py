"""The bounded TV-LQR beyond the LDS horizon (csrc/boxqp.hip, factor records in a workspace in HBM): the same
result as the on-chip path, bit for bit, and the public entry points at horizons that used to raise
NotImplementedError (quadrotor T = 100 / 200, planar hand solver 1 at T = 80)."""
import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return irs_mpc_amd


def bike_params(amd, T):
    p = amd.IrsLqrParameters()
    p.Q, p.Qd, p.R = np.diag([5, 5, 3, 0.1, 0.1]), np.diag([50., 50, 30, 1, 1]), np.diag([1, 0.1])
    p.x0 = np.zeros(5)
    p.xd_trj = np.tile(np.array([3.0, 1.0, np.pi / 2, 0, 0]), (T + 1, 1))
    p.u_trj_initial = np.tile(np.array([0.1, 0.0]), (T, 1))
    return p


HAND = orc.PlanarHandOracle
HAND_IDX = np.array([1, 4, 2, 5])
HAND_Q = HAND.pack([1e-3, 1e-3, 10.0], [1e-3, 1e-3], [1e-3, 1e-3])
HAND_GOAL = HAND.pack([0.3, -0.1, 0.5], [0, 0], [0, 0])


def hand_problem(amd, T, N, seed, oracle_tv=True):
    """The planar hand's descent problem: nominal trajectory, TV matrices (oracle or device sample pass on the same
    draws), weights and goal."""
    from irs_mpc_amd import device as dev
    from irs_mpc_amd._lib import SMOOTH_ZERO_ORDER_B
    sys_d, sys_o = amd.PlanarHandDynamics(0.1), orc.PlanarHandOracle(0.1)
    x0 = HAND.pack([0.0, 0.35, 0.0], [-np.pi / 4, -np.pi / 4], [np.pi / 4, np.pi / 4])
    for _ in range(4):
        x0 = sys_o.dynamics(x0, np.array([-np.pi / 4, -np.pi / 4, np.pi / 4, np.pi / 4]))
    u_trj = np.tile(x0[HAND_IDX], (T, 1))
    x_trj = orc.rollout(sys_o, x0, u_trj)
    du = (np.random.default_rng(seed).normal(size=(T, N, 4)) * 0.1).astype(np.float32)
    if oracle_tv:
        At, Bt, ct = orc.zero_order_B_decoupled(sys_o, x_trj, u_trj, du.astype(np.float64))
    else:
        o = sys_d.dm().smooth(SMOOTH_ZERO_ORDER_B, dev.to_dev(x_trj), dev.to_dev(u_trj), None, dev.to_dev(du, dev.F32))
        At, Bt, ct = (o[k].cpu().numpy() for k in ("At", "Bt", "ct"))
    Q, Qd, R = np.diag(HAND_Q), np.diag(100 * HAND_Q), 5.0 * np.eye(4)
    xd = np.tile(x0 + HAND_GOAL, (T + 1, 1))
    return sys_d, sys_o, x0, u_trj, x_trj, (At, Bt, ct), (Q, Qd, R, xd)


def quad_problem(amd, T, att=None, rate=None):
    """examples/quadrotor (quadrotor_first_order.py:12-44) with roll and pitch limited to +-att, or the body rates
    about those axes to +-rate."""
    from examples.problems import quadrotor
    sysd, p, _, _, _ = quadrotor(T)
    big = np.array([1e5, 1e5, 1e5, 2.0 * np.pi, np.pi / 2, 2.0 * np.pi, 1e5, 1e5, 1e5, 1e5, 1e5, 1e5])
    if att is not None:
        big[3] = big[4] = att
    if rate is not None:
        big[9] = big[10] = rate
    p.xbound = [-big, big]
    p.qp_rho, p.qp_max_iter = 1.0, 20000
    return sysd, p


def _ws(nbytes):
    return torch.empty((nbytes,), dtype=torch.uint8, device="cuda")


# ---------------------------------------------------------------- 1. the same result both ways
def test_box_descent_hbm_records_equal_on_chip(amd):
    """irs_tvlqr_box_descent_wsx with a workspace (records in HBM, forced at a horizon that fits on chip) == the
    on-chip call, bit for bit: the same operations in the same order, only the records' home differs."""
    from irs_mpc_amd import device as dev
    T, steer, ubnd = 30, 0.3, 2.0
    p = bike_params(amd, T)
    p.xbound = [-np.array([1e4, 1e4, 1e4, 1e4, steer]), np.array([1e4, 1e4, 1e4, 1e4, steer])]
    p.ubound = np.array([[-ubnd, -1e4], [ubnd, 1e4]])
    sol = amd.IrsLqrExact(amd.BicycleDynamics(0.1), p)
    dm = sol._dm
    assert dm.lib.irs_tvlqr_box_workspace_bytes(dm.model_id, T, 0) == 0          # the records fit on chip
    x, u = dev.to_dev(sol.x_trj), dev.to_dev(sol.u_trj)
    At, Bt, ct = sol._get_TV_matrices_dev(x, u)
    args = (At, Bt, ct, sol._Q, sol._Qd, sol._R, sol._xd, x[0].contiguous(), *sol._box_bounds())
    a = dm.tvlqr_box_descent(*args, alpha_R=0.5, eps=1e-10, max_iter=20000)
    b = dm.tvlqr_box_descent(*args, alpha_R=0.5, eps=1e-10, max_iter=20000, records_in_hbm=True)
    ia, ib = a["info"].cpu().numpy(), b["info"].cpu().numpy()
    assert ia[0] == 0 and ia[2] == 0, ia
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(a["x_new"].cpu().numpy(), b["x_new"].cpu().numpy())
    np.testing.assert_array_equal(a["u_new"].cpu().numpy(), b["u_new"].cpu().numpy())
    xn, un = a["x_new"].cpu().numpy(), a["u_new"].cpu().numpy()
    assert np.abs(xn[:, 4]).max() > steer - 1e-3                                 # state bound active
    assert np.abs(un[:, 0]).max() == pytest.approx(ubnd, abs=1e-9)                # input bound active


def test_box_solve_hbm_records_equal_on_chip(amd):
    """irs_tvlqr_box_solve_wsx, position-controlled form (planar hand, T = 10: trust region + rate limit) with the
    records in a workspace == without one, bit for bit."""
    from irs_mpc_amd import _lib, device as dev
    T = 10
    sys_d, sys_o, x0, u_trj, x_trj, (A, B, c), (Q, Qd, R, xd) = hand_problem(amd, T, 300, 77)
    idx = sys_o.indices_u_into_x
    rows = orc.quasistatic_bounds(x_trj, idx, None, np.array([-np.ones(4) * 0.05, np.ones(4) * 0.05]),
                                  np.array([-np.ones(4) * 0.03, np.ones(4) * 0.03]))
    dm = sys_d.dm()
    lib = _lib.load()
    d = [dev.to_dev(a) for a in (A, B, c, Q, Qd, R, xd, x0, rows[2], rows[3], rows[4], rows[5])]
    rec = lib.irs_tvlqr_box_workspace_bytes(dm.model_id, 2000, 1) // 2000 * T        # T records of this form
    assert lib.irs_tvlqr_box_workspace_bytes(dm.model_id, T, 1) == 0

    def solve(ws):
        xs, us = torch.zeros((T + 1, 7), dtype=dev.F64, device="cuda"), torch.zeros((T, 4), dtype=dev.F64, device="cuda")
        info = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        _lib.check(lib.irs_tvlqr_box_solve_wsx(dm.model_id, dm._p, dm._np, T, *[t.data_ptr() for t in d[:6]], 1.0,
                                               d[6].data_ptr(), d[7].data_ptr(), 1, None, None,
                                               *[t.data_ptr() for t in d[8:]], 100.0, 1.6, 40000, 1e-10,
                                               xs.data_ptr(), us.data_ptr(), info.data_ptr(),
                                               ws.data_ptr() if ws is not None else None,
                                               ws.numel() if ws is not None else 0, dev._stream()),
                   "irs_tvlqr_box_solve_wsx")
        return xs.cpu().numpy(), us.cpu().numpy(), info.cpu().numpy()

    xa, ua, ia = solve(None)
    xb, ub, ib = solve(_ws((rec + 255) // 256 * 256))
    assert ia[0] == 0 and ia[2] == 0, ia
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(ua, ub)
    assert np.abs(np.diff(np.vstack([x0[idx][None], ua]), axis=0)).max() == pytest.approx(0.03, abs=1e-7)
    # a workspace one byte short is refused
    with pytest.raises(_lib.IrsHipError):
        solve(_ws(rec - 1))


# ---------------------------------------------------------------- 2. the quadrotor past the old cap (T <= 50)
# Body-rate limits (x[9], x[10]) keep every tail QP of the descent feasible from any realised state: the controls
# drive the rates directly.  Roll and pitch are one integration further from the controls, and through the
# nonlinear attitude kinematics the realised state can leave a tail QP no feasible first step (the linear model's
# x_{t+1} angle is fixed by x_t); those limits are exercised on single QPs from x0 (solve_tvlqr, KKT certified).
RATE_LIM = 7.0            # the unbounded first descent turns at up to ~11-12 rad/s
ATT_LIM = 0.5             # ... and leans to 0.68 (roll), 0.83 (pitch)


def _kkt(amd, At, Bt, ct, p, xs, us):
    big = p.xbound[1]
    return orc.qp_box_kkt_residuals(At, Bt, ct, p.Q, p.Qd, p.R, p.x0, p.xd_trj, -big, big, np.full(4, -1e5),
                                    np.full(4, 1e5), xs, us, alpha_R=0.5)


def test_quadrotor_bounded_descent_beyond_the_lds_horizon(amd):
    """IrsLqrExact on the quadrotor at T = 100 (the LDS holds T <= 50) with body-rate limits that bind: the bounded
    descent runs with its records in HBM, every tail converges, the realised rates keep the limits and reach them.
    The first tail solved alone by solve_tvlqr passes the QP's KKT certificate."""
    T = 100
    sysd, p = quad_problem(amd, T, rate=RATE_LIM)
    sol = amd.IrsLqrExact(sysd, p)
    sol.verbose = False
    x_new, u_new = sol.local_descent(sol.x_trj, sol.u_trj)
    assert sol._box_used
    info = sol._last["box_info"].cpu().numpy()
    assert info[0] == 0 and info[2] == 0, info
    rates = np.abs(x_new[1:, 9:11]).max()
    assert RATE_LIM - 1e-3 < rates <= RATE_LIM + 1e-6, rates
    so = orc.QuadrotorOracle(0.05)
    At, Bt, ct = orc.exact_TV(so, sol.x_trj, sol.u_trj)
    big = p.xbound[1]
    xs, us = amd.solve_tvlqr(At, Bt, ct, p.Q, p.Qd, p.R, p.x0, p.xd_trj, None, x_bound_abs=np.stack([-big, big]),
                             rho=1.0, eps=1e-9, max_iter=40000)
    assert RATE_LIM - 1e-6 < np.abs(xs[1:, 9:11]).max() <= RATE_LIM + 1e-6
    res = _kkt(amd, At, Bt, ct, p, xs, us)
    assert max(res) < 1e-5, res


@pytest.mark.parametrize("T", [100, 200])
def test_quadrotor_solve_tvlqr_attitude_limits(amd, T):
    """solve_tvlqr with binding roll / pitch limits at T = 100 and at the reference script's horizon
    (quadrotor_first_order.py: T = 200): KKT certified."""
    sysd, p = quad_problem(amd, T, att=ATT_LIM)
    so = orc.QuadrotorOracle(0.05)
    x = orc.rollout(so, p.x0, p.u_trj_initial)
    At, Bt, ct = orc.exact_TV(so, x, p.u_trj_initial)
    big = p.xbound[1]
    xs, us = amd.solve_tvlqr(At, Bt, ct, p.Q, p.Qd, p.R, p.x0, p.xd_trj, None, x_bound_abs=np.stack([-big, big]),
                             rho=1.0, eps=1e-9, max_iter=40000)
    assert ATT_LIM - 1e-6 < np.abs(xs[1:, 3:5]).max() <= ATT_LIM + 1e-6
    res = _kkt(amd, At, Bt, ct, p, xs, us)
    assert max(res) < 1e-5, res


# ---------------------------------------------------------------- 3. the fused loop == the host loop past the cap
def test_fused_iterate_equals_the_host_loop_beyond_the_lds_horizon(amd, capsys):
    """IrsLqrExact.iterate through irs_iterate (the bounded descent behind the device-side flag, its records in the
    tail of the scratch) == the host loop, quadrotor T = 100 with binding body-rate limits, 3 iterations."""
    T, iters = 100, 3

    def make(verbose):
        sysd, p = quad_problem(amd, T, rate=RATE_LIM)
        sol = amd.IrsLqrExact(sysd, p)
        sol.verbose = verbose
        return sol

    a, b = make(False), make(True)
    ra = a.iterate(iters)
    rb = b.iterate(iters)
    capsys.readouterr()
    assert getattr(b, "_box_used", False)
    assert len(a.cost_lst) == len(b.cost_lst) == iters + 2 and a.iter == b.iter
    # (the fused path takes the cost the bounded kernel accumulates, the host loop a separate launch: the same sum
    # in another order)
    np.testing.assert_allclose(np.array(a.cost_lst), np.array(b.cost_lst), rtol=1e-13, atol=0)
    for xa, xb in zip(a.x_trj_lst, b.x_trj_lst):
        np.testing.assert_array_equal(xa, xb)
    for ua, ub in zip(a.u_trj_lst, b.u_trj_lst):
        np.testing.assert_array_equal(ua, ub)
    np.testing.assert_array_equal(ra[0], rb[0])


# ---------------------------------------------------------------- 4. quasistatic solver 1 past the old cap (T <= 56)
def test_quasistatic_admm_beyond_the_lds_horizon(amd):
    """DeviceModel.quasistatic_box_descent, solver 1 (ADMM on the [x; u_prev] augmentation) on the planar hand at
    T = 80: with one abs box it equals the exact active-set solver (3); with abs + rel + x bounds every bound holds
    and the abs box binds.  (At this horizon the ADMM converges to 1e-8 with rho = 30 within 14 000 iterations; with
    rho = 100, the value the T = 8 parity test uses, some tails need more than 20 000.)"""
    from irs_mpc_amd import device as dev
    T = 80
    sys_d, sys_o, x0, u_trj, x_trj, (At, Bt, ct), (Q, Qd, R, xd) = hand_problem(amd, T, 200, 21, oracle_tv=False)
    idx = sys_o.indices_u_into_x
    dm = sys_d.dm()
    assert dm.lib.irs_quasistatic_box_lds_bytes(dm.model_id, T, 1) > dm.BOX_LDS_LIMIT
    assert dm.quasistatic_descent_supported(T, 1)
    prob = [dev.to_dev(a) for a in (At, Bt, ct, Q, Qd, R, xd, x0)]
    ub = np.array([-np.ones(4) * 0.05, np.ones(4) * 0.05])
    rows = orc.quasistatic_bounds(x_trj, idx, None, ub, None)
    rows_d = [dev.to_dev(r) if np.isfinite(r).any() else None for r in rows]
    o1 = dm.quasistatic_box_descent(*prob, *rows_d, solver=1, rho=30.0, relax=1.6, max_iter=20000, eps=1e-8)
    o3 = dm.quasistatic_box_descent(*prob, *rows_d, solver=3, max_iter=2000, eps=1e-10)
    i1, i3 = o1["info"].cpu().numpy(), o3["info"].cpu().numpy()
    assert i1[0] == 0 and i1[2] == 0, i1
    assert i3[0] == 0 and i3[2] == 0, i3
    np.testing.assert_allclose(o1["u_new"].cpu().numpy(), o3["u_new"].cpu().numpy(), rtol=0, atol=2e-7)
    np.testing.assert_allclose(o1["x_new"].cpu().numpy(), o3["x_new"].cpu().numpy(), rtol=0, atol=2e-7)
    # abs + rel + x: only the ADMM solver takes these
    rb = np.array([-np.ones(4) * 0.03, np.ones(4) * 0.03])
    xb = np.array([-np.ones(7) * 0.04, np.ones(7) * 0.04])
    rows = orc.quasistatic_bounds(x_trj, idx, xb, ub, rb)
    rows_d = [dev.to_dev(r) if np.isfinite(r).any() else None for r in rows]
    o = dm.quasistatic_box_descent(*prob, *rows_d, solver=1, rho=30.0, relax=1.6, max_iter=20000, eps=1e-8)
    info = o["info"].cpu().numpy()
    assert info[0] == 0 and info[2] == 0, info
    un, xn = o["u_new"].cpu().numpy(), o["x_new"].cpu().numpy()
    assert np.all(un >= rows[2] - 1e-7) and np.all(un <= rows[3] + 1e-7)               # abs box
    assert np.isclose(np.abs(un - x_trj[:-1, idx]).max(), 0.05, atol=1e-7)             # ... binds
    du = np.diff(np.vstack([x0[idx][None], un]), axis=0)
    assert np.all(du >= rows[4] - 1e-7) and np.all(du <= rows[5] + 1e-7)               # rate limit
    assert np.all(np.isfinite(xn))


def test_irs_lqr_quasistatic_admm_constructs_and_iterates_beyond_the_lds_horizon(amd):
    """IrsLqrQuasistatic(..., qp_solver=1) at T = 80 (it raised NotImplementedError at T > 56) and one iteration:
    examples/planar_hand (run_planar_hand.py) with its trust region, seeded host draws."""
    from examples.run_quasistatic import problem
    T = 80
    q_dynamics, x0, u0, Q_dict, Qd_dict, R_dict, xd = problem(T, 0.1)
    p = amd.IrsLqrQuasistaticParameters()
    p.Q_dict, p.Qd_dict, p.R_dict = Q_dict, Qd_dict, R_dict
    p.x0, p.x_trj_d, p.u_trj_0, p.T = x0, xd, u0, T
    p.u_bounds_abs = np.array([-np.ones(4) * 0.05, np.ones(4) * 0.05])
    p.sampling = lambda u_initial, it: u_initial / (it ** 0.5)
    p.std_u_initial, p.num_samples, p.publish_every_iteration = np.ones(4) * 0.1, 200, False
    p.qp_solver, p.qp_rho, p.qp_max_iter, p.qp_eps = 1, 30.0, 20000, 1e-8
    np.random.seed(3)
    sol = amd.IrsLqrQuasistatic(q_dynamics, p)
    c0 = sol.cost
    sol.iterate(0)
    assert len(sol.cost_all_list) == 2 and np.all(np.isfinite(sol.cost_all_list))
    assert sol.cost_all_list[0] == c0
