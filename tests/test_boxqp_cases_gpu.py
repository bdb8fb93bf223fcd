"""The bounded TV-LQR kernel (csrc/boxqp.hip) on every compiled size, in both forms, under bound rows that differ from
step to step: the cases of oracle/boxqp_cases.py, admitted by tests/test_boxqp_cases_cpu.py.

Each case goes through solve_tvlqr with per-time bound arrays and is held to the suite's own figures for this
kernel: the solver-independent KKT certificate below 1e-5 (on the [x; u_prev] statement for the position-controlled
form) and the oracle's ADMM solution at atol 1e-7.  The cases are built so that a bound row read one step off, a
lo / hi mix-up or a row-0 broadcast moves the solution by more than 1e-4.

Once per form, on a size no test had checked: records in an HBM workspace == records on chip, and a constant bound
given as one row == the same bound tiled, both bit for bit.  And the descent entry with constant bounds
(irs_tvlqr_box_descent, stride-0 rows, T warm-started tails) on the three carts (6, 2), and the quasistatic
solver-1 descent on box pivoting (position-controlled (5, 2)).
"""
import numpy as np
import pytest
import torch

from oracle import boxqp_cases as bc
from oracle import irs_oracle as orc

pytestmark = pytest.mark.gpu


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


def bound_arrays(c, rows=None):
    """solve_tvlqr's bound arguments of a case: (2, rows, width) arrays."""
    r = bc.rows_of(c) if rows is None else rows
    kw = dict(x_bound_abs=np.stack([r["x_lo"], r["x_hi"]]), u_bound_abs=np.stack([r["u_lo"], r["u_hi"]]))
    if c["idx"] is not None:
        kw["u_bound_rel"] = np.stack([r["du_lo"], r["du_hi"]])
    return kw


def device_solve(amd, c, **bounds):
    return amd.solve_tvlqr(c["At"], c["Bt"], c["ct"], c["Q"], c["Qd"], c["R"], c["x0"], c["xd"], None,
                           indices_u_into_x=None if c["idx"] is None else list(c["idx"]), rho=c["rho"], eps=1e-10,
                           max_iter=40000, **bounds)


@pytest.mark.parametrize("cid", list(bc.CASES))
def test_case_kkt_certified_and_equal_to_the_oracle(amd, cid):
    c = bc.case(cid)
    xo, uo, it = bc.reference(cid)
    assert it < 40000
    xs, us = device_solve(amd, c, **bound_arrays(c))
    res = bc.kkt(c, xs, us)
    print("%s KKT residuals (dynamics, box, stationarity, multiplier sign):" % cid, res)
    assert max(res) < 1e-5, res
    report("u* vs oracle ADMM", us, uo, rtol=0, atol=1e-7)
    report("x* vs oracle ADMM", xs, xo, rtol=0, atol=1e-7)


# ------------------------------------------------------------------------------------------------ once per form
FORMS = ["p62-B2", "d52-B2"]


def _ws(nbytes):
    return torch.empty((nbytes,), dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("cid", FORMS)
def test_hbm_records_equal_on_chip(amd, cid):
    """irs_tvlqr_box_solve_wsx with the factor records in a workspace == without one, bit for bit."""
    from irs_mpc_amd import _lib, device as dev
    from irs_mpc_amd.tv_lqr import _model_for
    c = bc.case(cid)
    T, n, m = c["T"], c["At"].shape[1], c["Bt"].shape[2]
    du = c["idx"] is not None
    dm = _model_for(n, m, c["idx"])
    lib = _lib.load()
    d = [dev.to_dev(c[k]) for k in ("At", "Bt", "ct", "Q", "Qd", "R", "xd", "x0")]
    rows = [dev.to_dev(c[k]) for k in bc.ROW_KEYS]
    if not du:
        rows[4] = rows[5] = None
    assert lib.irs_tvlqr_box_workspace_bytes(dm.model_id, T, 1 if du else 0) == 0       # the records fit on chip
    rec = lib.irs_box_records_bytes(dm.model_id, T, _lib.BOX_ADMM_DU if du else _lib.BOX_ADMM)
    assert rec > 0

    def solve(ws):
        xs = torch.zeros((T + 1, n), dtype=dev.F64, device="cuda")
        us = torch.zeros((T, m), dtype=dev.F64, device="cuda")
        info = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        _lib.check(lib.irs_tvlqr_box_solve_wsx(dm.model_id, dm._p, dm._np, T, *[t.data_ptr() for t in d[:6]],
                                               1.0 if du else 0.5, d[6].data_ptr(), d[7].data_ptr(), 1 if du else 0,
                                               *[t.data_ptr() if t is not None else None for t in rows],
                                               c["rho"], 1.6, 40000, 1e-10, xs.data_ptr(), us.data_ptr(),
                                               info.data_ptr(), ws.data_ptr() if ws is not None else None,
                                               ws.numel() if ws is not None else 0, dev._stream()),
                   "irs_tvlqr_box_solve_wsx")
        return xs.cpu().numpy(), us.cpu().numpy(), info.cpu().numpy()

    xa, ua, ia = solve(None)
    xb, ub, ib = solve(_ws((rec + 255) // 256 * 256))
    assert ia[0] == 0 and ia[2] == 0, ia
    np.testing.assert_array_equal(ia, ib)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(ua, ub)
    xo, uo, _ = bc.reference(cid)
    report("u* (records in HBM) vs oracle ADMM", ub, uo, rtol=0, atol=1e-7)


def constant_bounds(c):
    """The B2 bounds of a case made constant in time, one row per argument: on u, per component the tightest finite
    level of its rows; on x, half the unconstrained peak of the component that peaks highest (steps 1 .. T), on
    that side only; and for the position-controlled form a rate limit at 0.7 of the largest unconstrained step."""
    T, n = c["T"], c["At"].shape[1]
    lo, hi = c["u_lo"], c["u_hi"]
    kw = dict(u_bound_abs=np.stack([
        np.where(np.isfinite(lo).any(axis=0), np.where(np.isfinite(lo), lo, -np.inf).max(axis=0), -np.inf),
        np.where(np.isfinite(hi).any(axis=0), np.where(np.isfinite(hi), hi, np.inf).min(axis=0), np.inf)]))
    i = int(np.argmax(np.abs(c["xs"][1:]).max(axis=0)))
    v = c["xs"][1 + int(np.argmax(np.abs(c["xs"][1:, i]))), i]
    xb = np.stack([np.full(n, -np.inf), np.full(n, np.inf)])
    xb[1 if v > 0 else 0, i] = 0.5 * v
    kw["x_bound_abs"] = xb
    if c["idx"] is not None:
        d = np.diff(np.vstack([c["x0"][list(c["idx"])][None], c["us"]]), axis=0)
        kw["u_bound_rel"] = np.stack([-0.7 * np.abs(d).max(axis=0), 0.7 * np.abs(d).max(axis=0)])
    return kw


def tiled(c, kw):
    """The same bounds as per-time rows."""
    rows = {"x_bound_abs": c["T"] + 1, "u_bound_abs": c["T"], "u_bound_rel": c["T"]}
    return {k: np.stack([np.tile(b[0], (rows[k], 1)), np.tile(b[1], (rows[k], 1))]) for k, b in kw.items()}


@pytest.mark.parametrize("cid", FORMS)
def test_one_row_equals_the_same_row_tiled(amd, cid):
    """Constant bounds given as one row, (2, n) / (2, m), for every bound argument of the form == the same bounds as
    (2, rows, width) arrays, bit for bit; the state, the input and (position-controlled) the rate bound all bind."""
    c = bc.case(cid)
    kw = constant_bounds(c)
    x1, u1 = device_solve(amd, c, **kw)
    x2, u2 = device_solve(amd, c, **tiled(c, kw))
    np.testing.assert_array_equal(x1, x2)
    np.testing.assert_array_equal(u1, u2)
    vals = {"x_bound_abs": x1[1:], "u_bound_abs": u1}
    if c["idx"] is not None:
        vals["u_bound_rel"] = np.diff(np.vstack([c["x0"][list(c["idx"])][None], u1]), axis=0)
    for k, b in kw.items():
        assert (vals[k] >= b[0] - 1e-7).all() and (vals[k] <= b[1] + 1e-7).all(), k
        assert (np.abs(vals[k] - b[0]) < 1e-7).any() or (np.abs(vals[k] - b[1]) < 1e-7).any(), (k, "does not bind")


# ------------------------------------------------------------------------------------------------ the descent entry
def test_three_cart_box_descent_vs_oracle(amd):
    """irs_tvlqr_box_descent (T warm-started tail QPs, constant bounds as stride-0 rows) through
    IrsLqrExact.local_descent on the three carts (6, 2): an input bound at 0.6 and a bound on the third cart's
    velocity at 0.7 of what the unbounded descent reaches, both binding, against the oracle's restatement at the
    tolerances of test_box_descent_vs_oracle."""
    T = 10
    so = orc.ThreeCartOracle(0.05)
    p = amd.IrsLqrParameters()
    p.Q, p.Qd, p.R = 0.01 * np.diag([50., 50, 50, 20, 100, 20]), np.diag([50., 50, 50, 20, 100, 20]), 0.01 * np.eye(2)
    p.x0 = np.array([0., 1, 2, 0, 0, 0])
    p.xd_trj = np.tile(np.array([2., 3, 4, 0, 0, 0]), (T + 1, 1))
    p.u_trj_initial = np.tile(np.array([0.1, -0.1]), (T, 1))
    x_trj = orc.rollout(so, p.x0, p.u_trj_initial)
    At, Bt, ct = orc.exact_TV(so, x_trj, p.u_trj_initial)
    xn, un, _, _ = orc.local_descent(so, At, Bt, ct, p.Q, p.Qd, p.R, p.x0, p.xd_trj)
    ubnd, vbnd = 0.6 * np.abs(un[:, 0]).max(), 0.7 * np.abs(xn[:, 5]).max()
    xhi, uhi = np.full(6, np.inf), np.array([ubnd, np.inf])
    xhi[5] = vbnd
    p.xbound, p.ubound = [-xhi, xhi], np.array([-uhi, uhi])
    p.qp_rho, p.qp_max_iter, p.qp_eps = 1.0, 20000, 1e-10
    sol = amd.IrsLqrExact(amd.ThreeCartDynamics(0.05), p)
    x_new, u_new = sol.local_descent(sol.x_trj, sol.u_trj)
    info = sol._last["box_info"].cpu().numpy() if sol._box_used else None
    assert sol._box_used and info[0] == 0 and info[2] == 0, info
    xo, uo, iters = orc.local_descent_box(so, At, Bt, ct, p.Q, p.Qd, p.R, p.x0, p.xd_trj, -xhi, xhi, -uhi, uhi,
                                          rho=1.0, max_iter=20000, eps=1e-10)
    assert max(iters) < 20000, iters
    report("u_new vs oracle", u_new, uo, rtol=1e-5, atol=1e-6)
    report("x_new vs oracle", x_new, xo, rtol=1e-5, atol=1e-6)
    assert np.abs(u_new[:, 0]).max() == pytest.approx(ubnd, abs=1e-9)              # the input bound is active
    assert np.abs(x_new[:, 5]).max() > vbnd - 1e-3                                 # and the state bound
    assert np.abs(u_new - un).max() > 1e-2


def test_box_pivoting_admm_descent_vs_oracle(amd):
    """The quasistatic descent with solver 1 (the ADMM kernel's position-controlled (5, 2) form, T warm-started tails,
    contact dynamics in the loop) on box pivoting at T = 8 with abs + rel rows, against the oracle's restatement at
    the tolerances of test_quasistatic_box_descent_vs_oracle.  The nominal hand push moves 0.0125 per step, inside the
    rate limit of 0.03, and the hand follows its command to 1.3e-2: every tail QP is feasible from the realised
    state.  Both the trust region and the rate limit bind."""
    from irs_mpc_amd import device as dev
    T = 8
    sys_d, sys_o = amd.BoxPivotingDynamics(0.1), orc.BoxPivotOracle(0.1)
    pack, idx = orc.BoxPivotOracle.pack, sys_o.indices_u_into_x
    x0 = sys_o.dynamics(pack([0.0, 0.5, 0.0], [-0.5, 0.5]), np.array([-0.5, 0.5]))      # resolve the initial overlap
    u_trj = np.stack([np.array([-0.5 + 0.1 * (t + 1) / T, 0.5]) for t in range(T)])
    x_trj = orc.rollout(sys_o, x0, u_trj)
    du = 0.1 * np.random.default_rng(8).normal(size=(T, 400, 2))
    At, Bt, ct = orc.zero_order_B_decoupled(sys_o, x_trj, u_trj, du)
    Q = np.diag(pack([5, 5, 50], [0, 0]))
    Qd, R = Q.copy(), 10.0 * np.eye(2)
    xd = np.tile(pack([1.0, 1.0, -np.pi / 2], [-0.5, 0.5]), (T + 1, 1))
    rows = orc.quasistatic_bounds(x_trj, idx, None, np.array([-np.ones(2) * 0.03, np.ones(2) * 0.03]),
                                  np.array([-np.ones(2) * 0.03, np.ones(2) * 0.03]))
    xo, uo, iters = orc.local_descent_quasistatic(sys_o, At, Bt, ct, Q, Qd, R, x0, xd, *rows, rho=1.0, max_iter=40000,
                                                  eps=1e-10, relax=1.6)
    assert max(iters) < 40000, iters
    rows_d = [dev.to_dev(r) if np.isfinite(r).any() else None for r in rows]
    o = sys_d.dm().quasistatic_box_descent(*[dev.to_dev(a) for a in (At, Bt, ct, Q, Qd, R, xd, x0)], *rows_d,
                                           solver=1, rho=1.0, relax=1.6, max_iter=40000, eps=1e-10)
    info = o["info"].cpu().numpy()
    assert info[0] == 0 and info[2] == 0, info
    un, xn = o["u_new"].cpu().numpy(), o["x_new"].cpu().numpy()
    report("u_new vs oracle", un, uo, rtol=0, atol=2e-7)
    report("x_new vs oracle", xn, xo, rtol=0, atol=2e-7)
    report("cost", float(o["cost"].item()), orc.eval_cost_quasistatic(xo, uo, xd, Q, Qd, R, idx), rtol=1e-7)
    assert np.isclose(np.abs(un - x_trj[:-1, idx]).max(), 0.03, atol=1e-7)           # the trust region binds,
    assert np.isclose(np.abs(un - xn[:-1, idx]).max(), 0.03, atol=1e-7)              # and the rate limit (from x_t[idx])
