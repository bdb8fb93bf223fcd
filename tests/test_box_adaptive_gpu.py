"""The adaptive ADMM penalty of the bounded TV-LQR kernel (csrc/boxqp.hip, box_descent_kernel<.., ADAPT = true>) on the
GPU: against its NumPy twin (tests/helpers/admm_adaptive_twin.py) and the QP's KKT certificate from three starting
penalties, records on chip == records in HBM bit for bit, the position-controlled form, and IrsLqrExact on the hard
bicycle problem against the reference's result file (tests/golden/bicycle_hard_exact.csv)."""
import os

import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc
from tests.helpers.admm_adaptive_twin import AdaptiveBoxAdmm, local_descent_box_adaptive

pytestmark = pytest.mark.gpu

RHO0 = [0.1, 10.0, 1000.0]
RELAX = 1.6             # DeviceModel's default; the twin runs at the same value


@pytest.fixture(scope="module")
def amd():
    import irs_mpc_amd
    from irs_mpc_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    _lib.load()
    return irs_mpc_amd


def report(what, got, want, atol):
    """Print the figure, then assert it."""
    err = np.abs(np.asarray(got, float) - np.asarray(want, float)).max()
    print("%s: max abs err %.3g (bound %.3g)" % (what, err, atol))
    assert err < atol, (what, err, atol)


# ------------------------------------------------------------------------------------ (a), (b): the T = 25 bicycle
@pytest.fixture(scope="module")
def bike25(amd):
    """The problem of test_box_qp_solution_satisfies_kkt (T = 25, steer bound 0.3 and input bound 2.0, both active), on
    the device and on the host, with the twin's descent and single solve from each starting rho (computed once)."""
    from irs_mpc_amd import device as dev
    T = 25
    s = orc.BicycleOracle(0.1)
    Q, Qd, R = np.diag([5, 5, 3, 0.1, 0.1]), np.diag([50., 50, 30, 1, 1]), np.diag([1, 0.1])
    x0, xd = np.zeros(5), np.tile(np.array([3.0, 1.0, np.pi / 2, 0, 0]), (T + 1, 1))
    u0 = np.tile(np.array([0.1, 0.0]), (T, 1))
    xlo, ulo = np.array([-np.inf] * 4 + [-0.3]), np.array([-2.0, -np.inf])
    box = (xlo, -xlo, ulo, -ulo)
    At, Bt, ct = orc.exact_TV(s, orc.rollout(s, x0, u0), u0)
    twin = {}
    for rho0 in RHO0:
        xn, un, iters, failed, adm = local_descent_box_adaptive(s, At, Bt, ct, Q, Qd, R, x0, xd, *box, rho=rho0,
                                                                max_iter=5000, eps=1e-8, relax=RELAX)
        assert not failed
        one = AdaptiveBoxAdmm(At, Bt, ct, Q, Qd, R, *box, rho0)
        zx, zu, _, it, conv = one.solve(xd, x0, 0, None, 5000, 1e-8, RELAX)
        assert conv and adm.factorisations >= one.factorisations
        twin[rho0] = dict(x_new=xn, u_new=un, factorisations=adm.factorisations, rho=adm.rho, x_star=zx.copy(),
                          u_star=zu.copy(), solve_factorisations=one.factorisations)
    host = dict(At=At, Bt=Bt, ct=ct, Q=Q, Qd=Qd, R=R, xd=xd, x0=x0, box=box)
    d = [dev.to_dev(a) for a in (At, Bt, ct, Q, Qd, R, xd, x0)]
    return dict(T=T, host=host, dev=d, box_dev=[dev.to_dev(b) for b in box],
                rows_dev=[dev.to_dev(np.tile(b, (rows, 1))) for b, rows in zip(box, (T + 1, T + 1, T, T))],
                twin=twin, dm=amd.BicycleDynamics(0.1).dm())


def test_adaptive_descent_matches_the_twin(bike25):
    """(a), as a descent: T warm-started tails, the penalty carried from tail to tail."""
    b = bike25
    counts = []
    for rho0 in RHO0:
        o = b["dm"].tvlqr_box_descent(*b["dev"], *b["box_dev"], alpha_R=0.5, rho=rho0, max_iter=5000, eps=1e-8,
                                      adaptive_rho=True)
        info, adapt = o["info"].cpu().numpy(), o["adapt"].cpu().numpy()
        tw = b["twin"][rho0]
        print("rho0 %g: info %s, %d factorisations (twin %d), final rho %.4g (twin %.4g)"
              % (rho0, info, adapt[0], tw["factorisations"], adapt[1], tw["rho"]))
        assert info[0] == 0 and info[2] == 0, info
        report("u_new vs twin, rho0 %g" % rho0, o["u_new"].cpu().numpy(), tw["u_new"], 1e-6)
        report("x_new vs twin, rho0 %g" % rho0, o["x_new"].cpu().numpy(), tw["x_new"], 1e-6)
        assert adapt[0] >= 1 and adapt[0] == int(adapt[0]) and adapt[1] > 0
        counts.append(adapt[0])
    assert max(counts) > 1, counts


def test_adaptive_single_tail_is_kkt_certified_and_matches_the_twin(bike25):
    """(a), as single_tail (irs_tvlqr_box_solve_set): the oracle's KKT certificate on the plan."""
    b, h = bike25, bike25["host"]
    for rho0 in RHO0:
        o = b["dm"].tvlqr_box_solve(*b["dev"], *b["rows_dev"], alpha_R=0.5, rho=rho0, max_iter=5000, eps=1e-8,
                                    adaptive_rho=True)
        info, adapt = o["info"].cpu().numpy(), o["adapt"].cpu().numpy()
        xs, us = o["x_star"].cpu().numpy(), o["u_star"].cpu().numpy()
        assert info[0] == 0 and info[2] == 0, info
        res = orc.qp_box_kkt_residuals(h["At"], h["Bt"], h["ct"], h["Q"], h["Qd"], h["R"], h["x0"], h["xd"], *h["box"],
                                       xs, us)
        print("rho0 %g: info %s, %d factorisations, final rho %.4g; KKT (dyn, box, stat, sign) %s"
              % (rho0, info, adapt[0], adapt[1], res))
        r_dyn, r_box, r_stat, sign_bad = res
        assert r_dyn < 1e-10 and r_box < 1e-8 and r_stat < 1e-6 and sign_bad < 1e-7, res
        assert (np.abs(xs[:, 4]) > 0.3 - 1e-6).sum() > 5 and (np.abs(us[:, 0]) > 2 - 1e-6).sum() > 2   # both active
        report("u* vs twin, rho0 %g" % rho0, us, b["twin"][rho0]["u_star"], 1e-6)
        assert adapt[0] == b["twin"][rho0]["solve_factorisations"]


def test_adaptive_records_in_hbm_equal_on_chip(bike25):
    """(b): with the records forced into the HBM workspace -- where a new rho rewrites them and the staging ring must
    not keep a stale one -- the same bits as on chip, descent and single solve, from a rho that makes the rule move."""
    b = bike25
    for rho0 in (0.1, 1000.0):
        kw = dict(alpha_R=0.5, rho=rho0, max_iter=5000, eps=1e-8, adaptive_rho=True)
        on = b["dm"].tvlqr_box_descent(*b["dev"], *b["box_dev"], **kw)
        hbm = b["dm"].tvlqr_box_descent(*b["dev"], *b["box_dev"], records_in_hbm=True, **kw)
        assert on["adapt"][0].item() > 1
        for k in ("x_new", "u_new", "info", "adapt"):
            assert torch.equal(on[k], hbm[k]), (rho0, k)
        on = b["dm"].tvlqr_box_solve(*b["dev"], *b["rows_dev"], **kw)
        hbm = b["dm"].tvlqr_box_solve(*b["dev"], *b["rows_dev"], records_in_hbm=True, **kw)
        for k in ("x_star", "u_star", "info", "adapt"):
            assert torch.equal(on[k], hbm[k]), (rho0, k)


def test_adaptive_descent_beyond_the_lds_horizon(amd):
    """(b), one horizon the LDS does not hold: the quadrotor at T = 100 (on chip: T <= 50) with body-rate limits that
    bind (the problem of test_quadrotor_bounded_descent_beyond_the_lds_horizon), adaptive from that test's rho = 1.  The
    descent converges on every tail and keeps and reaches the limits; the first tail alone passes the KKT certificate
    at that test's threshold."""
    from examples.problems import quadrotor
    from irs_mpc_amd import device as dev
    T, rate = 100, 7.0
    sysd, p, _, _, _ = quadrotor(T)
    big = np.array([1e5, 1e5, 1e5, 2.0 * np.pi, np.pi / 2, 2.0 * np.pi, 1e5, 1e5, 1e5, rate, rate, 1e5])
    p.xbound = [-big, big]
    p.qp_rho, p.qp_max_iter, p.qp_adaptive_rho = 1.0, 20000, True          # that test's penalty and limit
    sol = amd.IrsLqrExact(sysd, p)
    sol.verbose = False
    dm = sol._dm
    assert dm.lib.irs_tvlqr_box_workspace_bytes(dm.model_id, T, 0) > 0            # the records do not fit on chip
    x_new, u_new = sol.local_descent(sol.x_trj, sol.u_trj)
    assert sol._box_used
    info, adapt = sol._last["box_info"].cpu().numpy(), sol._last["box_adapt"].cpu().numpy()
    print("descent: info %s, %d factorisations, final rho %.4g" % (info, adapt[0], adapt[1]))
    assert info[0] == 0 and info[2] == 0, info
    rates = np.abs(x_new[1:, 9:11]).max()
    assert rate - 1e-3 < rates <= rate + 1e-6, rates
    so = orc.QuadrotorOracle(0.05)
    At, Bt, ct = orc.exact_TV(so, sol.x_trj, sol.u_trj)
    xs, us = amd.solve_tvlqr(At, Bt, ct, p.Q, p.Qd, p.R, p.x0, p.xd_trj, None, x_bound_abs=np.stack([-big, big]),
                             rho=1.0, eps=1e-9, max_iter=40000, adaptive_rho=True)
    assert rate - 1e-6 < np.abs(xs[1:, 9:11]).max() <= rate + 1e-6
    res = orc.qp_box_kkt_residuals(At, Bt, ct, p.Q, p.Qd, p.R, p.x0, p.xd_trj, -big, big, np.full(4, -1e5),
                                   np.full(4, 1e5), xs, us, alpha_R=0.5)
    print("first tail alone: KKT (dyn, box, stat, sign) %s" % (res,))
    assert max(res) < 1e-5, res


# ------------------------------------------------------------------------------------ (c): the position-controlled form
def test_adaptive_position_controlled_descent_matches_the_fixed_penalty(amd, golden_dir):
    """(c): box pushing at T = 10 from step 40 of the recorded push (sticking contact), a state trust region (0.04 on
    the hand) and a rate box (0.03): both bind.  Solver 1 adaptive from rho = 1 -- where the fixed penalty needs more
    than 5000 iterations on most tails -- and from 100 == solver 1 at the fixed rho = 100 the suite uses for this
    solver (test_irs_lqr_quasistatic_host_twin), converged to 1e-10."""
    from irs_mpc_amd import device as dev
    T, t0 = 10, 40
    sys_d, sys_o = amd.BoxPushingDynamics(0.1), orc.BoxPushOracle(0.1)
    pack, idx = orc.BoxPushOracle.pack, sys_o.indices_u_into_x
    xu = np.load(os.path.join(golden_dir, "box_pushing_xu_quasistatic.npy"))
    x0, u_trj = xu[t0, :5], xu[t0 + 1:t0 + 1 + T, 5:]
    x_trj = orc.rollout(sys_o, x0, u_trj)
    du = 0.05 * np.random.default_rng(11).normal(size=(T, 300, 2))
    At, Bt, ct = orc.zero_order_B_decoupled(sys_o, x_trj, u_trj, du)
    Q = np.diag(pack([5, 5, 50], [0, 0]))
    Qd, R = Q.copy(), 10.0 * np.eye(2)
    xd = np.tile(x_trj[-1] + pack([0.3, 0.2, 0.3], [0, 0]), (T + 1, 1))
    xb = pack([0.5, 0.5, 0.5], [0.04, 0.04])
    rows = orc.quasistatic_bounds(x_trj, idx, np.array([-xb, xb]), None, np.array([-np.ones(2) * 0.03, np.ones(2) * 0.03]))
    rows_d = [dev.to_dev(r) if np.isfinite(r).any() else None for r in rows]
    prob = [dev.to_dev(a) for a in (At, Bt, ct, Q, Qd, R, xd, x0)]
    dm = sys_d.dm()
    ref = dm.quasistatic_box_descent(*prob, *rows_d, solver=1, rho=100.0, relax=1.6, max_iter=40000, eps=1e-10)
    iref = ref["info"].cpu().numpy()
    assert iref[0] == 0 and iref[2] == 0, iref
    ur, xr = ref["u_new"].cpu().numpy(), ref["x_new"].cpu().numpy()
    assert np.isclose(np.abs(ur - xr[:-1, idx]).max(), 0.03, atol=1e-7)                      # the rate box binds
    assert np.abs(xr[1:, idx] - x_trj[1:, idx]).max() > 0.04 - 1e-3                          # and the trust region
    for rho0 in (1.0, 100.0):
        o = dm.quasistatic_box_descent(*prob, *rows_d, solver=1, rho=rho0, relax=1.6, max_iter=5000, eps=1e-8,
                                       adaptive_rho=True)
        info, adapt = o["info"].cpu().numpy(), o["adapt"].cpu().numpy()
        print("rho0 %g: info %s, %d factorisations, final rho %.4g" % (rho0, info, adapt[0], adapt[1]))
        assert info[0] == 0 and info[2] == 0, info
        report("u_new vs fixed rho = 100, rho0 %g" % rho0, o["u_new"].cpu().numpy(), ur, 1e-6)
        report("x_new vs fixed rho = 100, rho0 %g" % rho0, o["x_new"].cpu().numpy(), xr, 1e-6)
        report("cost, rho0 %g" % rho0, o["cost"].item() / ref["cost"].item(), 1.0, 1e-6)
    with pytest.raises(ValueError, match="solver must be 1"):
        dm.quasistatic_box_descent(*prob, None, None, None, None, rows_d[4], rows_d[5], solver=3, adaptive_rho=True)


# ------------------------------------------------------------------------------------ (d): the hard bicycle curve
def test_irs_lqr_exact_on_bicycle_hard_follows_the_reference_curve(amd, golden_dir):
    """(d): IrsLqrExact on bicycle_hard (examples/problems.py: T = 100, qp_adaptive_rho = True, every other QP setting
    at its default), iterate(1): two descents, against the first three entries of the reference's result file.  The
    margin is the one test_bicycle_exact_csv_end_to_end gives the easy twin (the reference's curve carries OSQP's
    1e-3 accuracy); the oracle's own distances are 6.6e-4 and 6.9e-4.  Cut from iterate(2): a descent of this problem
    takes 4 - 6.5 s on the device (120 000 - 180 000 ADMM iterations: the script's +-1e4 placeholders are finite, so
    every component carries a penalty term), and three took 17 s; the third (entry 3, margin 0.03) was at 5.8e-3 with
    every tail converged when measured that way."""
    from examples.problems import bicycle_hard
    gold = np.loadtxt(os.path.join(golden_dir, "bicycle_hard_exact.csv"))
    assert gold.shape == (27,)
    sysd, p, _, _, _ = bicycle_hard()
    assert p.qp_adaptive_rho is True and not hasattr(p, "qp_rho")
    sol = amd.IrsLqrExact(sysd, p)
    sol.verbose = False
    assert sol.T == 100
    calls = []
    dm, orig = sol._dm, sol._dm.tvlqr_box_descent

    def spy(*args, **kw):
        o = orig(*args, **kw)
        calls.append((kw.get("adaptive_rho"), o))
        return o

    dm.tvlqr_box_descent = spy
    try:
        sol.iterate(1)
    finally:
        del dm.tvlqr_box_descent
    rel = [abs(c - g) / g for c, g in zip(sol.cost_lst, gold)]
    print("cost_lst %s\ngolden   %s\nrelative distance %s" % (sol.cost_lst, list(gold[:3]), rel))
    for flag, o in calls:
        print("bounded descent: info %s, adapt %s" % (o["info"].cpu().numpy(), o["adapt"].cpu().numpy()))
    assert len(sol.cost_lst) == 3
    assert sol.cost_lst[0] == pytest.approx(gold[0], rel=1e-12)
    assert rel[1] < 0.012 and rel[2] < 0.012
    # every descent used the bounded kernel, in its adaptive form, and converged on every tail
    assert len(calls) == 2
    for flag, o in calls:
        assert flag is True
        info = o["info"].cpu().numpy()
        assert info[0] == 0 and info[2] == 0, info
        assert o["adapt"][0].item() >= 1 and o["adapt"][1].item() > 0
    assert sol._last["box_adapt"] is calls[-1][1]["adapt"]
