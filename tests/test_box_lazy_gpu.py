"""Lazily enforced bounds of the bounded TV-LQR kernel (csrc/boxqp.hip, box_descent_kernel<.., LAZY = true>) on the GPU:
against its NumPy twin (tests/helpers/admm_lazy_twin.py), today's kernel and the QP's KKT certificate on the T = 25
bicycle whose "no bound" entries are the scripts' finite +-1e4, a bound that starts to bind in the middle of a descent,
records on chip == records in HBM bit for bit, the adaptive penalty on top, the position-controlled form, and
IrsLqrExact on the hard bicycle problem against the reference's result file."""
import os
import time

import numpy as np
import pytest
import torch

from oracle import irs_oracle as orc
from tests.helpers.admm_lazy_twin import LazyBoxAdmm, local_descent_box_lazy

pytestmark = pytest.mark.gpu

RELAX = 1.6                     # DeviceModel's default; the twin runs at the same value
STEER, ACCEL, SPEED = 4, 5, 3   # components of [x (5) | u (2)]: x[4], u[0], x[3]
SPEED_BOUND = 2.039             # tail 0's plan peaks at 2.0356, the realised trajectory without the bound at 2.0422
KW = dict(alpha_R=0.5, rho=10.0, max_iter=5000, eps=1e-8)


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


def cpu(o, *keys):
    return [o[k].cpu().numpy() for k in keys]


@pytest.fixture(scope="module")
def bike25(amd):
    """The problem of test_box_qp_solution_satisfies_kkt (T = 25, steer bound 0.3 and input bound 2.0, both active) with
    its infinite entries written as +-1e4 (`box`), the same with the speed bound (`late`), and the +-inf statement
    (`inf`), on the device and on the host; the twin's descents, computed once."""
    from irs_mpc_amd import device as dev
    T = 25
    s = orc.BicycleOracle(0.1)
    Q, Qd, R = np.diag([5, 5, 3, 0.1, 0.1]), np.diag([50., 50, 30, 1, 1]), np.diag([1, 0.1])
    x0, xd = np.zeros(5), np.tile(np.array([3.0, 1.0, np.pi / 2, 0, 0]), (T + 1, 1))
    u0 = np.tile(np.array([0.1, 0.0]), (T, 1))
    xlo, ulo = np.array([-np.inf] * 4 + [-0.3]), np.array([-2.0, -np.inf])
    inf = (xlo, -xlo, ulo, -ulo)
    box = tuple(np.where(np.isfinite(b), b, np.sign(b) * 1e4) for b in inf)
    late = [b.copy() for b in box]
    late[0][SPEED], late[1][SPEED] = -SPEED_BOUND, SPEED_BOUND
    At, Bt, ct = orc.exact_TV(s, orc.rollout(s, x0, u0), u0)
    args = (s, At, Bt, ct, Q, Qd, R, x0, xd)
    tkw = dict(max_iter=5000, eps=1e-8, relax=RELAX)
    start = np.zeros(7, np.int32)
    start[[STEER, ACCEL]] = 1
    keys = ("x_new", "u_new", "iters", "failed", "events", "set")
    twin = dict(box=dict(zip(keys, local_descent_box_lazy(*args, *box, rho=10.0, **tkw))),
                late=dict(zip(keys, local_descent_box_lazy(*args, *late, rho=10.0, enforced=start, **tkw))))
    for rho0 in (0.1, 1000.0):
        twin[rho0] = dict(zip(keys, local_descent_box_lazy(*args, *box, rho=rho0, adaptive=True, **tkw)))
    for k, tw in twin.items():
        assert not tw["failed"], k
    host = dict(At=At, Bt=Bt, ct=ct, Q=Q, Qd=Qd, R=R, xd=xd, x0=x0, box=box)

    def on_dev(b):
        return dict(vec=[dev.to_dev(v) for v in b],
                    rows=[dev.to_dev(np.tile(v, (rows, 1))) for v, rows in zip(b, (T + 1, T + 1, T, T))])

    return dict(T=T, host=host, dev=[dev.to_dev(a) for a in (At, Bt, ct, Q, Qd, R, xd, x0)], box=on_dev(box),
                late=on_dev(late), inf=on_dev(inf), start=start, twin=twin, dm=amd.BicycleDynamics(0.1).dm())


def test_lazy_descent_enforces_only_what_binds(bike25):
    """1: the placeholder case as a descent."""
    b, tw = bike25, bike25["twin"]["box"]
    o = b["dm"].tvlqr_box_descent(*b["dev"], *b["box"]["vec"], lazy_bounds=True, **KW)
    today = b["dm"].tvlqr_box_descent(*b["dev"], *b["box"]["vec"], **KW)             # every finite bound penalised
    today_inf = b["dm"].tvlqr_box_descent(*b["dev"], *b["inf"]["vec"], **KW)
    info, enforced, lazy, adapt = cpu(o, "info", "enforced", "lazy", "adapt")
    info_today, info_inf = today["info"].cpu().numpy(), today_inf["info"].cpu().numpy()
    print("lazy: info %s, enforced %s, lazy %s, adapt %s (twin: %d iterations, worst tail %d, events %s); today's "
          "kernel: info %s on +-1e4, %s on +-inf" % (info, enforced, lazy, adapt, sum(tw["iters"]), max(tw["iters"]),
                                                     tw["events"], info_today, info_inf))
    assert info[0] == 0 and info[2] == 0, info
    assert info_today[0] == 0 and info_today[2] == 0 and info_inf[0] == 0 and info_inf[2] == 0
    assert enforced.tolist() == [0, 0, 0, 0, 1, 1, 0] and enforced.dtype == np.int32
    assert lazy[0] == 1 and lazy[1] == tw["events"][0][0] == 0
    assert adapt[0] == 2 and adapt[1] == 10.0 and adapt[2] == lazy[2] >= info[1]
    report("u_new vs twin", o["u_new"].cpu().numpy(), tw["u_new"], 1e-6)
    report("x_new vs twin", o["x_new"].cpu().numpy(), tw["x_new"], 1e-6)
    report("u_new vs today's kernel on +-inf", o["u_new"].cpu().numpy(), today_inf["u_new"].cpu().numpy(), 1e-6)
    report("x_new vs today's kernel on +-inf", o["x_new"].cpu().numpy(), today_inf["x_new"].cpu().numpy(), 1e-6)
    assert 5 * info[1] <= info_today[1], (info[1], info_today[1])


def test_lazy_single_tail_is_kkt_certified_against_the_full_box(bike25):
    """2: tvlqr_box_solve(lazy_bounds=True): the oracle's KKT certificate against the full +-1e4 box."""
    b, h = bike25, bike25["host"]
    o = b["dm"].tvlqr_box_solve(*b["dev"], *b["box"]["rows"], lazy_bounds=True, **KW)
    info, enforced, lazy, xs, us = cpu(o, "info", "enforced", "lazy", "x_star", "u_star")
    assert info[0] == 0 and info[2] == 0, info
    res = orc.qp_box_kkt_residuals(h["At"], h["Bt"], h["ct"], h["Q"], h["Qd"], h["R"], h["x0"], h["xd"], *h["box"], xs, us)
    print("info %s, enforced %s, lazy %s; KKT (dyn, box, stat, sign) %s" % (info, enforced, lazy, res))
    r_dyn, r_box, r_stat, sign_bad = res
    assert r_dyn < 1e-10 and r_box < 1e-8 and r_stat < 1e-6 and sign_bad < 1e-7, res
    assert (np.abs(xs[:, 4]) > 0.3 - 1e-6).sum() > 5 and (np.abs(us[:, 0]) > 2 - 1e-6).sum() > 2   # both active
    assert enforced.tolist() == [0, 0, 0, 0, 1, 1, 0] and lazy[0] == 1 and lazy[1] == 0


def test_lazy_descent_activates_a_bound_that_binds_late(bike25):
    """3: the speed bound, not in the set the launch starts from, is met by a later tail's plan only."""
    b, tw = bike25, bike25["twin"]["late"]
    o = b["dm"].tvlqr_box_descent(*b["dev"], *b["late"]["vec"], lazy_bounds=True, enforced=b["start"], **KW)
    info, enforced, lazy, x_new = cpu(o, "info", "enforced", "lazy", "x_new")
    print("info %s, enforced %s, lazy %s (twin events %s), max |speed| %.10f" % (info, enforced, lazy, tw["events"],
                                                                                np.abs(x_new[:, 3]).max()))
    assert info[0] == 0 and info[2] == 0, info
    assert lazy[0] >= 1 and lazy[1] >= 1
    assert enforced[SPEED] == 1 and enforced[STEER] == 1 and enforced[ACCEL] == 1
    assert np.abs(x_new[:, 3]).max() <= SPEED_BOUND + 1e-8
    report("u_new vs twin", o["u_new"].cpu().numpy(), tw["u_new"], 1e-6)
    report("x_new vs twin", x_new, tw["x_new"], 1e-6)
    assert b["start"].tolist() == [0, 0, 0, 0, 1, 1, 0]                  # the caller's array is not written


def test_lazy_records_in_hbm_equal_on_chip(bike25):
    """4: with the records forced into the HBM workspace -- where an activation rewrites records the staging ring may
    hold -- the same bits as on chip, descent and single solve, cases 1 and 3."""
    b = bike25
    for case, start in (("box", None), ("late", b["start"])):
        kw = dict(lazy_bounds=True, enforced=start, **KW)
        on = b["dm"].tvlqr_box_descent(*b["dev"], *b[case]["vec"], **kw)
        hbm = b["dm"].tvlqr_box_descent(*b["dev"], *b[case]["vec"], records_in_hbm=True, **kw)
        assert on["lazy"][0].item() >= 1
        for k in ("x_new", "u_new", "info", "enforced", "lazy", "adapt"):
            assert torch.equal(on[k], hbm[k]), (case, k)
        on = b["dm"].tvlqr_box_solve(*b["dev"], *b[case]["rows"], **kw)
        hbm = b["dm"].tvlqr_box_solve(*b["dev"], *b[case]["rows"], records_in_hbm=True, **kw)
        for k in ("x_star", "u_star", "info", "enforced", "lazy", "adapt"):
            assert torch.equal(on[k], hbm[k]), (case, k)


def test_lazy_with_the_adaptive_penalty_matches_the_twin(bike25):
    """5: both on, from two penalties two decades off."""
    b = bike25
    for rho0 in (0.1, 1000.0):
        tw = b["twin"][rho0]
        kw = dict(KW, rho=rho0)
        o = b["dm"].tvlqr_box_descent(*b["dev"], *b["box"]["vec"], lazy_bounds=True, adaptive_rho=True, **kw)
        info, enforced, lazy, adapt = cpu(o, "info", "enforced", "lazy", "adapt")
        print("rho0 %g: info %s, enforced %s, lazy %s, adapt %s (twin: %d iterations, events %s)"
              % (rho0, info, enforced, lazy, adapt, sum(tw["iters"]), tw["events"]))
        assert info[0] == 0 and info[2] == 0, info
        report("u_new vs twin, rho0 %g" % rho0, o["u_new"].cpu().numpy(), tw["u_new"], 1e-6)
        report("x_new vs twin, rho0 %g" % rho0, o["x_new"].cpu().numpy(), tw["x_new"], 1e-6)
        assert enforced.tolist() == tw["set"].astype(int).tolist()
        assert adapt[0] > 1 + lazy[0]                                     # the penalty moved as well


def test_lazy_position_controlled_descent_matches_the_fixed_penalty(amd, golden_dir):
    """6: the box-pushing problem of test_adaptive_position_controlled_descent_matches_the_fixed_penalty (T = 10, a
    state trust region and a rate box that both bind), solver 1 lazy from rho = 100 against that test's reference
    (every bound enforced, fixed rho = 100, eps = 1e-10).  Components: [x (5) | u abs (2) | du (2)]."""
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
    o = dm.quasistatic_box_descent(*prob, *rows_d, solver=1, rho=100.0, relax=1.6, max_iter=5000, eps=1e-8,
                                   lazy_bounds=True)
    info, enforced, lazy, x_new, u_new = cpu(o, "info", "enforced", "lazy", "x_new", "u_new")
    print("info %s (reference %s), enforced [x | u abs | du] %s, lazy %s" % (info, iref, enforced, lazy))
    assert info[0] == 0 and info[2] == 0, info
    assert enforced.shape == (9,)
    report("u_new vs every bound enforced", u_new, ref["u_new"].cpu().numpy(), 1e-6)
    report("x_new vs every bound enforced", x_new, ref["x_new"].cpu().numpy(), 1e-6)
    report("cost", o["cost"].item() / ref["cost"].item(), 1.0, 1e-6)
    # what was dropped holds on the realised trajectory (row t of the x bounds: x_t, t >= 1; of the u bounds: u_t; of
    # the du bounds: u_t - u_{t-1}, u_{-1} = x_0[idx]).  1e-9: the rounding of the sums that form the rows
    x_lo, x_hi, u_lo, u_hi, d_lo, d_hi = rows
    steps = u_new - np.vstack([x0[idx], u_new[:-1]])
    for i in range(5):
        if not enforced[i]:
            assert (x_new[1:, i] >= x_lo[1:, i] - 1e-9).all() and (x_new[1:, i] <= x_hi[1:, i] + 1e-9).all(), i
    for j in range(2):
        if not enforced[5 + j]:
            assert (u_new[:, j] >= u_lo[:, j] - 1e-9).all() and (u_new[:, j] <= u_hi[:, j] + 1e-9).all(), j
        if not enforced[7 + j]:
            assert (steps[:, j] >= d_lo[:, j] - 1e-9).all() and (steps[:, j] <= d_hi[:, j] + 1e-9).all(), j
    with pytest.raises(ValueError, match="solver must be 1"):
        dm.quasistatic_box_descent(*prob, None, None, None, None, rows_d[4], rows_d[5], solver=3, lazy_bounds=True)


def test_irs_lqr_exact_on_bicycle_hard_with_lazy_bounds(amd, golden_dir):
    """7: IrsLqrExact on bicycle_hard (T = 100, steer bound pi / 4, every other bound the script's +-1e4) with
    qp_lazy_bounds on top of the problem's qp_adaptive_rho, iterate(1): two descents, against the first three entries of
    the reference's result file at the margins of test_irs_lqr_exact_on_bicycle_hard_follows_the_reference_curve."""
    from examples.problems import bicycle_hard
    gold = np.loadtxt(os.path.join(golden_dir, "bicycle_hard_exact.csv"))
    sysd, p, _, _, _ = bicycle_hard()
    assert p.qp_adaptive_rho is True and p.qp_lazy_bounds is False
    p.qp_lazy_bounds = True
    sol = amd.IrsLqrExact(sysd, p)
    sol.verbose = False
    assert sol.T == 100
    calls = []
    dm, orig = sol._dm, sol._dm.tvlqr_box_descent

    def spy(*args, **kw):
        t = time.perf_counter()
        o = orig(*args, **kw)
        torch.cuda.synchronize()
        calls.append((kw, o, time.perf_counter() - t))
        return o

    dm.tvlqr_box_descent = spy
    try:
        sol.iterate(1)
    finally:
        del dm.tvlqr_box_descent
    rel = [abs(c - g) / g for c, g in zip(sol.cost_lst, gold)]
    print("cost_lst %s\ngolden   %s\nrelative distance %s" % (sol.cost_lst, list(gold[:3]), rel))
    for kw, o, wall in calls:
        print("bounded descent: %.3f s, info %s, adapt %s, lazy %s, enforced %s (started from %s)"
              % (wall, *cpu(o, "info", "adapt", "lazy", "enforced"),
                 None if kw["enforced"] is None else kw["enforced"].cpu().numpy()))
    assert len(sol.cost_lst) == 3
    assert sol.cost_lst[0] == pytest.approx(gold[0], rel=1e-12)
    assert rel[1] < 0.012 and rel[2] < 0.012
    assert len(calls) == 2
    for kw, o, _ in calls:
        assert kw["lazy_bounds"] is True and kw["adaptive_rho"] is True
        info = o["info"].cpu().numpy()
        assert info[0] == 0 and info[2] == 0, info
        assert "lazy" in o and o["enforced"].shape == (7,)
    assert calls[0][0]["enforced"] is None and calls[1][0]["enforced"] is calls[0][1]["enforced"]
    assert sol._last["box_lazy"] is calls[-1][1]["lazy"]
