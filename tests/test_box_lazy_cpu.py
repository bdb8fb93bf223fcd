"""Lazily enforced bounds of the bounded TV-LQR, without a GPU: the NumPy twin of the rule
(tests/helpers/admm_lazy_twin.py, built on the oracle's factor / solve alone) on the T = 25 bicycle whose "no bound"
entries are the scripts' finite +-1e4 -- the set it ends with, the iterations it saves, its exactness against the
+-inf statement and the QP's KKT conditions -- on a bound that starts to bind in the middle of a descent, and with the
adaptive penalty on top; the three C-ABI entries refuse bad arguments before any HIP call; the Python defaults."""
import ctypes
import os

import numpy as np
import pytest

from oracle import irs_oracle as orc
from tests.helpers.admm_adaptive_twin import local_descent_box_adaptive
from tests.helpers.admm_lazy_twin import LazyBoxAdmm, local_descent_box_lazy
from tests.test_box_adaptive_cpu import BIKE, ONE, PH_PARAMS, PLANAR_HAND, kkt25_problem

RELAX = 1.6                     # DeviceModel's default
STEER, ACCEL, SPEED = 4, 5, 3   # components of [x (5) | u (2)]: x[4], u[0], x[3]
SPEED_BOUND = 2.039             # tail 0's plan peaks at 2.0356, the realised trajectory without the bound at 2.0422


def placeholders(b):
    """The scripts' way to say "no bound": +-1e4 in place of +-inf."""
    return np.where(np.isfinite(b), b, np.sign(b) * 1e4)


@pytest.fixture(scope="module")
def prob():
    """The problem of kkt25_problem (steer 0.3 and accel 2.0 bind) stated three ways -- +-inf, +-1e4 placeholders, and
    the placeholders with the speed bound -- and the descents every test below shares, computed once."""
    p = kkt25_problem()
    s = orc.BicycleOracle(0.1)
    box_inf = (p["xlo"], p["xhi"], p["ulo"], p["uhi"])
    box = tuple(placeholders(b) for b in box_inf)
    late = [b.copy() for b in box]
    late[0][SPEED], late[1][SPEED] = -SPEED_BOUND, SPEED_BOUND
    args = (s, p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"], p["xd"])
    kw = dict(rho=10.0, max_iter=5000, eps=1e-8, relax=RELAX)
    p.update(box_inf=box_inf, box=box, late=tuple(late), args=args, kw=kw)
    p["lazy"] = local_descent_box_lazy(*args, *box, **kw)
    p["inf"] = local_descent_box_adaptive(*args, *box_inf, adaptive=False, **kw)
    p["all"] = local_descent_box_adaptive(*args, *box, adaptive=False, **kw)     # every finite bound penalised
    return p


def test_placeholder_descent_enforces_only_what_binds(prob):
    x_new, u_new, iters, failed, events, final, adm = prob["lazy"]
    _, u_inf, _, failed_inf, _ = prob["inf"]
    _, _, iters_all, failed_all, _ = prob["all"]
    print("lazy: %d iterations, worst tail %d, events %s, final set %s, %d factorisations; all enforced: %d iterations, "
          "worst tail %d; |u_new - u_new(+-inf)| %.2e" % (sum(iters), max(iters), events, np.flatnonzero(final),
                                                           adm.factorisations, sum(iters_all), max(iters_all),
                                                           np.abs(u_new - u_inf).max()))
    assert not failed and not failed_inf and not failed_all
    assert sorted(np.flatnonzero(final)) == [STEER, ACCEL]
    assert len(events) == 1 and adm.factorisations == 2
    assert np.abs(u_new - u_inf).max() < 1e-9
    assert 5 * sum(iters) <= sum(iters_all)


def test_placeholder_first_tail_is_kkt_certified_against_the_full_box(prob):
    p = prob
    adm = LazyBoxAdmm(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], *p["box"], 10.0)
    zx, zu, _, it, conv = adm.solve(p["xd"], p["x0"], 0, None, 20000, 1e-10, RELAX)
    assert conv and sorted(np.flatnonzero(adm.set)) == [STEER, ACCEL]
    res = orc.qp_box_kkt_residuals(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"], p["xd"], *p["box"], zx, zu)
    print("%d iterations; KKT (dyn, box, stat, sign) %s" % (it, res))
    r_dyn, r_box, r_stat, sign_bad = res
    assert r_dyn < 1e-10 and r_box < 1e-8 and r_stat < 1e-7 and sign_bad < 1e-7
    assert (np.abs(zx[:, 4]) > 0.3 - 1e-6).sum() > 5 and (np.abs(zu[:, 0]) > 2 - 1e-6).sum() > 2


def test_a_bound_that_binds_late_is_activated_at_that_tail(prob):
    p = prob
    start = np.zeros(7, int)
    start[[STEER, ACCEL]] = 1
    x_new, u_new, iters, failed, events, final, _ = local_descent_box_lazy(*p["args"], *p["late"], enforced=start,
                                                                           **p["kw"])
    _, u_all, _, failed_all, _ = local_descent_box_adaptive(*p["args"], *p["late"], adaptive=False, **p["kw"])
    dist = np.abs(u_new - u_all).max()
    print("events %s, final set %s, max |speed| %.10f, |u_new - u_new(all enforced)| %.2e, %d iterations"
          % (events, np.flatnonzero(final), np.abs(x_new[:, 3]).max(), dist, sum(iters)))
    assert not failed and not failed_all
    assert len(events) == 1 and events[0][0] >= 1 and events[0][1] == (SPEED,)
    assert final[SPEED] and sorted(np.flatnonzero(final)) == [SPEED, STEER, ACCEL]
    assert np.abs(x_new[:, 3]).max() <= SPEED_BOUND + 1e-8
    assert dist < 1e-6


@pytest.mark.parametrize("rho0", [0.1, 1000.0])
def test_lazy_with_the_adaptive_penalty_reaches_the_certified_solution(prob, rho0):
    """The certified solution: the +-inf statement at fixed rho = 10, eps = 1e-10 (the `fixed` of
    test_box_adaptive_cpu.py's kkt25, whose KKT residuals test_twin_converges_.. checks)."""
    p = prob
    mats = (p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"])
    F = orc.tvlqr_box_factor(*mats, *p["box_inf"], 10.0)
    fx, fu, _, it_f = orc.tvlqr_box_solve(F, *mats[:5], p["xd"], p["x0"], 0, *p["box_inf"], None, 20000, 1e-10)
    assert it_f < 20000
    adm = LazyBoxAdmm(*mats, *p["box"], rho0, adaptive=True)
    zx, zu, _, it, conv = adm.solve(p["xd"], p["x0"], 0, None, 20000, 1e-10, RELAX)
    print("rho0 %g: %d iterations, %d factorisations, final rho %g, events %s" % (rho0, it, adm.factorisations, adm.rho,
                                                                                  adm.events))
    assert conv and sorted(np.flatnonzero(adm.set)) == [STEER, ACCEL]
    assert adm.factorisations > 1 + len(adm.events)            # two decades off: the penalty has to move too
    assert np.abs(zu - fu).max() < 1e-6 and np.abs(zx - fx).max() < 1e-6


# ---- the three lazy entries: refused before any HIP call ------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from irs_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def _calls(lib):
    """name -> call(settings, ...) of the three entries, each with otherwise valid arguments (no workspace, no set)."""
    from irs_mpc_amd._lib import dbl_array
    bike, ph = dbl_array([0.1]), dbl_array(PH_PARAMS)

    def descent(st, ws=(None, 0)):
        return lib.irs_tvlqr_box_descent_lazy(BIKE, bike, 1, 10, *[ONE] * 6, 0.5, *[ONE] * 6, st, ONE, ONE, ONE, None,
                                              *ws, None, None, None)

    def solve(st, ws=(None, 0)):
        return lib.irs_tvlqr_box_solve_lazy(BIKE, bike, 1, 10, *[ONE] * 6, 0.5, ONE, ONE, 0, ONE, ONE, None, None, None,
                                            None, st, ONE, ONE, ONE, None, *ws, None, None, None)

    def quasi(st, ws=(None, 0), solver=1, T=10):
        return lib.irs_quasistatic_box_descent_lazy(PLANAR_HAND, ph, 12, T, *[ONE] * 8, None, None, ONE, ONE, None, None,
                                                    solver, st, ONE, ONE, None, ONE, None, *ws, None, None, None)

    return dict(descent=descent, solve=solve, quasi=quasi)


def _settings(**kw):
    from irs_mpc_amd._lib import admm_settings
    base = dict(rho=10.0, relax=1.6, max_iter=100, eps=1e-8, adaptive=False)
    base.update(kw)
    return ctypes.byref(admm_settings(**base))


@pytest.mark.parametrize("entry", ["descent", "solve", "quasi"])
def test_lazy_entries_refuse_bad_arguments_without_gpu(lib, entry):
    call = _calls(lib)[entry]
    assert call(None) == -1 and b"settings" in lib.irs_last_error()                       # NULL settings
    assert entry.encode() in lib.irs_last_error() and b"_lazy" in lib.irs_last_error()
    assert call(_settings(rho=0.0)) == -1 and b"ADMM parameter" in lib.irs_last_error()
    assert call(_settings(adaptive=True, trigger=1.0)) == -1 and b"adaptive" in lib.irs_last_error()
    # a workspace that is too small: 256-byte aligned, one byte
    if entry == "quasi":
        T = 100                                 # beyond the on-chip horizon: this entry takes the workspace then only
        assert lib.irs_quasistatic_descent_workspace_bytes(PLANAR_HAND, T, 1) > 1
        assert call(_settings(), ws=(256, 1), T=T) == -4
    else:
        assert call(_settings(), ws=(256, 1)) == -4
    assert b"workspace" in lib.irs_last_error()


@pytest.mark.parametrize("solver", [0, 2, 3, 7])
def test_quasistatic_lazy_entry_is_the_admm_alone(lib, solver):
    assert _calls(lib)["quasi"](_settings(), solver=solver) == -1
    assert b"solver must be 1" in lib.irs_last_error()


def test_python_layers_carry_the_flag_and_default_to_off():
    import inspect

    import irs_mpc_amd as amd
    from irs_mpc_amd import device, tv_lqr
    for fn in (device.DeviceModel.tvlqr_box_descent, device.DeviceModel.tvlqr_box_solve,
               device.DeviceModel.quasistatic_box_descent):
        par = inspect.signature(fn).parameters
        assert par["lazy_bounds"].default is False and par["enforced"].default is None
    par = inspect.signature(tv_lqr.solve_tvlqr).parameters["lazy_bounds"]
    assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY
    assert amd.IrsLqrParameters().qp_lazy_bounds is False
    assert amd.IrsLqrQuasistaticParameters().qp_lazy_bounds is False
    for script in ("run.py", "run_quasistatic.py"):
        assert "--lazy-bounds" in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                    "examples", script)).read()


def test_batched_quasistatic_class_refuses_the_flag():
    """IrsLqrQuasistaticBatch descends by solver 3's method, which has no penalty term to keep off a component: refused
    before the device is touched."""
    import irs_mpc_amd as amd
    from examples.run_quasistatic import problem
    T = 10
    q_dynamics, x0, u0, Q_dict, Qd_dict, R_dict, xd = problem(T, 0.1)
    ps = []
    for b in range(2):
        p = amd.IrsLqrQuasistaticParameters()
        p.Q_dict, p.Qd_dict, p.R_dict = Q_dict, Qd_dict, R_dict
        p.x0, p.x_trj_d, p.u_trj_0, p.T = x0, xd, u0, T
        p.u_bounds_abs = np.array([-np.ones(4) * 0.05, np.ones(4) * 0.05])
        p.sampling, p.std_u_initial, p.num_samples = (lambda u_initial, it: u_initial), np.ones(4) * 0.3, 512
        p.gradient_mode, p.publish_every_iteration, p.device_rng_seed = "exact", False, 7 + b
        ps.append(p)
    ps[1].qp_lazy_bounds = True
    with pytest.raises(NotImplementedError, match="qp_lazy_bounds"):
        amd.IrsLqrQuasistaticBatch(q_dynamics, ps)
