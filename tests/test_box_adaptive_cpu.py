"""The adaptive ADMM penalty of the bounded TV-LQR, without a GPU: the NumPy twin of the rule
(tests/helpers/admm_adaptive_twin.py, built on the oracle's factor / solve) is certified by the QP's KKT conditions
from three starting penalties, and needs no more iterations than the fixed penalty on a tail of the hard bicycle
curve; the three C-ABI entries that take irs_admm_settings refuse bad arguments before any HIP call."""
import ctypes
import os

import numpy as np
import pytest

from oracle import irs_oracle as orc
from tests.helpers.admm_adaptive_twin import AdaptiveBoxAdmm, local_descent_box_adaptive

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bike_problem(T, goal=(3.0, 1.0, np.pi / 2, 0, 0)):
    Q, Qd, R = np.diag([5, 5, 3, 0.1, 0.1]), np.diag([50., 50, 30, 1, 1]), np.diag([1, 0.1])
    return Q, Qd, R, np.zeros(5), np.tile(np.array(goal), (T + 1, 1)), np.tile(np.array([0.1, 0.0]), (T, 1))


def kkt25_problem():
    """The problem of test_box_qp_solution_satisfies_kkt (tests/test_oracle_golden.py): T = 25, steer bound 0.3 and
    input bound 2.0, both active."""
    T = 25
    s = orc.BicycleOracle(0.1)
    Q, Qd, R, x0, xd, u0 = bike_problem(T)
    xlo = np.array([-np.inf] * 4 + [-0.3])
    ulo = np.array([-2.0, -np.inf])
    At, Bt, ct = orc.exact_TV(s, orc.rollout(s, x0, u0), u0)
    return dict(At=At, Bt=Bt, ct=ct, Q=Q, Qd=Qd, R=R, x0=x0, xd=xd, xlo=xlo, xhi=-xlo, ulo=ulo, uhi=-ulo)


@pytest.fixture(scope="module")
def kkt25():
    p = kkt25_problem()
    box = (p["xlo"], p["xhi"], p["ulo"], p["uhi"])
    F = orc.tvlqr_box_factor(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], *box, 10.0)
    zx, zu, _, it = orc.tvlqr_box_solve(F, p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["xd"], p["x0"], 0, *box, None,
                                        20000, 1e-10)
    assert it < 20000
    p["fixed"] = (zx.copy(), zu.copy())
    return p


@pytest.mark.parametrize("rho0", [0.1, 10.0, 1000.0])
def test_twin_converges_to_the_certified_solution_from_any_rho(kkt25, rho0):
    p = kkt25
    box = (p["xlo"], p["xhi"], p["ulo"], p["uhi"])
    adm = AdaptiveBoxAdmm(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], *box, rho0)
    zx, zu, _, it, conv = adm.solve(p["xd"], p["x0"], 0, None, 20000, 1e-10)
    print("rho0 %g: %d iterations, %d factorisations, final rho %g" % (rho0, it, adm.factorisations, adm.rho))
    assert conv
    assert (np.abs(zx[:, 4]) > 0.3 - 1e-6).sum() > 5 and (np.abs(zu[:, 0]) > 2 - 1e-6).sum() > 2
    r_dyn, r_box, r_stat, sign_bad = orc.qp_box_kkt_residuals(p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"],
                                                              p["xd"], *box, zx, zu)
    print("KKT: r_dyn %.2e r_box %.2e r_stat %.2e sign %.2e" % (r_dyn, r_box, r_stat, sign_bad))
    assert r_dyn < 1e-10 and r_box < 1e-8 and r_stat < 1e-7 and sign_bad < 1e-7
    fx, fu = p["fixed"]
    assert np.abs(zu - fu).max() < 1e-6 and np.abs(zx - fx).max() < 1e-6
    if rho0 != 10.0:
        assert adm.factorisations > 1          # two decades off: the rule has to move


def test_twin_needs_no_more_iterations_on_a_hard_bicycle_tail():
    """The first tail of descent 2 of the hard bicycle curve (T = 100, goal [-3, -1, -pi/2, 0, 0], steer bound pi/4,
    exact linearisation), descent 1 taken at eps = 1e-3: the adaptive rule from rho = 10 against fixed rho = 10, both
    at eps = 1e-8."""
    T = 100
    s = orc.BicycleOracle(0.1)
    Q, Qd, R, x0, xd, u0 = bike_problem(T, goal=(-3.0, -1.0, -np.pi / 2, 0, 0))
    xlo = np.array([-np.inf] * 4 + [-np.pi / 4])
    inf2 = np.full(2, np.inf)
    box = (xlo, -xlo, -inf2, inf2)
    x = orc.rollout(s, x0, u0)
    At, Bt, ct = orc.exact_TV(s, x, u0)
    x1, u1, iters = orc.local_descent_box(s, At, Bt, ct, Q, Qd, R, x0, xd, *box, rho=10.0, max_iter=5000, eps=1e-3)
    assert max(iters) < 5000
    At, Bt, ct = orc.exact_TV(s, x1, u1)
    fixed = AdaptiveBoxAdmm(At, Bt, ct, Q, Qd, R, *box, 10.0, adaptive=False)
    _, fu, _, it_fixed, conv_fixed = fixed.solve(xd, x0, 0, None, 5000, 1e-8)
    adm = AdaptiveBoxAdmm(At, Bt, ct, Q, Qd, R, *box, 10.0)
    _, au, _, it_adapt, conv_adapt = adm.solve(xd, x0, 0, None, 5000, 1e-8)
    print("fixed rho = 10: %d iterations; adaptive: %d iterations, %d factorisations, final rho %g; |du| %.2e"
          % (it_fixed, it_adapt, adm.factorisations, adm.rho, np.abs(au - fu).max()))
    assert conv_fixed and conv_adapt
    assert it_adapt <= it_fixed
    assert np.abs(au - fu).max() < 1e-6


def test_twin_fixed_form_is_the_oracles_descent():
    """adaptive=False, the twin's own loop around single iterations of the oracle: the oracle's descent, bit for bit."""
    p = kkt25_problem()
    s = orc.BicycleOracle(0.1)
    box = (p["xlo"], p["xhi"], p["ulo"], p["uhi"])
    args = (s, p["At"], p["Bt"], p["ct"], p["Q"], p["Qd"], p["R"], p["x0"], p["xd"]) + box
    xo, uo, iters_o = orc.local_descent_box(*args, rho=10.0, max_iter=5000, eps=1e-8)
    xt, ut, iters_t, failed, adm = local_descent_box_adaptive(*args, rho=10.0, max_iter=5000, eps=1e-8, adaptive=False)
    assert iters_t == iters_o and not failed and adm.factorisations == 1
    assert np.array_equal(xt, xo) and np.array_equal(ut, uo)


# ---- the three entries that take irs_admm_settings: refused before any HIP call -----------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from irs_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


ONE = 8     # any non-null address: validation happens before anything is dereferenced
BIKE, PENDULUM, PLANAR_HAND = 2, 0, 4
PH_PARAMS = [0.1, 10.0, 1.0, 0.25, 0.5, 50.0, 25.0, 0.3, 0.2, 0.05, 0.1, 50.0]


def _calls(lib):
    """(name, call(settings, **changes)) of the three entries, each with otherwise valid arguments."""
    from irs_mpc_amd._lib import dbl_array
    bike, pend, ph = dbl_array([0.1]), dbl_array([0.05]), dbl_array(PH_PARAMS)

    def descent(st, model=BIKE, params=bike, n_params=1, **_):
        return lib.irs_tvlqr_box_descent_set(model, params, n_params, 10, *[ONE] * 6, 0.5, *[ONE] * 6, st, ONE, ONE, ONE,
                                             None, None, 0, None)

    def solve(st, model=BIKE, params=bike, n_params=1, position=0, **_):
        return lib.irs_tvlqr_box_solve_set(model, params, n_params, 10, *[ONE] * 6, 0.5, ONE, ONE, position, ONE, ONE,
                                           None, None, None, None, st, ONE, ONE, ONE, None, None, 0, None)

    def quasi(st, model=PLANAR_HAND, params=ph, n_params=12, solver=1, **_):
        return lib.irs_quasistatic_box_descent_set(model, params, n_params, 10, *[ONE] * 8, None, None, ONE, ONE, None,
                                                   None, solver, st, ONE, ONE, None, ONE, None, None, 0, None)

    return dict(descent=descent, solve=solve, quasi=quasi), dict(pend=pend)


def _settings(**kw):
    from irs_mpc_amd._lib import admm_settings
    base = dict(rho=10.0, relax=1.6, max_iter=100, eps=1e-8, adaptive=True)
    base.update(kw)
    return ctypes.byref(admm_settings(**base))


@pytest.mark.parametrize("entry", ["descent", "solve", "quasi"])
def test_settings_entries_refuse_bad_arguments_without_gpu(lib, entry):
    from irs_mpc_amd import _lib
    assert _lib.AdmmSettings().check_every == 0 and _lib.ADMM_CHECK_EVERY > 0
    call = _calls(lib)[0][entry]
    assert call(None) == -1 and b"settings" in lib.irs_last_error()                       # NULL settings
    for bad in (dict(rho=0.0), dict(rho=-1.0), dict(relax=0.0), dict(relax=2.0), dict(relax=-0.5), dict(max_iter=0),
                dict(eps=0.0)):
        assert call(_settings(**bad)) == -1, bad
        assert b"ADMM parameter" in lib.irs_last_error()
    for bad in (dict(check_every=0), dict(check_every=-3), dict(trigger=1.0), dict(trigger=0.5), dict(max_refactor=-1)):
        assert call(_settings(**bad)) == -1, bad
        assert b"adaptive" in lib.irs_last_error()
    # the rule's constants are not read with adaptive == 0 -- but then the settings pass, so no call is made here


def test_settings_entries_refuse_a_model_without_the_form(lib):
    calls, p = _calls(lib)
    # an unknown model; the pendulum has no position-controlled form
    assert calls["descent"](_settings(), model=99) == -3
    assert calls["solve"](_settings(), model=99) == -3
    assert calls["solve"](_settings(), model=PENDULUM, params=p["pend"], n_params=1, position=1) == -3
    assert b"position controlled" in lib.irs_last_error()
    assert calls["quasi"](_settings(), model=PENDULUM, params=p["pend"], n_params=1) == -3
    assert b"position controlled" in lib.irs_last_error()
    # a parameter vector of the wrong length
    assert calls["descent"](_settings(), n_params=3) == -1


@pytest.mark.parametrize("solver", [0, 2, 3, 7])
def test_quasistatic_settings_entry_is_the_admm_alone(lib, solver):
    calls, _ = _calls(lib)
    assert calls["quasi"](_settings(), solver=solver) == -1
    assert b"solver must be 1" in lib.irs_last_error()


def test_python_layers_carry_the_flag():
    """The keyword on every layer that reaches the kernel, the parameter objects' field, and the example that sets it."""
    import inspect

    import irs_mpc_amd as amd
    from irs_mpc_amd import device, tv_lqr
    from irs_mpc_amd.irs_lqr_quasistatic import QP_DEFAULTS, QP_FIELDS
    for fn in (device.DeviceModel.tvlqr_box_descent, device.DeviceModel.tvlqr_box_solve,
               device.DeviceModel.quasistatic_box_descent):
        assert inspect.signature(fn).parameters["adaptive_rho"].default is False
    par = inspect.signature(tv_lqr.solve_tvlqr).parameters["adaptive_rho"]
    assert par.default is False and par.kind is inspect.Parameter.KEYWORD_ONLY
    assert amd.IrsLqrParameters().qp_adaptive_rho is False
    assert amd.IrsLqrQuasistaticParameters().qp_adaptive_rho is False
    assert QP_FIELDS == ("qp_solver", "qp_rho", "qp_max_iter", "qp_eps") and len(QP_DEFAULTS) == 4
    src = open(os.path.join(ROOT, "examples", "problems.py")).read()
    assert "qp_adaptive_rho = True" in src.split("def bicycle_hard")[1].split("\ndef ")[0]


def test_batched_quasistatic_class_refuses_the_flag():
    """IrsLqrQuasistaticBatch descends by solver 3's method, which has no penalty to adapt: refused before the device is
    touched."""
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
    ps[1].qp_adaptive_rho = True
    with pytest.raises(NotImplementedError, match="qp_adaptive_rho"):
        amd.IrsLqrQuasistaticBatch(q_dynamics, ps)
