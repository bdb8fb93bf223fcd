"""Batched quasistatic descent, the part that needs no GPU: the new C entries are exported and bound, the workspace
query follows the one planner, argument errors come back as status codes before anything is dereferenced, and
IrsLqrQuasistaticBatch refuses parameter lists it cannot run as one launch -- naming the field -- before it touches
the device."""
import copy
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANAR_HAND, BOX_PIVOT, PENDULUM = 4, 5, 0
PH = [0.1, 10.0, 1.0, 0.25, 0.5, 50.0, 25.0, 0.3, 0.2, 0.05, 0.1, 50.0]      # planar-hand constants (12)
INVALID, UNSUPPORTED, WORKSPACE = -1, -3, -4
NEW = ("irs_quasistatic_descent_batch_workspace_bytes", "irs_quasistatic_box_descent_batch",
       "irs_quasistatic_bound_rows_batch")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from irs_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from irs_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "irs_hip.h")).read()
    for s in NEW:
        assert s + "(" in header, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s
    assert lib.irs_abi_version() == 1


def round256(v):
    return (v + 255) // 256 * 256


def test_batch_workspace_follows_the_planner(lib):
    from irs_mpc_amd._lib import BOX_ACTIVE_SET_MFMA
    for model, T_on, T_off in ((PLANAR_HAND, 50, 60), (BOX_PIVOT, 80, 130)):
        # on chip (the planner says TilesLds: the single query is 0 and the LDS size is within the budget)
        assert 0 < lib.irs_quasistatic_box_lds_bytes(model, T_on, 3) <= 160 * 1024 - 512
        assert lib.irs_quasistatic_descent_workspace_bytes(model, T_on, 3) == 0
        for B in (1, 8, 300):
            assert lib.irs_quasistatic_descent_batch_workspace_bytes(model, T_on, B) == 0
        # beyond the LDS horizon: B slices of the single-problem records, each rounded up to 256 bytes
        single = lib.irs_quasistatic_descent_workspace_bytes(model, T_off, 3)
        assert single > 0
        for B in (1, 2, 64):
            assert lib.irs_quasistatic_descent_batch_workspace_bytes(model, T_off, B) == B * round256(single)
        assert lib.irs_box_horizon_limit(model, BOX_ACTIVE_SET_MFMA) > T_off          # no cap, no second budget
    # a model without the tile form; nonsense sizes
    assert lib.irs_quasistatic_descent_batch_workspace_bytes(PENDULUM, 50, 8) == 0
    assert lib.irs_quasistatic_descent_batch_workspace_bytes(PLANAR_HAND, 0, 8) == 0
    assert lib.irs_quasistatic_descent_batch_workspace_bytes(PLANAR_HAND, 60, 0) == 0


def descent_batch(lib, model=PLANAR_HAND, params=PH, T=10, B=3, u=True, du=False, half=False, ws=None, ws_bytes=0):
    from irs_mpc_amd._lib import dbl_array
    one = 256       # any non-null, 256-aligned address: validation happens before anything is dereferenced
    p = dbl_array(params)
    u_lo, u_hi = (one, None if half else one) if u else (None, None)
    du_lo, du_hi = (one, one) if du else (None, None)
    return lib.irs_quasistatic_box_descent_batch(model, p, len(params), T, B, one, one, one, one, one, one, one, one,
                                                 u_lo, u_hi, du_lo, du_hi, 100, 1e-9, one, one, one, one, one,
                                                 ws, ws_bytes, None)


def test_batch_descent_argument_errors_without_gpu(lib):
    assert descent_batch(lib, B=0) == INVALID
    assert descent_batch(lib, B=-2) == INVALID
    assert b"irs_quasistatic_box_descent_batch" in lib.irs_last_error()
    assert descent_batch(lib, T=0) == INVALID
    assert descent_batch(lib, u=True, du=True) == INVALID              # both bound pairs
    assert descent_batch(lib, u=False, du=False) == INVALID            # neither
    assert descent_batch(lib, half=True) == INVALID                    # half a pair
    assert descent_batch(lib, params=PH[:5]) == INVALID                # wrong number of model constants
    assert descent_batch(lib, model=PENDULUM, params=[0.05]) == UNSUPPORTED   # no tile form
    assert descent_batch(lib, model=99) == UNSUPPORTED
    # beyond the LDS horizon: no workspace, one that is too small, one that is misaligned
    need = lib.irs_quasistatic_descent_batch_workspace_bytes(PLANAR_HAND, 60, 3)
    assert descent_batch(lib, T=60) == WORKSPACE
    assert descent_batch(lib, T=60, ws=256, ws_bytes=need - 1) == WORKSPACE
    assert descent_batch(lib, T=60, ws=264, ws_bytes=need) == INVALID
    # a forced workspace at an on-chip horizon must hold the records too
    assert descent_batch(lib, T=10, ws=256, ws_bytes=64) == WORKSPACE


def test_bound_rows_argument_errors_without_gpu(lib):
    one = 256
    assert lib.irs_quasistatic_bound_rows_batch(7, 4, 10, 0, one, one, one, 0, 0, one, one, None) == INVALID
    assert lib.irs_quasistatic_bound_rows_batch(7, 4, 0, 3, one, one, one, 0, 0, one, one, None) == INVALID
    assert lib.irs_quasistatic_bound_rows_batch(7, 4, 10, 3, None, one, one, 0, 0, one, one, None) == INVALID
    assert lib.irs_quasistatic_bound_rows_batch(7, 4, 10, 3, one, one, None, 0, 1, one, one, None) == INVALID
    assert lib.irs_quasistatic_bound_rows_batch(7, 4, 10, 3, one, one, one, 0, 1, None, one, None) == INVALID


# ---- the class: what it refuses, before the device is touched -------------------------------------------------------
def sampling(u_initial, it):
    return u_initial / (it ** 0.8)


def make_params(B=3, T=10):
    import irs_mpc_amd as amd
    from examples.run_quasistatic import problem
    q_dynamics, x0, u0, Q_dict, Qd_dict, R_dict, xd = problem(T, 0.1)
    ps = []
    for b in range(B):
        p = amd.IrsLqrQuasistaticParameters()
        p.Q_dict, p.Qd_dict, p.R_dict = Q_dict, Qd_dict, R_dict
        p.x0, p.x_trj_d, p.u_trj_0, p.T = x0, xd, u0, T
        p.u_bounds_abs = np.array([-np.ones(4) * 0.05, np.ones(4) * 0.05])
        p.sampling, p.std_u_initial, p.num_samples = sampling, np.ones(4) * 0.3, 512
        p.gradient_mode, p.publish_every_iteration, p.device_rng_seed = "zero_order_B", False, 7 + b
        ps.append(p)
    return q_dynamics, ps


def test_exported():
    import irs_mpc_amd as amd
    from irs_mpc_amd import all as amd_all
    assert amd_all.IrsLqrQuasistaticBatch is amd.IrsLqrQuasistaticBatch


@pytest.mark.parametrize("field,value", [
    ("T", 12), ("gradient_mode", "first_order"), ("decouple_AB", False), ("num_samples", 100),
    ("sampling", lambda u, it: u), ("Q_dict", "scaled"), ("Qd_dict", "scaled"), ("R_dict", "scaled"),
    ("qp_max_iter", 77), ("qp_eps", 1e-6), ("qp_solver", 3), ("qp_rho", 1.0)])
def test_disagreeing_parameters_raise_value_error_naming_the_field(field, value):
    import irs_mpc_amd as amd
    q_dynamics, ps = make_params()
    if value == "scaled":
        value = {k: 2.0 * np.asarray(v) for k, v in getattr(ps[1], field).items()}
    setattr(ps[1], field, value)
    with pytest.raises(ValueError, match=field):
        amd.IrsLqrQuasistaticBatch(q_dynamics, ps)


def test_mixed_bound_kinds_raise_value_error():
    import irs_mpc_amd as amd
    q_dynamics, ps = make_params()
    ps[2].u_bounds_rel, ps[2].u_bounds_abs = ps[2].u_bounds_abs, None
    with pytest.raises(ValueError, match="u_bounds"):
        amd.IrsLqrQuasistaticBatch(q_dynamics, ps)
    q_dynamics, ps = make_params()
    ps[1].x_bounds_abs = np.zeros((2, 7))
    with pytest.raises(ValueError, match="x_bounds_abs"):
        amd.IrsLqrQuasistaticBatch(q_dynamics, ps)
    with pytest.raises(ValueError, match="empty"):
        amd.IrsLqrQuasistaticBatch(q_dynamics, [])


def all_set(ps, field, value):
    for p in ps:
        setattr(p, field, copy.deepcopy(value))
    return ps


def test_unsupported_parameter_lists_raise_not_implemented():
    import irs_mpc_amd as amd
    q_dynamics, ps = make_params()
    for field, value in (("gradient_mode", "zero_order_AB"), ("decouple_AB", False), ("device_rng_seed", None),
                         ("x_bounds_abs", np.zeros((2, 7))), ("u_bounds_rel", np.array([-np.ones(4), np.ones(4)])),
                         ("qp_solver", 1), ("qp_solver", 2)):
        q_dynamics, ps = make_params()
        with pytest.raises(NotImplementedError):
            amd.IrsLqrQuasistaticBatch(q_dynamics, all_set(ps, field, value))
    # one problem without a seed is enough
    q_dynamics, ps = make_params()
    ps[1].device_rng_seed = None
    with pytest.raises(NotImplementedError, match="device_rng_seed"):
        amd.IrsLqrQuasistaticBatch(q_dynamics, ps)


def test_descent_failure_message():
    """One function turns a descent's (info row, smoothing-failed flag) into None or the single class's ValueError
    text; a failed smoothing solve wins over a failed QP, as in both loops."""
    from irs_mpc_amd.irs_lqr_quasistatic import MSG_QP, MSG_SMOOTH, descent_failure
    assert MSG_SMOOTH == "randomized-smoothing least squares is rank deficient"
    assert MSG_QP == "TV_LQR failed. Optimization problem is not solved."
    clean = np.array([0, 17, 0], np.int32)                # [1]: iterations used, not a failure
    assert descent_failure(clean, False) is None
    assert descent_failure(clean, np.bool_(True)) == MSG_SMOOTH
    for bad in ([3, 0, 0], [0, 5, 2], [1, 1, 1]):         # Hessian not PD at t = 2; two tails at max_iter; both
        assert descent_failure(np.array(bad, np.int32), False) == MSG_QP
        assert descent_failure(np.array(bad, np.int32), True) == MSG_SMOOTH
