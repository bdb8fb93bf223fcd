"""Batched bounded TV-LQR, the part that needs no GPU: irs_tvlqr_box_descent_batch and its workspace query are
declared, exported and bound; the query is B slices of the rounded single-problem record size for the analytic models and
0 for what the batch does not serve; every argument error comes back as its status code, with the entry's name in
irs_last_error, before anything is dereferenced; and IrsLqrBatch(bounded=True) refuses in its constructor, before a GPU
is touched, settings the problems of a launch cannot share."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PENDULUM, QUADROTOR, BICYCLE, THREE_CART, PLANAR_HAND, BOX_PIVOT, PLANAR_HAND_EXACT = 0, 1, 2, 3, 4, 5, 8
BOX_ADMM = 0
INVALID, UNSUPPORTED, WORKSPACE = -1, -3, -4
PH = [0.1, 10.0, 1.0, 0.25, 0.5, 50.0, 25.0, 0.3, 0.2, 0.05, 0.1, 50.0]      # planar-hand constants (12)
BP = [0.1, 10.0, 1.0, 0.5, 0.5, 50.0, 0.1, 50.0]                             # box-pivoting constants (8)
ENTRY = "irs_tvlqr_box_descent_batch"
NEW = (ENTRY, "irs_tvlqr_box_descent_batch_workspace_bytes")
ONE = 256       # any non-null, 256-aligned address: validation happens before anything is dereferenced
REQUIRED = ("At", "Bt", "ct", "Q", "Qd", "R", "xd_trj", "x0", "xlo", "xhi", "ulo", "uhi", "x_new", "u_new", "info")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from irs_mpc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.load()


def analytic_params():
    from irs_mpc_amd import BicycleDynamics, PendulumDynamics, QuadrotorDynamics, ThreeCartDynamics
    return {PENDULUM: PendulumDynamics(0.05).device_params(), QUADROTOR: QuadrotorDynamics(0.05).device_params(),
            BICYCLE: BicycleDynamics(0.1).device_params(), THREE_CART: ThreeCartDynamics(0.05).device_params()}


def round256(v):
    return (v + 255) // 256 * 256


def named(lib):
    return ENTRY.encode() in lib.irs_last_error()


def test_both_symbols_are_declared_exported_and_bound(lib):
    from irs_mpc_amd import _lib
    header = open(os.path.join(ROOT, "include", "irs_hip.h")).read()
    for s in NEW:
        assert s + "(" in header, s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s


@pytest.mark.parametrize("model", [PENDULUM, QUADROTOR, BICYCLE, THREE_CART])
def test_workspace_is_B_rounded_single_record_sizes(lib, model):
    limit = lib.irs_box_horizon_limit(model, BOX_ADMM)
    assert limit > 0
    for T in (1, 6, 12, 100, limit):
        single = lib.irs_box_records_bytes(model, T, BOX_ADMM)
        assert single > 0
        for B in (1, 3, 64, 512):
            assert lib.irs_tvlqr_box_descent_batch_workspace_bytes(model, T, B) == B * round256(single), (T, B)
        for B in (0, -1):
            assert lib.irs_tvlqr_box_descent_batch_workspace_bytes(model, T, B) == 0
    for T in (0, -4, limit + 1, 10 * limit):
        assert lib.irs_tvlqr_box_descent_batch_workspace_bytes(model, T, 3) == 0, T


def test_workspace_is_zero_for_what_is_not_served(lib):
    for model in (PLANAR_HAND, BOX_PIVOT, PLANAR_HAND_EXACT, 6, 7, 9, 10, 11, 99, -1):      # contact, unknown
        assert lib.irs_tvlqr_box_descent_batch_workspace_bytes(model, 12, 3) == 0, model


def box_batch(lib, model=BICYCLE, params=None, T=12, B=3, null=None, rho=10.0, relax=1.6, max_iter=5000, eps=1e-8,
              ws=None, ws_bytes=0, cost=ONE, run_flag=None):
    from irs_mpc_amd._lib import dbl_array
    if params is None:
        params = analytic_params()[model]
    p = {k: ONE for k in REQUIRED}
    if null is not None:
        p[null] = None
    return lib.irs_tvlqr_box_descent_batch(model, dbl_array(list(params)), len(params), T, B, p["At"], p["Bt"], p["ct"],
                                           p["Q"], p["Qd"], p["R"], 0.5, p["xd_trj"], p["x0"], p["xlo"], p["xhi"],
                                           p["ulo"], p["uhi"], rho, relax, max_iter, eps, p["x_new"], p["u_new"], cost,
                                           p["info"], run_flag, ws, ws_bytes, None)


def test_argument_errors_without_gpu(lib):
    for kw in (dict(B=0), dict(B=-2), dict(T=0), dict(T=-1),
               dict(rho=0.0), dict(rho=-1.0), dict(relax=0.0), dict(relax=2.0), dict(max_iter=0), dict(eps=0.0),
               dict(params=()), dict(params=[0.1, 1.0, 2.0])):
        assert box_batch(lib, **kw) == INVALID, kw
        assert named(lib), (kw, lib.irs_last_error())
    for name in REQUIRED:
        assert box_batch(lib, null=name) == INVALID, name
        assert named(lib), (name, lib.irs_last_error())


def test_workspace_errors_without_gpu(lib):
    for model in (PENDULUM, QUADROTOR, BICYCLE, THREE_CART):
        need = lib.irs_tvlqr_box_descent_batch_workspace_bytes(model, 12, 3)
        two = lib.irs_tvlqr_box_descent_batch_workspace_bytes(model, 12, 2)
        assert need > two > 0
        for kw in (dict(ws=ONE, ws_bytes=need - 1), dict(ws=ONE, ws_bytes=two), dict(ws=ONE, ws_bytes=0),
                   dict(ws=ONE + 8, ws_bytes=need), dict(ws=ONE + 8, ws_bytes=1 << 40)):
            assert box_batch(lib, model=model, **kw) == WORKSPACE, (model, kw)
            assert named(lib), (model, kw, lib.irs_last_error())


def test_unsupported_without_gpu(lib):
    for kw in (dict(model=PLANAR_HAND, params=PH), dict(model=PLANAR_HAND_EXACT, params=PH),
               dict(model=BOX_PIVOT, params=BP), dict(model=99, params=[0.1]), dict(model=-1, params=[0.1])):
        for ws in (dict(), dict(ws=ONE, ws_bytes=1 << 40)):
            assert box_batch(lib, **kw, **ws) == UNSUPPORTED, (kw, ws)
            assert named(lib), (kw, lib.irs_last_error())


def test_horizon_refusals_are_the_single_entrys(lib):
    """No workspace at a horizon whose records do not fit LDS, and a horizon beyond the limit: IRS_ERR_UNSUPPORTED with
    the text irs_tvlqr_box_descent_wsx / _if give for the same model and horizon."""
    from irs_mpc_amd._lib import dbl_array
    quad = analytic_params()[QUADROTOR]
    limit = lib.irs_box_horizon_limit(QUADROTOR, BOX_ADMM)
    T_hbm = next(T for T in range(1, limit) if lib.irs_tvlqr_box_workspace_bytes(QUADROTOR, T, 0) > 0)
    a = [ONE] * 6
    for T, ws in ((T_hbm, None), (limit + 1, ONE)):
        assert box_batch(lib, model=QUADROTOR, T=T, ws=ws, ws_bytes=1 << 40 if ws else 0) == UNSUPPORTED
        batch_text = lib.irs_last_error()
        if ws is None:
            rc = lib.irs_tvlqr_box_descent_if(QUADROTOR, dbl_array(list(quad)), len(quad), T, *a, 0.5, ONE, ONE, ONE, ONE,
                                              ONE, ONE, 10.0, 1.6, 5000, 1e-8, ONE, ONE, ONE, ONE, None, None)
        else:
            rc = lib.irs_tvlqr_box_descent_wsx(QUADROTOR, dbl_array(list(quad)), len(quad), T, *a, 0.5, ONE, ONE, ONE, ONE,
                                               ONE, ONE, 10.0, 1.6, 5000, 1e-8, ONE, ONE, ONE, ONE, 1 << 40, None)
        assert rc == UNSUPPORTED
        assert lib.irs_last_error() == batch_text, (T, batch_text, lib.irs_last_error())


# ---- the class: what bounded=True refuses in the constructor, before any GPU is touched -------------------------------
def make_problems(B=3, T=10):
    from examples.problems import pendulum
    ps = []
    for b in range(B):
        system, p, _, _, _ = pendulum(T)
        p.x0 = np.array([0.1 * b, 0.0])
        ps.append(p)
    return system, ps


def test_class_refusals_without_gpu():
    import irs_mpc_amd as amd
    for field, value in (("qp_eps", 1e-6), ("qp_rho", 5.0), ("qp_max_iter", 100)):
        system, ps = make_problems()
        setattr(ps[1], field, value)
        with pytest.raises(ValueError, match=field):
            amd.IrsLqrBatch(system, ps, "exact", bounded=True)
    for flag in ("qp_adaptive_rho", "qp_lazy_bounds"):
        system, ps = make_problems()
        setattr(ps[2], flag, True)
        with pytest.raises(NotImplementedError, match=flag):
            amd.IrsLqrBatch(system, ps, "exact", bounded=True)
