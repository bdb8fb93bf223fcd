"""Batched iRS-LQR for the analytic models, the part that needs no GPU: the new entries (irs_tvlqr_descent_batch,
irs_tvlqr_plan_within_bounds_batch, irs_smooth_rng_general_batch and its two workspace companions) are declared,
exported and bound; the workspace query is B slices of the single-problem layout and 0 for what is not served; every
refusal comes back as its status code, with the entry's name in irs_last_error, before anything is dereferenced;
irs_smooth_rng_batch still refuses the analytic models; and IrsLqrBatch refuses in its constructor what it does not
run."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PENDULUM, QUADROTOR, BICYCLE, THREE_CART, PLANAR_HAND, BOX_PIVOT, PLANAR_HAND_EXACT = 0, 1, 2, 3, 4, 5, 8
ZERO_ORDER_AB, FIRST_ORDER, ZERO_ORDER_B = 0, 1, 2
INVALID, UNSUPPORTED, WORKSPACE = -1, -3, -4
PH = [0.1, 10.0, 1.0, 0.25, 0.5, 50.0, 25.0, 0.3, 0.2, 0.05, 0.1, 50.0]      # planar-hand constants (12)
NEW = ("irs_tvlqr_descent_batch", "irs_tvlqr_plan_within_bounds_batch", "irs_smooth_general_batch_workspace_bytes",
       "irs_smooth_general_batch_workspace_init", "irs_smooth_rng_general_batch")
ONE = 256       # any non-null, 256-aligned address: validation happens before anything is dereferenced


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


@pytest.mark.parametrize("model", [PENDULUM, QUADROTOR, BICYCLE, THREE_CART])
@pytest.mark.parametrize("mode", [ZERO_ORDER_AB, FIRST_ORDER])
def test_workspace_is_B_slices_of_the_single_layout(lib, model, mode):
    for T, N in ((30, 10000), (50, 10000), (3, 2500), (4, 100)):
        single = lib.irs_smooth_workspace_bytes(model, mode, T, N)
        assert single > 0
        for B in (1, 2, 64, 512):
            assert lib.irs_smooth_general_batch_workspace_bytes(model, mode, T, N, B) == B * round256(single), (T, N, B)
        for B in (0, -1):
            assert lib.irs_smooth_general_batch_workspace_bytes(model, mode, T, N, B) == 0


def test_workspace_is_zero_for_what_is_not_served(lib):
    for mode in (ZERO_ORDER_AB, FIRST_ORDER, ZERO_ORDER_B):
        for model in (PLANAR_HAND, BOX_PIVOT, PLANAR_HAND_EXACT, 6, 7, 9, 10, 11, 99, -1):      # contact, unknown
            assert lib.irs_smooth_general_batch_workspace_bytes(model, mode, 30, 10000, 8) == 0, (model, mode)
    assert lib.irs_smooth_general_batch_workspace_bytes(PENDULUM, ZERO_ORDER_B, 30, 10000, 8) == 0
    assert lib.irs_smooth_general_batch_workspace_bytes(PENDULUM, 7, 30, 10000, 8) == 0
    assert lib.irs_smooth_general_batch_workspace_bytes(PENDULUM, ZERO_ORDER_AB, 0, 10000, 8) == 0
    assert lib.irs_smooth_general_batch_workspace_bytes(PENDULUM, ZERO_ORDER_AB, 30, 0, 8) == 0
    # the descent needs none, as before
    assert lib.irs_quasistatic_descent_batch_workspace_bytes(PENDULUM, 30, 8) == 0


# ---- irs_smooth_rng_general_batch -----------------------------------------------------------------------------------
def general_batch(lib, model=PENDULUM, params=(0.05,), mode=ZERO_ORDER_AB, T=10, N=512, B=3, n=2, m=1, x_stride=None,
                  u_stride=None, null=None, ws=ONE, ws_bytes=None):
    from irs_mpc_amd._lib import dbl_array
    ptr = {k: ONE for k in ("x_trj", "u_trj", "std_x", "std_u", "seed", "sums", "At", "Bt", "ct", "info")}
    if null is not None:
        ptr[null] = None
    if ws_bytes is None:
        ws_bytes = lib.irs_smooth_general_batch_workspace_bytes(model, mode, T, N, B)
    return lib.irs_smooth_rng_general_batch(model, dbl_array(list(params)), len(params), mode, T, N, B, ptr["x_trj"],
                                            (T + 1) * n if x_stride is None else x_stride, ptr["u_trj"],
                                            T * m if u_stride is None else u_stride, ptr["std_x"], ptr["std_u"],
                                            ptr["seed"], 1, ptr["sums"], ptr["At"], ptr["Bt"], ptr["ct"], ptr["info"], ws,
                                            ws_bytes, None)


def named(lib, entry):
    return entry.encode() in lib.irs_last_error()


def test_general_batch_argument_errors_without_gpu(lib):
    for kw in (dict(B=0), dict(B=-2), dict(T=0), dict(N=0), dict(N=-5),
               dict(T=1025, B=1),                     # the single entry's cap: one slice's arrival counters
               dict(T=10, B=6554),                    # B T = 65540 rows > grid.y
               dict(T=1024, B=64),                    # 65536
               dict(x_stride=10 * 2 - 1), dict(u_stride=10 * 1 - 1), dict(x_stride=0), dict(u_stride=-10),
               dict(params=()), dict(params=(0.05, 1.0)), dict(mode=5)):
        assert general_batch(lib, ws_bytes=1 << 40, **kw) == INVALID, kw
        assert named(lib, "irs_smooth_rng_general_batch"), (kw, lib.irs_last_error())
    for name in ("x_trj", "u_trj", "std_x", "std_u", "seed", "sums", "At", "Bt", "ct", "info"):
        assert general_batch(lib, null=name) == INVALID, name
        assert named(lib, "irs_smooth_rng_general_batch"), name


def test_general_batch_unsupported_without_gpu(lib):
    BP = [0.1, 10.0, 1.0, 0.5, 0.5, 50.0, 0.1, 50.0]                         # box-pivoting constants (8)
    for kw in (dict(model=PLANAR_HAND_EXACT, params=PH, n=7, m=4, mode=ZERO_ORDER_B),
               dict(model=PLANAR_HAND_EXACT, params=PH, n=7, m=4, mode=FIRST_ORDER),
               dict(model=PLANAR_HAND, params=PH, n=7, m=4), dict(model=BOX_PIVOT, params=BP, n=5, m=2),
               dict(model=BOX_PIVOT, params=BP, n=5, m=2, mode=ZERO_ORDER_B),
               dict(mode=ZERO_ORDER_B), dict(model=99), dict(model=11)):
        assert general_batch(lib, ws_bytes=1 << 40, **kw) == UNSUPPORTED, kw
        assert named(lib, "irs_smooth_rng_general_batch"), (kw, lib.irs_last_error())


def test_general_batch_workspace_errors_without_gpu(lib):
    from irs_mpc_amd import QuadrotorDynamics
    for model, params, n, m in ((PENDULUM, (0.05,), 2, 1), (QUADROTOR, QuadrotorDynamics(0.05).device_params(), 12, 4)):
        for mode in (ZERO_ORDER_AB, FIRST_ORDER):
            kw = dict(model=model, params=params, n=n, m=m, mode=mode)
            need = lib.irs_smooth_general_batch_workspace_bytes(model, mode, 10, 512, 3)
            assert need > 0
            assert general_batch(lib, ws=None, **kw) == WORKSPACE and named(lib, "irs_smooth_rng_general_batch")
            assert general_batch(lib, ws_bytes=need - 1, **kw) == WORKSPACE and named(lib, "irs_smooth_rng_general_batch")
            assert general_batch(lib, ws_bytes=0, **kw) == WORKSPACE
            assert general_batch(lib, ws=ONE + 8, **kw) == WORKSPACE and named(lib, "irs_smooth_rng_general_batch")
            two = lib.irs_smooth_general_batch_workspace_bytes(model, mode, 10, 512, 2)      # two slices, three problems
            assert general_batch(lib, ws_bytes=two, **kw) == WORKSPACE
    assert lib.irs_smooth_general_batch_workspace_init(None, 4096, None) == INVALID
    assert named(lib, "irs_smooth_general_batch_workspace_init")
    assert lib.irs_smooth_general_batch_workspace_init(ONE, 0, None) == INVALID


def test_rng_batch_still_refuses_the_analytic_models(lib):
    from irs_mpc_amd._lib import dbl_array
    from irs_mpc_amd.device import DeviceModel
    for mode in (ZERO_ORDER_AB, FIRST_ORDER, ZERO_ORDER_B):
        assert lib.irs_smooth_batch_workspace_bytes(PENDULUM, mode, 10, 512, 3) == 0
        rc = lib.irs_smooth_rng_batch(PENDULUM, dbl_array([0.05]), 1, mode, 10, 512, 3, ONE, 22, ONE, 10, ONE, ONE, 1, ONE,
                                      ONE, ONE, ONE, ONE, ONE, 1 << 40, None)
        assert rc == UNSUPPORTED and named(lib, "irs_smooth_rng_batch")
    pend = DeviceModel(PENDULUM, [0.05])
    assert not pend.smooth_batch_supported(ZERO_ORDER_AB) and not pend.smooth_batch_supported(FIRST_ORDER)
    assert pend.smooth_general_batch_supported(ZERO_ORDER_AB) and pend.smooth_general_batch_supported(FIRST_ORDER)
    assert not pend.smooth_general_batch_supported(ZERO_ORDER_B)
    assert not DeviceModel(PLANAR_HAND_EXACT, PH).smooth_general_batch_supported(FIRST_ORDER)


# ---- irs_tvlqr_descent_batch, irs_tvlqr_plan_within_bounds_batch ----------------------------------------------------
DESCENT_PTRS = ("At", "Bt", "ct", "Q", "Qd", "R", "xd_trj", "x0", "K", "k", "x_new", "u_new", "cost", "info")


def descent_batch(lib, model=PENDULUM, params=(0.05,), T=5, B=3, null=None):
    from irs_mpc_amd._lib import dbl_array
    p = {k: ONE for k in DESCENT_PTRS}
    if null is not None:
        p[null] = None
    return lib.irs_tvlqr_descent_batch(model, dbl_array(list(params)), len(params), T, B, p["At"], p["Bt"], p["ct"], p["Q"],
                                       p["Qd"], p["R"], 0.5, p["xd_trj"], p["x0"], p["K"], p["k"], p["x_new"], p["u_new"],
                                       p["cost"], p["info"], None)


def test_descent_batch_refusals_without_gpu(lib):
    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(params=()), dict(params=(0.05, 0.1))):
        assert descent_batch(lib, **kw) == INVALID, kw
        assert named(lib, "irs_tvlqr_descent_batch"), (kw, lib.irs_last_error())
    for name in DESCENT_PTRS:
        assert descent_batch(lib, null=name) == INVALID, name
        assert named(lib, "irs_tvlqr_descent_batch"), name
    for kw in (dict(model=99), dict(model=11), dict(model=-1), dict(model=PLANAR_HAND, params=PH),
               dict(model=PLANAR_HAND_EXACT, params=PH), dict(model=BOX_PIVOT, params=[0.1, 10.0, 1.0, 0.5, 0.5, 50.0, 0.1, 50.0])):
        assert descent_batch(lib, **kw) == UNSUPPORTED, kw
        assert named(lib, "irs_tvlqr_descent_batch"), (kw, lib.irs_last_error())


PLAN_PTRS = ("At", "Bt", "ct", "K", "k", "x_new", "xlo", "xhi", "ulo", "uhi", "flag")


def plan_batch(lib, n=2, m=1, T=5, B=3, null=None):
    p = {k: ONE for k in PLAN_PTRS}
    if null is not None:
        p[null] = None
    return lib.irs_tvlqr_plan_within_bounds_batch(n, m, T, B, *[p[k] for k in PLAN_PTRS], None)


def test_plan_batch_refusals_without_gpu(lib):
    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(n=0), dict(n=33), dict(m=0), dict(m=17)):
        assert plan_batch(lib, **kw) == INVALID, kw
        assert named(lib, "irs_tvlqr_plan_within_bounds_batch"), (kw, lib.irs_last_error())
    for name in PLAN_PTRS:
        assert plan_batch(lib, null=name) == INVALID, name
        assert named(lib, "irs_tvlqr_plan_within_bounds_batch"), name


# ---- the class: what the constructor refuses, before any GPU is touched ----------------------------------------------
def make_problems(B=3, T=10, N=2500):
    import irs_mpc_amd as amd
    from examples.problems import pendulum
    ps, smps = [], []
    for b in range(B):
        system, p, smoothing, _, _ = pendulum(T)
        p.x0 = np.array([0.1 * b, 0.0])
        ps.append(p)
        smps.append(amd.GaussianSmoothing(smoothing["std_x"], smoothing["std_u"], N, power=smoothing["power"], seed=3 + b))
    return system, ps, smps


def test_class_refusals_without_gpu():
    import irs_mpc_amd as amd
    from irs_mpc_amd.all import IrsLqrBatch
    assert IrsLqrBatch is amd.IrsLqrBatch
    system, ps, smps = make_problems()
    with pytest.raises(ValueError, match="order"):
        amd.IrsLqrBatch(system, ps, "second_order")
    with pytest.raises(ValueError, match="empty"):
        amd.IrsLqrBatch(system, [], "exact")
    # a host closure cannot be drawn on the device
    closure = lambda x, u, it: (np.zeros((4, 2)), np.zeros((4, 1)))      # noqa: E731
    for order in ("zero_order", "first_order"):
        with pytest.raises(NotImplementedError, match="drawn on the host"):
            amd.IrsLqrBatch(system, ps, order, [smps[0], closure, smps[2]])
        with pytest.raises(ValueError, match="sampling_list"):
            amd.IrsLqrBatch(system, ps, order, smps[:2])
        with pytest.raises(ValueError, match="sampling_list"):
            amd.IrsLqrBatch(system, ps, order)
    # what the one launch shares: T, Q, N
    system, ps, smps = make_problems()
    ps[2].u_trj_initial = ps[2].u_trj_initial[:-1]
    with pytest.raises(ValueError, match="T"):
        amd.IrsLqrBatch(system, ps, "exact")
    system, ps, smps = make_problems()
    ps[1].Q = 2.0 * ps[1].Q
    with pytest.raises(ValueError, match=r"\.Q differs"):
        amd.IrsLqrBatch(system, ps, "exact")
    system, ps, smps = make_problems()
    smps[1].num_samples = 1000
    with pytest.raises(ValueError, match="num_samples"):
        amd.IrsLqrBatch(system, ps, "zero_order", smps)
    system, ps, smps = make_problems()
    smps[2].power = 0.8
    with pytest.raises(ValueError, match="power"):
        amd.IrsLqrBatch(system, ps, "first_order", smps)
    # the bounded descent's extensions, and systems without a device functor
    for flag in ("qp_adaptive_rho", "qp_lazy_bounds"):
        system, ps, smps = make_problems()
        setattr(ps[0], flag, True)
        with pytest.raises(NotImplementedError, match=flag):
            amd.IrsLqrBatch(system, ps, "exact")
    from examples.torch_systems import TorchPendulum
    system, ps, smps = make_problems()
    with pytest.raises(NotImplementedError, match="TorchDynamicalSystem"):
        amd.IrsLqrBatch(TorchPendulum(0.05), ps, "exact")
