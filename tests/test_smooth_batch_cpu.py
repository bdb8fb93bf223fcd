"""Batched sample pass (irs_smooth_rng_batch), the part that needs no GPU: the three entries are declared, exported
and bound, the workspace query is B slices of the single-problem layout, every argument error comes back as its status
code before anything is dereferenced, and IrsLqrQuasistaticBatch accepts `batched_sample_pass` without changing what it
refuses.  The entry serves the uniform-geometry kernel (the exact planar hand's u-only modes); the models of the general
kernel -- box pivoting among them -- are refused as unsupported, and their size query is 0."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PENDULUM, PLANAR_HAND, BOX_PIVOT, PLANAR_HAND_EXACT = 0, 4, 5, 8
ZERO_ORDER_AB, FIRST_ORDER, ZERO_ORDER_B = 0, 1, 2
PH = [0.1, 10.0, 1.0, 0.25, 0.5, 50.0, 25.0, 0.3, 0.2, 0.05, 0.1, 50.0]      # planar-hand constants (12)
INVALID, UNSUPPORTED, WORKSPACE = -1, -3, -4
NEW = ("irs_smooth_batch_workspace_bytes", "irs_smooth_batch_workspace_init", "irs_smooth_rng_batch")


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


@pytest.mark.parametrize("mode", [ZERO_ORDER_B, FIRST_ORDER])
def test_batch_workspace_is_B_slices_of_the_single_layout(lib, mode):
    model = PLANAR_HAND_EXACT
    for T, N in ((50, 10000), (80, 6250), (4, 100)):
        single = lib.irs_smooth_workspace_bytes(model, mode, T, N)
        assert single > 0
        for B in (1, 2, 64, 512):
            assert lib.irs_smooth_batch_workspace_bytes(model, mode, T, N, B) == B * round256(single), (T, N, B)
        for B in (0, -1):
            assert lib.irs_smooth_batch_workspace_bytes(model, mode, T, N, B) == 0


def test_batch_workspace_is_zero_for_what_is_not_served(lib, monkeypatch):
    # the general kernel's models: box pivoting, the planar hand with projected sweeps -- and the exact planar hand
    # itself once IRS_UG=0 (read per call) sends it to the general kernel
    for mode in (ZERO_ORDER_B, FIRST_ORDER):
        for T, N in ((50, 10000), (80, 6250), (4, 100)):
            assert lib.irs_smooth_workspace_bytes(BOX_PIVOT, mode, T, N) > 0
            for B in (1, 2, 64, 512):
                assert lib.irs_smooth_batch_workspace_bytes(BOX_PIVOT, mode, T, N, B) == 0
                assert lib.irs_smooth_batch_workspace_bytes(PLANAR_HAND, mode, T, N, B) == 0
    monkeypatch.setenv("IRS_UG", "0")
    assert lib.irs_smooth_batch_workspace_bytes(PLANAR_HAND_EXACT, ZERO_ORDER_B, 50, 10000, 8) == 0
    monkeypatch.delenv("IRS_UG")
    assert lib.irs_smooth_batch_workspace_bytes(PLANAR_HAND_EXACT, ZERO_ORDER_B, 50, 10000, 8) > 0
    assert lib.irs_smooth_batch_workspace_bytes(PLANAR_HAND, ZERO_ORDER_AB, 50, 10000, 8) == 0
    assert lib.irs_smooth_batch_workspace_bytes(BOX_PIVOT, ZERO_ORDER_AB, 50, 10000, 8) == 0
    for mode in (ZERO_ORDER_B, FIRST_ORDER):
        assert lib.irs_smooth_batch_workspace_bytes(PENDULUM, mode, 50, 10000, 8) == 0        # an analytic model
        assert lib.irs_smooth_batch_workspace_bytes(99, mode, 50, 10000, 8) == 0
    assert lib.irs_smooth_batch_workspace_bytes(PLANAR_HAND, 7, 50, 10000, 8) == 0
    # nonsense sizes of a served model
    assert lib.irs_smooth_batch_workspace_bytes(PLANAR_HAND_EXACT, ZERO_ORDER_B, 4, 100, 8) > 0
    assert lib.irs_smooth_batch_workspace_bytes(PLANAR_HAND_EXACT, ZERO_ORDER_B, 0, 100, 8) == 0
    assert lib.irs_smooth_batch_workspace_bytes(PLANAR_HAND_EXACT, ZERO_ORDER_B, 4, 0, 8) == 0
    assert lib.irs_smooth_batch_workspace_bytes(PLANAR_HAND_EXACT, ZERO_ORDER_B, -3, 100, 8) == 0


ONE = 256       # any non-null, 256-aligned address: validation happens before anything is dereferenced


def rng_batch(lib, model=PLANAR_HAND_EXACT, params=PH, mode=ZERO_ORDER_B, T=10, N=512, B=3, n=7, m=4, x_stride=None,
              u_stride=None, null=None, ws=ONE, ws_bytes=None):
    from irs_mpc_amd._lib import dbl_array
    ptr = {k: ONE for k in ("x_trj", "u_trj", "std_u", "seed", "sums", "At", "Bt", "ct", "info")}
    if null is not None:
        ptr[null] = None
    if ws_bytes is None:
        ws_bytes = lib.irs_smooth_batch_workspace_bytes(model, mode, T, N, B)
    return lib.irs_smooth_rng_batch(model, dbl_array(params), len(params), mode, T, N, B, ptr["x_trj"],
                                    (T + 1) * n if x_stride is None else x_stride, ptr["u_trj"],
                                    T * m if u_stride is None else u_stride, ptr["std_u"], ptr["seed"], 1, ptr["sums"],
                                    ptr["At"], ptr["Bt"], ptr["ct"], ptr["info"], ws, ws_bytes, None)


def named(lib):
    return b"irs_smooth_rng_batch" in lib.irs_last_error()


def test_rng_batch_argument_errors_without_gpu(lib):
    for kw in (dict(B=0), dict(B=-2), dict(T=0), dict(N=0), dict(N=-5),
               dict(T=1025, B=1),                     # the single entry's cap: one slice's arrival counters
               dict(T=10, B=6554),                    # B T = 65540 rows > grid.y
               dict(T=1024, B=64),                    # 65536
               dict(x_stride=10 * 7 - 1), dict(u_stride=10 * 4 - 1), dict(x_stride=0), dict(u_stride=-40),
               dict(params=PH[:5]), dict(params=PH + [1.0])):
        assert rng_batch(lib, **kw) == INVALID, kw
        assert named(lib), (kw, lib.irs_last_error())
    for name in ("x_trj", "u_trj", "std_u", "seed", "sums", "At", "Bt", "ct", "info"):
        assert rng_batch(lib, null=name) == INVALID, name
        assert named(lib), name
    # (a slice's partial sums beyond the hand-off's 32-bit buffer size are refused too, but the planner caps a
    # timestep's workgroups at the compute units / T, so no (T, N) reaches that check)


BP = [0.1, 10.0, 1.0, 0.5, 0.5, 50.0, 0.1, 50.0]                             # box-pivoting constants (8)


def test_rng_batch_unsupported_without_gpu(lib, monkeypatch):
    for kw in (dict(mode=ZERO_ORDER_AB), dict(model=PLANAR_HAND, mode=ZERO_ORDER_AB),
               dict(model=PLANAR_HAND), dict(model=PLANAR_HAND, mode=FIRST_ORDER),             # the general kernel
               dict(model=BOX_PIVOT, params=BP, n=5, m=2), dict(model=BOX_PIVOT, params=BP, n=5, m=2, mode=FIRST_ORDER),
               dict(model=PENDULUM, params=[0.05], n=2, m=1), dict(model=PENDULUM, params=[0.05], n=2, m=1, mode=FIRST_ORDER),
               dict(model=99)):
        assert rng_batch(lib, ws_bytes=1 << 40, **kw) == UNSUPPORTED, kw
        assert named(lib), (kw, lib.irs_last_error())
    assert rng_batch(lib, mode=5) == INVALID and named(lib)
    need = lib.irs_smooth_batch_workspace_bytes(PLANAR_HAND_EXACT, ZERO_ORDER_B, 10, 512, 3)
    monkeypatch.setenv("IRS_UG", "0")                     # read per call: the general kernel would run
    assert rng_batch(lib, ws_bytes=need) == UNSUPPORTED and named(lib)


def test_device_model_reports_what_is_served(lib, monkeypatch):
    from irs_mpc_amd.device import DeviceModel
    hand, box = DeviceModel(PLANAR_HAND_EXACT, PH), DeviceModel(BOX_PIVOT, BP)
    assert hand.smooth_batch_supported(ZERO_ORDER_B) and hand.smooth_batch_supported(FIRST_ORDER)
    assert not hand.smooth_batch_supported(ZERO_ORDER_AB)
    assert not box.smooth_batch_supported(ZERO_ORDER_B) and not box.smooth_batch_supported(FIRST_ORDER)
    assert not DeviceModel(PENDULUM, [0.05]).smooth_batch_supported(FIRST_ORDER)
    monkeypatch.setenv("IRS_UG", "0")
    assert not hand.smooth_batch_supported(ZERO_ORDER_B)


def test_rng_batch_workspace_errors_without_gpu(lib):
    for model, mode in ((PLANAR_HAND_EXACT, ZERO_ORDER_B), (PLANAR_HAND_EXACT, FIRST_ORDER)):
        kw = dict(model=model, mode=mode)
        need = lib.irs_smooth_batch_workspace_bytes(model, mode, 10, 512, 3)
        assert need > 0
        assert rng_batch(lib, ws=None, **kw) == WORKSPACE and named(lib)
        assert rng_batch(lib, ws_bytes=need - 1, **kw) == WORKSPACE and named(lib)
        assert rng_batch(lib, ws_bytes=0, **kw) == WORKSPACE
        assert rng_batch(lib, ws=ONE + 8, **kw) == WORKSPACE and named(lib)          # not 256-byte aligned
        # two slices do not serve three problems
        assert rng_batch(lib, ws_bytes=lib.irs_smooth_batch_workspace_bytes(model, mode, 10, 512, 2), **kw) == WORKSPACE
    assert lib.irs_smooth_batch_workspace_init(None, 4096, None) == INVALID
    assert lib.irs_smooth_batch_workspace_init(ONE, 0, None) == INVALID


# ---- the class ------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("batched", [True, False])
def test_class_accepts_the_keyword_and_refuses_what_it_refused(batched):
    import irs_mpc_amd as amd
    q_dynamics, ps = make_params()
    ps[1].device_rng_seed = None
    with pytest.raises(NotImplementedError, match="device_rng_seed"):
        amd.IrsLqrQuasistaticBatch(q_dynamics, ps, batched_sample_pass=batched)
    q_dynamics, ps = make_params()
    ps[2].T = 12
    with pytest.raises(ValueError, match="T"):
        amd.IrsLqrQuasistaticBatch(q_dynamics, ps, batched_sample_pass=batched)
